// actor_critic.hip — the actor-critic (A2C / PPO) part of the device path: the sampling head of a vector step, the
// on-policy rollout window with its lambda-returns, the append that fills the window's rings from the fused acting step, and
// the loss with its gradients (include/mirl.h has the contracts).
// Each exists for a Discrete action space (Categorical head, one int32 per action) and for a Box one (Normal head, up to 16
// float32 components per action); what does not depend on the distribution is stated once and shared.
// All are latency-sized: a few thousand rows of at most 64 actions.  Plain C++, float64 inside, one rounding to
// float32 per output; no float atomics, every sum in a fixed order, so a rerun repeats the first run bit for bit.
#include "common.hpp"
#include "philox.hpp"
#include "ac_head.hpp"

namespace mirl {

// ---- 1. the sampling head ------------------------------------------------------------------------------------------
// Everything after the uniform is ac_head_row (ac_head.hpp): softmax pieces, inverse CDF (or the first maximum),
// log-probability of the chosen action — shared with the fused MLP acting step (csrc/act_mlp.hip).
__global__ __launch_bounds__(64) void k_actor_head_ac(int E, int A, const float* __restrict__ logits, long pitch,
                                                      const float* __restrict__ values, const float* __restrict__ u, int greedy,
                                                      int* __restrict__ actions, float* __restrict__ logp, float* __restrict__ values_out,
                                                      int out_pitch) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= E) return;
  float lp;
  actions[e] = ac_head_row(logits + (long)e * pitch, A, greedy ? 0.f : u[e], greedy, &lp);
  logp[(long)e * out_pitch] = lp;
  values_out[(long)e * out_pitch] = values[e];
}

// The same head drawing its own uniform: one Philox4x32-10 block per (step, env), the 24-bit uniform of k_actor_head
// (csrc/acting.hip).  The value is read with a pitch of its own: logits and value may be columns of one [E][A + 1] product.
__global__ __launch_bounds__(64) void k_actor_head_ac_rng(int E, int A, const float* __restrict__ logits, long pitch,
                                                          const float* __restrict__ values, long value_pitch, uint64_t rng_seed,
                                                          const uint64_t* __restrict__ rng_step, int greedy, int* __restrict__ actions,
                                                          float* __restrict__ logp, float* __restrict__ values_out, int out_pitch) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= E) return;
  float u = 0.f;
  if (!greedy) {
    uint32_t r[4];
    philox_4x32(rng_seed, *rng_step, (uint32_t)e, r);
    u = (float)(r[0] >> 8) * (1.0f / 16777216.0f);
  }
  float lp;
  actions[e] = ac_head_row(logits + (long)e * pitch, A, u, greedy, &lp);
  logp[(long)e * out_pitch] = lp;
  values_out[(long)e * out_pitch] = values[(long)e * value_pitch];
}

// ---- 1b. the Normal (continuous) head: independent Gaussians over a Box action, state-independent log-std ----------------
// (policies/torch/distributions/normal.py:9-36).  The pieces the head and the loss share, the SAME sequence of operations in
// both: component d of an action a (float32) under N(mean_d, exp(logstd_d)) contributes
//   -(a_d - mean_d)^2 / (2 exp(2 logstd_d)) - logstd_d - log(2 pi) / 2
// to the joint log-probability, the contributions added in ascending d and the sum rounded once to float32.
constexpr int kMaxBoxDims = 16;
constexpr double kHalfLog2Pi = 0.9189385332046727;      // log(2 pi) / 2, correctly rounded

__device__ inline double normal_log_prob_term(double a, double mean, double logstd) {
  const double diff = a - mean;
  return -(diff * diff) / (2.0 * exp(2.0 * logstd)) - logstd - kHalfLog2Pi;
}

// One thread per env.  a_d = float32(mean_d + exp(logstd_d) eps_d) with eps the caller's standard-normal draws (the kernel
// is deterministic); the log-probability is that of the ROUNDED action — torch evaluates log_prob of the sampled float32
// tensor, and the learner later sees that tensor.
__global__ __launch_bounds__(64) void k_actor_head_normal(int E, int D, const float* __restrict__ mean, long pitch,
                                                          const float* __restrict__ logstd, const float* __restrict__ values,
                                                          const float* __restrict__ eps, float* __restrict__ actions,
                                                          float* __restrict__ logp, float* __restrict__ values_out, int out_pitch) {
  const int e = blockIdx.x * 64 + threadIdx.x;
  if (e >= E) return;
  const float* m = mean + (long)e * pitch;
  double lp = 0.0;
  for (int d = 0; d < D; ++d) {
    const double ls = (double)logstd[d];
    const float a = (float)((double)m[d] + exp(ls) * (double)eps[(long)e * D + d]);
    actions[(long)e * D + d] = a;
    lp += normal_log_prob_term((double)a, (double)m[d], ls);
  }
  logp[(long)e * out_pitch] = (float)lp;
  values_out[(long)e * out_pitch] = values[e];
}

// ---- 2. the on-policy window ---------------------------------------------------------------------------------------
// One workgroup per (t, sequence): thread 0 walks the transition's return, all threads move its two observation rows.
struct WindowArgs {
  int T, B, E, cap, nstep_target;
  double gamma, lam;
  long obs_bytes;
  const int* plan;                 // [B][3]: env, ring slot of the sequence's first transition, 1 = that transition is the env's first ever
  const unsigned char* obs_ring;   // [cap][E][obs_bytes]: next_state of the transition
  const int* actions_ring;         // [cap][E][action_words]: opaque 4-byte words (one int32 action, or the float32 components of a Box one)
  const float* rewards_ring;
  const unsigned char* dones_ring;
  const float* logp_ring;          // [(slot E + env) pol_pitch]
  const float* values_ring;
  int pol_pitch;
  float *returns, *nsteps, *masks;
  int* actions;                    // [T B][action_words]
  float *logp, *values;
  unsigned char *states, *target_states;
  int vec16, action_words;
  // the recurrent state stored with each next_state (S = 0: none, the two older entries)
  int S;                           // float32 words per transition: hx, cx of every recurrent layer
  const float* state_ring;         // [cap][E][S]
  const float* initials_ring;      // [cap][E]: 1 = that next_state opens an episode
  float *states_state, *target_state;        // [T B][S]
  float *states_initials, *target_initials;  // [T B]
  int state_vec16;
};

// `width` bytes per access: 16 (the launcher saw 16-byte aligned bases and a row length that keeps every row aligned),
// 4 (float32 rows) or 1
__device__ inline void copy_row(unsigned char* __restrict__ dst, const unsigned char* __restrict__ src, long bytes, int width) {
  if (width == 16) {
    const uint4* s = (const uint4*)src;
    uint4* d = (uint4*)dst;
    for (long q = threadIdx.x; q < bytes / 16; q += blockDim.x) d[q] = s[q];
  } else if (width == 4) {
    const unsigned* s = (const unsigned*)src;
    unsigned* d = (unsigned*)dst;
    for (long q = threadIdx.x; q < bytes / 4; q += blockDim.x) d[q] = s[q];
  } else {
    for (long q = threadIdx.x; q < bytes; q += blockDim.x) dst[q] = src[q];
  }
}

__global__ __launch_bounds__(256) void k_online_window(WindowArgs a) {
  const int b = blockIdx.x % a.B, t = blockIdx.x / a.B;
  const int env = a.plan[3 * b], first = a.plan[3 * b + 1], own = a.plan[3 * b + 2];
  // fixed_target: no target looks past the window (history.py:187-190); the steps covered advance whatever the dones are
  const int want = min(a.nstep_target, a.T - t);
  const long out = (long)t * a.B + b;
  auto at = [&](int i) { return (long)((first + i) % a.cap) * a.E + env; };     // ring row of the sequence's transition i
  if (threadIdx.x == 0) {
    const long r0 = at(t);
    double ret = (double)a.rewards_ring[r0];
    float mask = a.dones_ring[r0] ? 0.f : 1.f;
    for (int k = 1; k < want; ++k) {
      const long rj = at(t + k);
      if (mask != 0.f) {
        const double v = (double)a.values_ring[rj * a.pol_pitch], r = (double)a.rewards_ring[rj];
        ret += (pow(a.gamma, (double)k) * pow(a.lam, (double)(k - 1))) * (v + a.lam * (r - v));
      }
      if (a.dones_ring[rj]) mask = 0.f;
    }
    a.returns[out] = (float)ret;
    a.nsteps[out] = (float)want;
    a.masks[out] = mask;
    for (int w = 0; w < a.action_words; ++w) a.actions[out * a.action_words + w] = a.actions_ring[r0 * a.action_words + w];
    a.logp[out] = a.logp_ring[r0 * a.pol_pitch];
    a.values[out] = a.values_ring[r0 * a.pol_pitch];
  }
  // the transition starts from the previous vector step's next_state (an env's very first one from its own) and its target is
  // the next_state of the last step it covers: the ring rows every block of a stored next_state — observation, recurrent
  // state, initials flag — is read from
  const long s_row = (t == 0 && own) ? at(0) : (long)((first + t - 1 + a.cap) % a.cap) * a.E + env;
  const long t_row = at(t + want - 1);
  copy_row(a.states + out * a.obs_bytes, a.obs_ring + s_row * a.obs_bytes, a.obs_bytes, a.vec16 ? 16 : 1);
  copy_row(a.target_states + out * a.obs_bytes, a.obs_ring + t_row * a.obs_bytes, a.obs_bytes, a.vec16 ? 16 : 1);
  if (a.S) {
    const long sb = (long)a.S * 4;
    const int width = a.state_vec16 ? 16 : 4;
    copy_row((unsigned char*)(a.states_state + out * a.S), (const unsigned char*)(a.state_ring + s_row * a.S), sb, width);
    copy_row((unsigned char*)(a.target_state + out * a.S), (const unsigned char*)(a.state_ring + t_row * a.S), sb, width);
    if (threadIdx.x == 0) {
      a.states_initials[out] = a.initials_ring[s_row];
      a.target_initials[out] = a.initials_ring[t_row];
    }
  }
}

// ---- 2b. appending one vector step to the rings the window reads ---------------------------------------------------------
// One workgroup per env.  The slot is (*head_word + k) mod cap: the word lives on the device, so a captured launch lands in
// the right slot at every ring position.  Nothing outside the slot is written, no atomics.
struct AppendArgs {
  int E, cap, k;
  const long long* head_word;
  long obs_bytes;
  const unsigned char* obs; const int* actions; const float* rewards; const unsigned char* dones;
  const float* policy; long policy_pitch;
  int S; const float* state; const float* initials;
  unsigned char* obs_ring; int* actions_ring; float* rewards_ring; unsigned char* dones_ring; float* policy_ring;
  float* state_ring; float* initials_ring;
  int obs_width, state_width;
};

__global__ __launch_bounds__(256) void k_online_append(AppendArgs a) {
  const int e = blockIdx.x;
  long long slot = (*a.head_word + (long long)a.k) % (long long)a.cap;
  if (slot < 0) slot += a.cap;
  const long row = (long)slot * a.E + e;
  copy_row(a.obs_ring + row * a.obs_bytes, a.obs + (long)e * a.obs_bytes, a.obs_bytes, a.obs_width);
  if (a.S) copy_row((unsigned char*)(a.state_ring + row * a.S), (const unsigned char*)(a.state + (long)e * a.S), (long)a.S * 4, a.state_width);
  if (threadIdx.x == 0) {
    a.actions_ring[row] = a.actions[e];
    a.rewards_ring[row] = a.rewards[e];
    a.dones_ring[row] = a.dones[e];
    a.policy_ring[2 * row] = a.policy[(long)e * a.policy_pitch];
    a.policy_ring[2 * row + 1] = a.policy[(long)e * a.policy_pitch + 1];
    if (a.S) a.initials_ring[row] = a.initials[e];
  }
}

// a launch of its own: no workgroup of an append launch can see the word move
__global__ void k_online_advance(long long* head_word, long long steps) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *head_word += steps;
}

// ---- 3. the loss ---------------------------------------------------------------------------------------------------
// ONE workgroup: thread i takes rows i, i + 1024, ... in ascending order into float64 accumulators, the workgroup adds
// them in a fixed tree.  M is a few thousand rows (16 envs x 128 steps), so one compute unit is enough and the whole
// loss — advantage statistics, forward, both gradients, the logged scalars — is one launch.
constexpr int kLossThreads = 1024;

__device__ inline double block_sum(double v, double* lds) {
  __syncthreads();
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int s = kLossThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) lds[threadIdx.x] += lds[threadIdx.x + s];
    __syncthreads();
  }
  return lds[0];
}

struct LossArgs {
  long M; int A;
  const float* logits; long pitch;
  const float* values; const int* actions; const float* targets; const float* acting_values; const float* old_log_probs;
  double vf_coef, entropy_factor, clip_value; int adv_norm;
  float* dlogits; long dpitch; float* dvalues; float* log_probs; float* stats;
};

// The parts of the loss that do not depend on the action distribution — stated once, used by the Categorical and the Normal
// kernel: the advantage statistics, a row's advantage, its action gain with the coefficient of the log-probability's
// gradient, its value terms, and the stats block.
struct AdvNorm { double mean, denom; };

__device__ inline AdvNorm advantage_stats(const float* __restrict__ targets, const float* __restrict__ acting_values, long M,
                                          int adv_norm, double invM, double* lds) {
  AdvNorm n;
  n.mean = 0.0; n.denom = 1.0;
  if (adv_norm) {
    // torch: (adv - adv.mean()) / (adv.std() + 1e-5), the unbiased std; two passes, the second on the centred values
    double s = 0.0;
    for (long i = threadIdx.x; i < M; i += kLossThreads) s += (double)targets[i] - (double)acting_values[i];
    n.mean = block_sum(s, lds) * invM;
    double q = 0.0;
    for (long i = threadIdx.x; i < M; i += kLossThreads) {
      const double c = ((double)targets[i] - (double)acting_values[i]) - n.mean;
      q += c * c;
    }
    n.denom = sqrt(block_sum(q, lds) / (double)(M - 1)) + 1e-5;
  }
  return n;
}

__device__ inline double row_advantage(const float* __restrict__ targets, const float* __restrict__ acting_values, long i,
                                       int adv_norm, const AdvNorm& n) {
  double adv = (double)targets[i] - (double)acting_values[i];
  if (adv_norm) adv = (adv - n.mean) / n.denom;
  return adv;
}

// gain_i and coef_i = d gain_i / d log-prob (before the 1 / M of the mean): A2C without old log-probabilities, else PPO's
// clipped surrogate
struct RowGain { double gain, coef; };

__device__ inline RowGain row_gain(float lp32, double adv, const float* __restrict__ old_log_probs, long i, double lo, double hi) {
  RowGain g;
  if (!old_log_probs) {
    g.gain = (double)lp32 * adv;
    g.coef = adv;
  } else {
    const double ratio = exp((double)lp32 - (double)old_log_probs[i]);
    const double s1 = ratio * adv, s2 = fmin(fmax(ratio, lo), hi) * adv;
    g.gain = fmin(s1, s2);
    // autograd: minimum() hands a tie half the gradient each way, clamp() passes it inside [lo, hi], bounds included
    const bool inside = ratio >= lo && ratio <= hi;
    const double share = inside ? 1.0 : (s1 < s2 ? 1.0 : (s1 == s2 ? 0.5 : 0.0));
    g.coef = share * (ratio * adv);
  }
  return g;
}

__device__ inline void write_stats(float* __restrict__ stats, double vf_coef, double entropy_factor, double gain, double vl,
                                   double ent, double val) {
  stats[0] = (float)(vf_coef * vl - gain - entropy_factor * ent);
  stats[1] = (float)vl;
  stats[2] = (float)(-gain);
  stats[3] = (float)ent;
  stats[4] = (float)val;
}

__global__ __launch_bounds__(kLossThreads) void k_ac_loss(LossArgs a) {
  __shared__ double lds[kLossThreads];
  const double invM = 1.0 / (double)a.M;
  const AdvNorm norm = advantage_stats(a.targets, a.acting_values, a.M, a.adv_norm, invM, lds);
  const double lo = 1.0 - a.clip_value, hi = 1.0 + a.clip_value;
  double s_gain = 0.0, s_vl = 0.0, s_ent = 0.0, s_val = 0.0;
  for (long i = threadIdx.x; i < a.M; i += kLossThreads) {
    const float* z = a.logits + i * a.pitch;
    const RowSoftmax r = row_softmax(z, a.A);
    const double logS = log(r.S);
    int act = a.actions[i];
    act = act < 0 ? 0 : (act >= a.A ? a.A - 1 : act);          // (an action outside [0, A) reads no memory outside the row)
    const float lp32 = row_log_prob(z, act, r, logS);
    if (a.log_probs) a.log_probs[i] = lp32;
    const double H = logS - r.W / r.S;                          // -sum_j p_j log p_j
    const double adv = row_advantage(a.targets, a.acting_values, i, a.adv_norm, norm);
    const RowGain rg = row_gain(lp32, adv, a.old_log_probs, i, lo, hi);
    const double gain = rg.gain, coef = rg.coef;
    const double t = (double)a.targets[i], v = (double)a.values[i];
    s_gain += gain;
    s_vl += (t - v) * (t - v);
    s_ent += H;
    s_val += v;
    a.dvalues[i] = (float)(a.vf_coef * (2.0 * (v - t)) * invM);
    float* g = a.dlogits + i * a.dpitch;
    const double w = coef * invM, we = a.entropy_factor * invM;
    for (int j = 0; j < a.A; ++j) {
      const double d = (double)z[j] - (double)r.zmax;
      const double p = exp(d) / r.S;
      double gj = -(w * ((j == act ? 1.0 : 0.0) - p));
      if (a.entropy_factor != 0.0) gj += we * (p * ((d - logS) + H));
      g[j] = (float)gj;
    }
  }
  const double gain = block_sum(s_gain, lds) * invM;
  const double vl = block_sum(s_vl, lds) * invM;
  const double ent = block_sum(s_ent, lds) * invM;
  const double val = block_sum(s_val, lds) * invM;
  if (threadIdx.x == 0) write_stats(a.stats, a.vf_coef, a.entropy_factor, gain, vl, ent, val);
}

// ---- 3b. the loss under the Normal head ----------------------------------------------------------------------------------
// The skeleton above with the Normal pieces of 1b in the softmax's place.  Per row: the joint log-probability of the stored
// float32 action (rounded once, then used as the float32 it is), and with s2_d = exp(2 logstd_d), diff_d = a_d - mean_d
//   d log-prob / d mean_d = diff_d / s2_d,        d log-prob / d logstd_d = diff_d^2 / s2_d - 1.
// The entropy of component d is 1/2 + log(2 pi) / 2 + logstd_d whatever the row.  The reference's evaluate_actions returns it
// un-summed, [M][D], and the trainer takes .mean() over all M D elements (a2c.py:113): the entropy term is the MEAN over the
// components, not their sum, and its gradient to logstd_d is 1 / D.  dlogstd is a reduction over the M rows: thread i adds
// its rows in ascending order into D float64 accumulators, the workgroup adds those in the fixed tree — no atomics.
struct NormalLossArgs {
  long M; int D;
  const float* mean; long pitch; const float* logstd;
  const float* values; const float* actions; const float* targets; const float* acting_values; const float* old_log_probs;
  double vf_coef, entropy_factor, clip_value; int adv_norm;
  float* dmean; long dpitch; float* dlogstd; float* dvalues; float* log_probs; float* stats;
};

__global__ __launch_bounds__(kLossThreads) void k_ac_loss_normal(NormalLossArgs a) {
  __shared__ double lds[kLossThreads];
  const double invM = 1.0 / (double)a.M;
  const AdvNorm norm = advantage_stats(a.targets, a.acting_values, a.M, a.adv_norm, invM, lds);
  const double lo = 1.0 - a.clip_value, hi = 1.0 + a.clip_value;
  double ent_sum = 0.0;
  for (int d = 0; d < a.D; ++d) ent_sum += (0.5 + kHalfLog2Pi) + (double)a.logstd[d];
  const double ent = ent_sum / (double)a.D;
  double s_gain = 0.0, s_vl = 0.0, s_val = 0.0;
  double acc[kMaxBoxDims];
#pragma unroll
  for (int d = 0; d < kMaxBoxDims; ++d) acc[d] = 0.0;
  for (long i = threadIdx.x; i < a.M; i += kLossThreads) {
    const float* m = a.mean + i * a.pitch;
    const float* act = a.actions + i * a.D;
    double lp = 0.0;
    for (int d = 0; d < a.D; ++d) lp += normal_log_prob_term((double)act[d], (double)m[d], (double)a.logstd[d]);
    const float lp32 = (float)lp;
    if (a.log_probs) a.log_probs[i] = lp32;
    const double adv = row_advantage(a.targets, a.acting_values, i, a.adv_norm, norm);
    const RowGain rg = row_gain(lp32, adv, a.old_log_probs, i, lo, hi);
    const double t = (double)a.targets[i], v = (double)a.values[i];
    s_gain += rg.gain;
    s_vl += (t - v) * (t - v);
    s_val += v;
    a.dvalues[i] = (float)(a.vf_coef * (2.0 * (v - t)) * invM);
    float* g = a.dmean + i * a.dpitch;
    const double w = rg.coef * invM;
#pragma unroll
    for (int d = 0; d < kMaxBoxDims; ++d) {
      if (d < a.D) {
        const double diff = (double)act[d] - (double)m[d], s2 = exp(2.0 * (double)a.logstd[d]);
        g[d] = (float)(-(w * (diff / s2)));
        acc[d] += -(w * ((diff * diff) / s2 - 1.0));
      }
    }
  }
  const double gain = block_sum(s_gain, lds) * invM;
  const double vl = block_sum(s_vl, lds) * invM;
  const double val = block_sum(s_val, lds) * invM;
#pragma unroll
  for (int d = 0; d < kMaxBoxDims; ++d) {
    if (d < a.D) {                                               // (uniform: every thread takes the same barriers)
      const double total = block_sum(acc[d], lds);
      if (threadIdx.x == 0) a.dlogstd[d] = (float)(total - a.entropy_factor / (double)a.D);
    }
  }
  if (threadIdx.x == 0) write_stats(a.stats, a.vf_coef, a.entropy_factor, gain, vl, ent, val);
}

}  // namespace mirl

extern "C" int mirl_actor_head_ac(int32_t E, int32_t A, const float* logits, int64_t pitch, const float* values, const float* u,
                                  int32_t greedy, int32_t* actions, float* action_log_probs, float* values_out, int32_t out_pitch,
                                  void* stream) {
  if (E < 1 || E > (1 << 24) || A < 1 || A > 64 || pitch < A || !logits || !values || (greedy != 0 && greedy != 1) || (!greedy && !u) ||
      !actions || !action_log_probs || !values_out || out_pitch < 1)
    return mirl::fail(MIRL_ERR_ARG, "bad actor_head_ac arguments (1 <= E <= 2^24, 1 <= A <= 64, pitch >= A, greedy 0 | 1, u unless greedy, "
                                    "out_pitch >= 1, no null operands)");
  mirl::ProfScope ps("k_actor_head_ac", (double)E * (A + 6) * 4.0, (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_actor_head_ac, dim3((E + 63) / 64), dim3(64), 0, (hipStream_t)stream, (int)E, (int)A, logits, (long)pitch, values, u,
                     (int)greedy, actions, action_log_probs, values_out, (int)out_pitch);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_actor_head_ac_rng(int32_t E, int32_t A, const float* logits, int64_t pitch, const float* values, int64_t value_pitch,
                                      uint64_t rng_seed, const uint64_t* rng_step, int32_t greedy, int32_t* actions,
                                      float* action_log_probs, float* values_out, int32_t out_pitch, void* stream) {
  if (E < 1 || E > (1 << 24) || A < 1 || A > 64 || pitch < A || value_pitch < 1 || !logits || !values || (greedy != 0 && greedy != 1) ||
      !rng_step || !actions || !action_log_probs || !values_out || out_pitch < 1)
    return mirl::fail(MIRL_ERR_ARG, "bad actor_head_ac_rng arguments (1 <= E <= 2^24, 1 <= A <= 64, pitch >= A, value_pitch >= 1, "
                                    "greedy 0 | 1, out_pitch >= 1, no null operands)");
  mirl::ProfScope ps("k_actor_head_ac_rng", (double)E * (A + 5) * 4.0, (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_actor_head_ac_rng, dim3((E + 63) / 64), dim3(64), 0, (hipStream_t)stream, (int)E, (int)A, logits, (long)pitch,
                     values, (long)value_pitch, rng_seed, rng_step, (int)greedy, actions, action_log_probs, values_out, (int)out_pitch);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

// the widest access both ends of a row copy allow: 16 bytes, 4 bytes, else single bytes
static int row_width(int64_t bytes, const void* a, const void* b) {
  if (bytes % 16 == 0 && mirl::aligned16(a, b)) return 16;
  if (bytes % 4 == 0 && (uintptr_t)a % 4 == 0 && (uintptr_t)b % 4 == 0) return 4;
  return 1;
}

extern "C" int mirl_online_append(int32_t E, int32_t cap, const int64_t* head_word, int32_t k, int64_t obs_bytes, const void* obs,
                                  const int32_t* actions, const float* rewards, const uint8_t* dones, const float* policy,
                                  int64_t policy_pitch, int32_t state_f32, const float* state, const float* initials, void* obs_ring,
                                  int32_t* actions_ring, float* rewards_ring, uint8_t* dones_ring, float* policy_ring,
                                  float* state_ring, float* initials_ring, void* stream) {
  if (E < 1 || E > (1 << 24) || cap < 1 || k < 0 || obs_bytes < 1 || policy_pitch < 2 || state_f32 < 0 || state_f32 > (1 << 20) ||
      (double)cap * (double)E * (double)obs_bytes >= 9.0e18 || !head_word || !obs || !actions || !rewards || !dones || !policy ||
      !obs_ring || !actions_ring || !rewards_ring || !dones_ring || !policy_ring)
    return mirl::fail(MIRL_ERR_ARG, "bad online_append arguments (1 <= E <= 2^24, cap >= 1, k >= 0, obs_bytes >= 1, policy_pitch >= 2, "
                                    "0 <= state_f32 <= 2^20, no null operands)");
  if (state_f32 && (!state || !initials || !state_ring || !initials_ring || (uintptr_t)state % 4 || (uintptr_t)state_ring % 4))
    return mirl::fail(MIRL_ERR_ARG, "bad online_append arguments (state_f32 > 0 needs state, initials and their rings, float32 blocks "
                                    "on 4-byte boundaries)");
  mirl::AppendArgs a;
  a.E = E; a.cap = cap; a.k = k; a.head_word = (const long long*)head_word; a.obs_bytes = obs_bytes;
  a.obs = (const unsigned char*)obs; a.actions = actions; a.rewards = rewards; a.dones = dones; a.policy = policy;
  a.policy_pitch = policy_pitch; a.S = state_f32; a.state = state; a.initials = initials;
  a.obs_ring = (unsigned char*)obs_ring; a.actions_ring = actions_ring; a.rewards_ring = rewards_ring; a.dones_ring = dones_ring;
  a.policy_ring = policy_ring; a.state_ring = state_ring; a.initials_ring = initials_ring;
  a.obs_width = row_width(obs_bytes, obs, obs_ring);
  a.state_width = state_f32 ? row_width((int64_t)state_f32 * 4, state, state_ring) : 4;
  mirl::ProfScope ps("k_online_append", (double)E * (2.0 * (double)obs_bytes + 8.0 * state_f32 + 40.0), (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_online_append, dim3((unsigned)E), dim3(256), 0, (hipStream_t)stream, a);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_online_advance(int64_t* head_word, int64_t steps, void* stream) {
  if (!head_word || steps < 0) return mirl::fail(MIRL_ERR_ARG, "bad online_advance arguments (head_word not null, steps >= 0)");
  mirl::ProfScope ps("k_online_advance", 16.0, (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_online_advance, dim3(1), dim3(1), 0, (hipStream_t)stream, (long long*)head_word, (long long)steps);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_actor_head_normal(int32_t E, int32_t D, const float* mean, int64_t pitch, const float* logstd, const float* values,
                                      const float* eps, float* actions, float* action_log_probs, float* values_out, int32_t out_pitch,
                                      void* stream) {
  if (E < 1 || E > (1 << 24) || D < 1 || D > mirl::kMaxBoxDims || pitch < D || !mean || !logstd || !values || !eps || !actions ||
      !action_log_probs || !values_out || out_pitch < 1)
    return mirl::fail(MIRL_ERR_ARG, "bad actor_head_normal arguments (1 <= E <= 2^24, 1 <= D <= 16, pitch >= D, out_pitch >= 1, "
                                    "no null operands)");
  mirl::ProfScope ps("k_actor_head_normal", (double)E * (3.0 * D + 3.0) * 4.0, (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_actor_head_normal, dim3((E + 63) / 64), dim3(64), 0, (hipStream_t)stream, (int)E, (int)D, mean, (long)pitch,
                     logstd, values, eps, actions, action_log_probs, values_out, (int)out_pitch);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

// the recurrent blocks of mirl_online_window_rec; the two older entries pass none (S = 0)
struct WindowState {
  int32_t S = 0;
  const float* state_ring = nullptr;
  const float* initials_ring = nullptr;
  float *states_state = nullptr, *target_state = nullptr, *states_initials = nullptr, *target_initials = nullptr;
};

// all three window entries: the protocol is stated once, mirl_online_window is action_words = 1, and both older entries S = 0
static int online_window(const char* name, int32_t T, int32_t B, int32_t E, int32_t cap, int32_t nstep_target, double gamma, double lam,
                         int64_t obs_bytes, int32_t action_words, const int32_t* plan, const void* obs_ring, const void* actions_ring,
                         const float* rewards_ring, const uint8_t* dones_ring, const float* logp_ring, const float* values_ring,
                         int32_t pol_pitch, float* returns, float* nsteps, float* target_masks, void* actions,
                         float* action_log_probs, float* values, void* states, void* target_states, const WindowState& rec, void* stream) {
  // (the plan's entries are device data: the caller keeps env in [0, E), the slot in [0, cap) and T + 1 <= cap steps behind them)
  if (T < 1 || B < 1 || E < 1 || cap < T || nstep_target < 1 || obs_bytes < 1 || pol_pitch < 1 || !(gamma >= 0.0) || !(lam >= 0.0) ||
      action_words < 1 || action_words > mirl::kMaxBoxDims ||
      (int64_t)T * B > (1 << 24) || (double)cap * (double)E * (double)obs_bytes >= 9.0e18 || !plan || !obs_ring || !actions_ring ||
      !rewards_ring || !dones_ring || !logp_ring || !values_ring || !returns || !nsteps || !target_masks || !actions ||
      !action_log_probs || !values || !states || !target_states)
    return mirl::fail(MIRL_ERR_ARG, std::string("bad ") + name + " arguments (T, B, E >= 1, cap >= T, nstep_target >= 1, obs_bytes >= 1, "
                                    "T B <= 2^24, 1 <= action_words <= 16, no null operands)");
  if (rec.S && (rec.S < 1 || rec.S > (1 << 20) || !rec.state_ring || !rec.initials_ring || !rec.states_state || !rec.target_state ||
                !rec.states_initials || !rec.target_initials || (uintptr_t)rec.state_ring % 4 || (uintptr_t)rec.states_state % 4 ||
                (uintptr_t)rec.target_state % 4))
    return mirl::fail(MIRL_ERR_ARG, std::string("bad ") + name + " arguments (1 <= state_f32 <= 2^20, float32 state blocks on 4-byte "
                                    "boundaries, no null operands)");
  mirl::WindowArgs a;
  a.S = rec.S; a.state_ring = rec.state_ring; a.initials_ring = rec.initials_ring; a.states_state = rec.states_state;
  a.target_state = rec.target_state; a.states_initials = rec.states_initials; a.target_initials = rec.target_initials;
  a.state_vec16 = (rec.S && rec.S % 4 == 0 && mirl::aligned16(rec.state_ring, rec.states_state, rec.target_state)) ? 1 : 0;
  a.action_words = action_words;
  a.T = T; a.B = B; a.E = E; a.cap = cap; a.nstep_target = nstep_target; a.gamma = gamma; a.lam = lam; a.obs_bytes = obs_bytes;
  a.plan = plan; a.obs_ring = (const unsigned char*)obs_ring; a.actions_ring = (const int*)actions_ring; a.rewards_ring = rewards_ring;
  a.dones_ring = dones_ring; a.logp_ring = logp_ring; a.values_ring = values_ring; a.pol_pitch = pol_pitch;
  a.returns = returns; a.nsteps = nsteps; a.masks = target_masks; a.actions = (int*)actions; a.logp = action_log_probs; a.values = values;
  a.states = (unsigned char*)states; a.target_states = (unsigned char*)target_states;
  a.vec16 = (obs_bytes % 16 == 0 && mirl::aligned16(obs_ring, states, target_states)) ? 1 : 0;
  mirl::ProfScope ps("k_online_window", (double)T * B * (4.0 * (double)obs_bytes + 32.0 + 8.0 * action_words + (rec.S ? 16.0 * rec.S + 16.0 : 0.0)),
                     (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_online_window, dim3((unsigned)(T * B)), dim3(256), 0, (hipStream_t)stream, a);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_online_window(int32_t T, int32_t B, int32_t E, int32_t cap, int32_t nstep_target, double gamma, double lam,
                                  int64_t obs_bytes, const int32_t* plan, const void* obs_ring, const int32_t* actions_ring,
                                  const float* rewards_ring, const uint8_t* dones_ring, const float* logp_ring, const float* values_ring,
                                  int32_t pol_pitch, float* returns, float* nsteps, float* target_masks, int32_t* actions,
                                  float* action_log_probs, float* values, void* states, void* target_states, void* stream) {
  return online_window("online_window", T, B, E, cap, nstep_target, gamma, lam, obs_bytes, 1, plan, obs_ring, actions_ring, rewards_ring,
                       dones_ring, logp_ring, values_ring, pol_pitch, returns, nsteps, target_masks, actions, action_log_probs, values,
                       states, target_states, WindowState(), stream);
}

extern "C" int mirl_online_window_box(int32_t T, int32_t B, int32_t E, int32_t cap, int32_t nstep_target, double gamma, double lam,
                                      int64_t obs_bytes, const int32_t* plan, const void* obs_ring, const void* actions_ring,
                                      const float* rewards_ring, const uint8_t* dones_ring, const float* logp_ring,
                                      const float* values_ring, int32_t pol_pitch, float* returns, float* nsteps, float* target_masks,
                                      void* actions, float* action_log_probs, float* values, void* states, void* target_states,
                                      int32_t action_words, void* stream) {
  return online_window("online_window_box", T, B, E, cap, nstep_target, gamma, lam, obs_bytes, action_words, plan, obs_ring, actions_ring,
                       rewards_ring, dones_ring, logp_ring, values_ring, pol_pitch, returns, nsteps, target_masks, actions,
                       action_log_probs, values, states, target_states, WindowState(), stream);
}

extern "C" int mirl_online_window_rec(int32_t T, int32_t B, int32_t E, int32_t cap, int32_t nstep_target, double gamma, double lam,
                                      int64_t obs_bytes, const int32_t* plan, const void* obs_ring, const void* actions_ring,
                                      const float* rewards_ring, const uint8_t* dones_ring, const float* logp_ring,
                                      const float* values_ring, int32_t pol_pitch, float* returns, float* nsteps, float* target_masks,
                                      void* actions, float* action_log_probs, float* values, void* states, void* target_states,
                                      int32_t action_words, const float* state_ring, const float* initials_ring, int32_t state_f32,
                                      float* states_state, float* target_state, float* states_initials, float* target_initials,
                                      void* stream) {
  if (state_f32 < 1) return mirl::fail(MIRL_ERR_ARG, "bad online_window_rec arguments (state_f32 >= 1)");
  WindowState rec;
  rec.S = state_f32; rec.state_ring = state_ring; rec.initials_ring = initials_ring; rec.states_state = states_state;
  rec.target_state = target_state; rec.states_initials = states_initials; rec.target_initials = target_initials;
  return online_window("online_window_rec", T, B, E, cap, nstep_target, gamma, lam, obs_bytes, action_words, plan, obs_ring, actions_ring,
                       rewards_ring, dones_ring, logp_ring, values_ring, pol_pitch, returns, nsteps, target_masks, actions,
                       action_log_probs, values, states, target_states, rec, stream);
}

extern "C" int mirl_ac_loss_normal(int64_t M, int32_t D, const float* mean, int64_t pitch, const float* logstd, const float* values,
                                   const float* actions, const float* targets, const float* acting_values, const float* old_log_probs,
                                   double vf_coef, double entropy_factor, double clip_value, int32_t adv_norm, float* dmean,
                                   int64_t dpitch, float* dlogstd, float* dvalues, float* log_probs, float* stats, void* stream) {
  if (M < 1 || M > (1 << 22) || D < 1 || D > mirl::kMaxBoxDims || pitch < D || dpitch < D || (adv_norm != 0 && adv_norm != 1) ||
      (adv_norm && M < 2) || !mean || !logstd || !values || !actions || !targets || !acting_values || !dmean || !dlogstd || !dvalues ||
      !stats || (old_log_probs && !(clip_value >= 0.0)))
    return mirl::fail(MIRL_ERR_ARG, "bad ac_loss_normal arguments (1 <= M <= 2^22, M >= 2 with adv_norm, 1 <= D <= 16, pitches >= D, "
                                    "adv_norm 0 | 1, clip_value >= 0 with old_log_probs, no null operands)");
  mirl::NormalLossArgs a;
  a.M = M; a.D = D; a.mean = mean; a.pitch = pitch; a.logstd = logstd; a.values = values; a.actions = actions; a.targets = targets;
  a.acting_values = acting_values; a.old_log_probs = old_log_probs; a.vf_coef = vf_coef; a.entropy_factor = entropy_factor;
  a.clip_value = clip_value; a.adv_norm = adv_norm; a.dmean = dmean; a.dpitch = dpitch; a.dlogstd = dlogstd; a.dvalues = dvalues;
  a.log_probs = log_probs; a.stats = stats;
  mirl::ProfScope ps("k_ac_loss_normal", (double)M * (3.0 * D + 8.0) * 4.0, (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_ac_loss_normal, dim3(1), dim3(mirl::kLossThreads), 0, (hipStream_t)stream, a);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_ac_loss(int64_t M, int32_t A, const float* logits, int64_t pitch, const float* values, const int32_t* actions,
                            const float* targets, const float* acting_values, const float* old_log_probs, double vf_coef,
                            double entropy_factor, double clip_value, int32_t adv_norm, float* dlogits, int64_t dpitch, float* dvalues,
                            float* log_probs, float* stats, void* stream) {
  if (M < 1 || M > (1 << 22) || A < 1 || A > 64 || pitch < A || dpitch < A || (adv_norm != 0 && adv_norm != 1) || (adv_norm && M < 2) ||
      !logits || !values || !actions || !targets || !acting_values || !dlogits || !dvalues || !stats ||
      (old_log_probs && !(clip_value >= 0.0)))
    return mirl::fail(MIRL_ERR_ARG, "bad ac_loss arguments (1 <= M <= 2^22, M >= 2 with adv_norm, 1 <= A <= 64, pitches >= A, "
                                    "adv_norm 0 | 1, clip_value >= 0 with old_log_probs, no null operands)");
  mirl::LossArgs a;
  a.M = M; a.A = A; a.logits = logits; a.pitch = pitch; a.values = values; a.actions = actions; a.targets = targets;
  a.acting_values = acting_values; a.old_log_probs = old_log_probs; a.vf_coef = vf_coef; a.entropy_factor = entropy_factor;
  a.clip_value = clip_value; a.adv_norm = adv_norm; a.dlogits = dlogits; a.dpitch = dpitch; a.dvalues = dvalues;
  a.log_probs = log_probs; a.stats = stats;
  mirl::ProfScope ps("k_ac_loss", (double)M * (2.0 * A + 8.0) * 4.0, (hipStream_t)stream);
  hipLaunchKernelGGL(mirl::k_ac_loss, dim3(1), dim3(mirl::kLossThreads), 0, (hipStream_t)stream, a);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}
