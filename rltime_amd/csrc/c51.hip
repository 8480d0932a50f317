// c51.hip — distributional DQN (C51) arithmetic for gfx950: the categorical target
// projection, the softmax loss with its analytic backward, and the acting head.
//
//   k_target_c51      training/torch/dist_dqn.py:30-97 (selection softmax / expectation /
//                     argmax, target softmax, projection with two index_add_ passes)
//   k_loss_c51        dist_dqn.py:99-142 (softmax of the chosen action's atoms, clamped
//                     cross-entropy or _calc_loss of p - t) forward + backward
//   k_actor_head_c51  policies/torch/dist_dqn.py:_actor_predict_postprocess after the dueling
//                     combine, argmax and epsilon-greedy exactly as k_actor_head (acting.hip)
//
// One wavefront per row throughout; lane l owns atoms l, l + 64, l + 128, l + 192 (Z <= 256).
// fp32 like the reference.  The projection's Tz / b arithmetic is the reference's float32
// operation sequence (build.sh passes -ffp-contract=off; the division by dz is a true
// division, as on the CPU): whether b lands on an integer decides whether an atom's mass
// is dropped, so these few operations must round exactly as the reference's do.
#include "common.hpp"
#include "philox.hpp"

namespace mirl {

constexpr int kC51MaxAtoms = 256;
constexpr int kStrips = kC51MaxAtoms / 64;

__device__ __forceinline__ float wave_max(float v) {
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v = v + __shfl_xor(v, o);
  return v;
}

// softmax over the Z atoms of one row (x[j], lane-strided in registers): p[s] = exp(x - max) * (1 / sum)
// like torch's CPU softmax over the last dimension
__device__ __forceinline__ void wave_softmax(const float x[kStrips], float p[kStrips], int Z, int lane) {
  float mx = -INFINITY;
#pragma unroll
  for (int s = 0; s < kStrips; ++s) if (lane + 64 * s < Z) mx = fmaxf(mx, x[s]);
  mx = wave_max(mx);
  float sum = 0.f;
#pragma unroll
  for (int s = 0; s < kStrips; ++s) { p[s] = (lane + 64 * s < Z) ? expf(x[s] - mx) : 0.f; sum += p[s]; }
  const float inv = 1.0f / wave_sum(sum);
#pragma unroll
  for (int s = 0; s < kStrips; ++s) p[s] = p[s] * inv;
}

// sum_j softmax(row)_j * support_j, the expected value of one action's distribution
__device__ __forceinline__ float wave_expectation(const float* __restrict__ row, const float sup[kStrips], int Z, int lane) {
  float x[kStrips], p[kStrips];
#pragma unroll
  for (int s = 0; s < kStrips; ++s) x[s] = (lane + 64 * s < Z) ? row[lane + 64 * s] : 0.f;
  wave_softmax(x, p, Z, lane);
  float e = 0.f;
#pragma unroll
  for (int s = 0; s < kStrips; ++s) e += p[s] * sup[s];
  return wave_sum(e);
}

// proj: 0 = the reference's projection (Tz = (r + mask * gamma^n) * z_j; an atom with b on an integer is dropped),
//       1 = the paper's (Tz = r + mask * gamma^n * z_j; an atom with b on an integer keeps its whole mass)
__global__ void __launch_bounds__(256)
k_target_c51(int64_t M, int A, int Z, const float* __restrict__ lt, const float* __restrict__ ls,
             const float* __restrict__ support, const float* __restrict__ returns, const float* __restrict__ nsteps,
             const float* __restrict__ masks, float gamma, float vmin, float vmax, float dz, int proj,
             float* __restrict__ out) {
  __shared__ float s_lo[4][kC51MaxAtoms], s_up[4][kC51MaxAtoms];
  __shared__ int s_l[4][kC51MaxAtoms], s_u[4][kC51MaxAtoms];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * 4 + wave;
  if (m >= M) return;                            // whole wave exits together; only wave barriers below
  float sup[kStrips];
#pragma unroll
  for (int s = 0; s < kStrips; ++s) sup[s] = (lane + 64 * s < Z) ? support[lane + 64 * s] : 0.f;
  // dist_dqn.py:64-69: argmax_a sum_j softmax(sel)_aj * z_j, first maximum
  const float* srow = ls + m * (int64_t)A * Z;
  int best = 0;
  float bv = wave_expectation(srow, sup, Z, lane);
  for (int a = 1; a < A; ++a) {
    const float v = wave_expectation(srow + (int64_t)a * Z, sup, Z, lane);
    if (v > bv) { bv = v; best = a; }
  }
  // :73-76: the target net's distribution of that action
  const float* trow = lt + (m * A + best) * (int64_t)Z;
  float x[kStrips], p[kStrips];
#pragma unroll
  for (int s = 0; s < kStrips; ++s) x[s] = (lane + 64 * s < Z) ? trow[lane + 64 * s] : 0.f;
  wave_softmax(x, p, Z, lane);
  // :82-87: Tz, clamp, b, l, u — the reference's float32 operations in its order
  const float r = returns[m], disc = masks[m] * powf(gamma, nsteps[m]);
  const float coef = r + disc;
#pragma unroll
  for (int s = 0; s < kStrips; ++s) {
    const int j = lane + 64 * s;
    if (j < Z) {
      float tz = proj ? r + disc * sup[s] : coef * sup[s];
      tz = fminf(fmaxf(tz, vmin), vmax);
      const float b = (tz - vmin) / dz;
      const float lf = floorf(b), uf = ceilf(b);
      float lo = p[s] * (uf - b), up = p[s] * (b - lf);
      if (proj && lf == uf) lo = p[s];           // the paper: all of the mass to the bin b sits on
      s_lo[wave][j] = lo; s_up[wave][j] = up;
      s_l[wave][j] = (int)lf; s_u[wave][j] = (int)uf;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  // :89-94: two index_add_ passes; bin k sums its lower shares over ascending j, then its upper shares — the
  // reference's accumulation order, with no atomics (lane k owns bin k)
#pragma unroll
  for (int s = 0; s < kStrips; ++s) {
    const int k = lane + 64 * s;
    if (k < Z) {
      float acc = 0.f;
      for (int j = 0; j < Z; ++j) if (s_l[wave][j] == k) acc += s_lo[wave][j];
      for (int j = 0; j < Z; ++j) if (s_u[wave][j] == k) acc += s_up[wave][j];
      out[m * Z + k] = acc;
    }
  }
}

// dist_dqn.py:99-142.  mode: 0 = cross-entropy -sum_j t_j log(clamp(p_j, 1e-5, 1 - 1e-5)), 1 = mse, 2 = huber of
// p - t summed over atoms.  Outputs: row_loss[m] = w * loss, report[m] = loss (losses_to_report), dx = d(row_scale *
// sum_m row_loss) / d logits, zero outside the chosen action's Z columns.
__global__ void __launch_bounds__(256)
k_loss_c51(int64_t M, int A, int Z, const float* __restrict__ logits, const int64_t* __restrict__ actions,
           const float* __restrict__ targets, const float* __restrict__ weights, int mode, float kappa, float row_scale,
           float* __restrict__ row_loss, float* __restrict__ dx, float* __restrict__ report) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t m = (int64_t)blockIdx.x * 4 + wave;
  if (m >= M) return;
  const int a = (int)actions[m];
  const float* row = logits + (m * A + a) * (int64_t)Z;
  float x[kStrips], p[kStrips], t[kStrips], g[kStrips];
#pragma unroll
  for (int s = 0; s < kStrips; ++s) {
    const bool in = lane + 64 * s < Z;
    x[s] = in ? row[lane + 64 * s] : 0.f;
    t[s] = in ? targets[m * Z + lane + 64 * s] : 0.f;
  }
  wave_softmax(x, p, Z, lane);
  const float lo = 1e-5f, hi = (float)(1.0 - 1e-5);     // clamp(1e-5, 1 - 1e-5) of float32 probabilities
  float loss = 0.f, tin = 0.f, pg = 0.f;
#pragma unroll
  for (int s = 0; s < kStrips; ++s) {
    if (lane + 64 * s >= Z) { g[s] = 0.f; continue; }
    if (mode == 0) {
      const float pc = fminf(fmaxf(p[s], lo), hi);
      loss -= t[s] * logf(pc);
      g[s] = (p[s] >= lo && p[s] <= hi) ? t[s] : 0.f;     // torch's clamp passes the gradient on [lo, hi]
      tin += g[s];
    } else {
      const float e = p[s] - t[s];
      float val, gr;
      if (mode == 1) { val = e * e; gr = 2.f * e; }
      else {
        const float ae = fabsf(e);
        if (ae <= kappa) { val = 0.5f * e * e; gr = e; } else { val = kappa * (ae - 0.5f * kappa); gr = e > 0.f ? kappa : -kappa; }
      }
      loss += val;
      g[s] = gr;
      pg += p[s] * gr;
    }
  }
  loss = wave_sum(loss);
  // softmax backward: dx_k = p_k (g_k - sum_j p_j g_j); for the cross-entropy g_j = -t_j / p_j on the clamp's
  // pass-through set, which folds to dx_k = -t_k [k in] + p_k sum_j t_j [j in]
  const float sum_g = mode == 0 ? wave_sum(tin) : wave_sum(pg);
  const float w = weights ? weights[m] : 1.f;
  if (lane == 0) { report[m] = loss; row_loss[m] = loss * w; }
  const float sc = w * row_scale;
  float* grow = dx + m * (int64_t)A * Z;
  for (int aa = 0; aa < A; ++aa) {
#pragma unroll
    for (int s = 0; s < kStrips; ++s) {
      const int j = lane + 64 * s;
      if (j < Z) {
        float v = 0.f;
        if (aa == a) v = (mode == 0 ? (p[s] * sum_g - g[s]) : p[s] * (g[s] - sum_g)) * sc;
        grow[(int64_t)aa * Z + j] = v;
      }
    }
  }
}

// The distributional acting head, one wave per env: q_a = sum_j softmax_j(V_j + A_aj - mean_a A_aj) z_j (without a value
// stream: softmax of A_aj), first-maximum argmax, then epsilon-greedy with k_actor_head's draws (acting.hip): the
// Philox block of (seed, *rng_step, env) when rng_step is given, else the caller's uniforms u / random actions rnd.
__global__ void __launch_bounds__(256)
k_actor_head_c51(int E, int A, int Z, const float* __restrict__ adv, int adv_pitch, const float* __restrict__ val,
                 int val_pitch, const float* __restrict__ support, const double* __restrict__ eps,
                 const double* __restrict__ expo, double eps_min, const float* __restrict__ u, const int64_t* __restrict__ rnd,
                 uint64_t rng_seed, const uint64_t* __restrict__ rng_step, int32_t* __restrict__ actions,
                 float* __restrict__ qvalues, float* __restrict__ eps_used) {
  const int lane = threadIdx.x & 63;
  const int e = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (e >= E) return;
  const float* row = adv + (int64_t)e * adv_pitch;
  float sup[kStrips], mean[kStrips], v[kStrips];
#pragma unroll
  for (int s = 0; s < kStrips; ++s) {
    const int j = lane + 64 * s;
    sup[s] = j < Z ? support[j] : 0.f;
    mean[s] = 0.f; v[s] = 0.f;
    if (val && j < Z) {                          // dqn.py:74-87 per atom: mean over actions
      float acc = 0.f;
      for (int a = 0; a < A; ++a) acc = acc + row[(int64_t)a * Z + j];
      mean[s] = acc / (float)A;
      v[s] = val[(int64_t)e * val_pitch + j];
    }
  }
  float best = 0.f; int arg = 0;
  for (int a = 0; a < A; ++a) {
    float x[kStrips], p[kStrips];
#pragma unroll
    for (int s = 0; s < kStrips; ++s) {
      const int j = lane + 64 * s;
      x[s] = 0.f;
      if (j < Z) x[s] = val ? (v[s] + row[(int64_t)a * Z + j]) - mean[s] : row[(int64_t)a * Z + j];
    }
    wave_softmax(x, p, Z, lane);
    float q = 0.f;
#pragma unroll
    for (int s = 0; s < kStrips; ++s) q += p[s] * sup[s];
    q = wave_sum(q);
    if (lane == 0) qvalues[(int64_t)e * A + a] = q;
    if (a == 0 || q > best) { best = q; arg = a; }    // first maximum, like argmax
  }
  if (lane == 0) {
    int act = arg;
    if (eps) {                                          // epsilon_greedy.py:74-100, as k_actor_head
      double pe = pow(*eps, expo ? expo[e] : 1.0);
      float per = (float)(pe > eps_min ? pe : eps_min);
      if (rng_step) {
        uint32_t r[4];
        philox_4x32(rng_seed, *rng_step, (uint32_t)e, r);
        const float uf = (float)(r[0] >> 8) * (1.0f / 16777216.0f);
        if (uf < per) act = (int)(((uint64_t)r[1] * (uint64_t)A) >> 32);
      } else if (u[e] < per) act = (int)rnd[e];
      if (eps_used) eps_used[e] = per;
    }
    actions[e] = act;
  }
}

}  // namespace mirl

using namespace mirl;

extern "C" int mirl_q_target_c51(int64_t M, int32_t A, int32_t Z, const float* logits_target, const float* logits_select,
                                 const float* support, const float* returns, const float* nsteps, const float* masks,
                                 double gamma, double vmin, double vmax, double delta_z, int32_t projection, float* targets,
                                 void* stream) {
  if (M <= 0 || A <= 0 || Z < 2 || !logits_target || !logits_select || !support || !returns || !nsteps || !masks || !targets ||
      (projection != 0 && projection != 1) || !(delta_z > 0.0))
    return fail(MIRL_ERR_ARG, "bad q_target_c51 arguments");
  if (Z > kC51MaxAtoms) return fail(MIRL_ERR_ARG, "q_target_c51: at most 256 atoms");
  ProfScope ps("k_target_c51", (double)M * ((logits_select == logits_target ? 1.0 : 2.0) * A * Z * 4 + Z * 4 + 12),
               (hipStream_t)stream);
  hipLaunchKernelGGL(k_target_c51, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, M, (int)A, (int)Z,
                     logits_target, logits_select, support, returns, nsteps, masks, (float)gamma, (float)vmin, (float)vmax,
                     (float)delta_z, (int)projection, targets);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_loss_c51(int64_t M, int32_t A, int32_t Z, const float* logits, const int64_t* actions, const float* targets,
                             const float* weights, int32_t mode, double kappa, double row_scale, float* row_loss, float* dlogits,
                             float* report, void* stream) {
  if (M <= 0 || A <= 0 || Z <= 0 || !logits || !actions || !targets || !row_loss || !dlogits || !report || mode < 0 || mode > 2)
    return fail(MIRL_ERR_ARG, "bad loss_c51 arguments");
  if (Z > kC51MaxAtoms) return fail(MIRL_ERR_ARG, "loss_c51: at most 256 atoms");
  ProfScope ps("k_loss_c51", (double)M * ((double)Z * 4 * 2 + (double)A * Z * 4 + 8 + (weights ? 4 : 0) + 8), (hipStream_t)stream);
  hipLaunchKernelGGL(k_loss_c51, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, M, (int)A, (int)Z, logits,
                     actions, targets, weights, (int)mode, (float)kappa, (float)row_scale, row_loss, dlogits, report);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_actor_head_c51(int32_t E, int32_t A, int32_t Z, const float* adv, int32_t adv_pitch, const float* val,
                                   int32_t val_pitch, const float* support, const double* eps, const double* expo, double eps_min,
                                   const float* u, const int64_t* rnd, uint64_t rng_seed, const uint64_t* rng_step,
                                   int32_t* actions, float* qvalues, float* eps_used, void* stream) {
  if (E <= 0 || A <= 0 || Z <= 0 || adv_pitch < A * Z || !adv || !support || !actions || !qvalues ||
      (val && val_pitch < Z) || (eps && !rng_step && (!u || !rnd)))
    return fail(MIRL_ERR_ARG, "bad actor_head_c51 arguments");
  if (Z > kC51MaxAtoms) return fail(MIRL_ERR_ARG, "actor_head_c51: at most 256 atoms");
  ProfScope ps("k_actor_head_c51", 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(k_actor_head_c51, dim3((E + 3) / 4), dim3(256), 0, (hipStream_t)stream, (int)E, (int)A, (int)Z, adv,
                     (int)adv_pitch, val, (int)val_pitch, support, eps, expo, eps_min, u, rnd, rng_seed, rng_step, actions, qvalues,
                     eps_used);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}
