// act_mlp.hip — the whole acting network of an MLP Q-learning policy (cartpole_dqn / cartpole_iqn: 4 -> 64 -> 64 -> 2,
// 32 quantile rows per env for IQN) for one vector step in ONE launch.
//
// Reference order (rltime/policies/torch/dqn.py:50-87,132-148, iqn.py:67-131, exploration/epsilon_greedy.py:74-100):
//   f        = the observation through L Linear + ReLU layers (L in {0, 1, 2}; L = 0: f is the observation)
//   tau[n]   = given, or the 24-bit uniform of Philox4x32-10(seed ^ 0x7A5, *step, e N + n)   (as k_cos_embed_rng / k_act_embed)
//   x[n]     = relu(cos(freq tau[n]) . wq^T + bq) * f                                         (N >= 1 and D > 0; else x[0] = f)
//   hid[n]   = relu(x[n] . wfc^T + bfc)        [last FC | dueling value-hidden], HID wide
//   out[n]   = hid[n] . wout^T + bout          A advantages [+ 1 value]
//   q[a]     = mean_n (V + A_a - mean_a A)     (mean_n A_a without a value stream, or with need_q = 0)
//   action   = first maximum, then the epsilon-greedy remap on the Philox block (seed, *step, e) of k_actor_head
//
// One workgroup of 256 threads per env.  Every product is the same loop (`dense`): a thread owns ONE output unit j and
// RB = 16 rows of the chunk (RB = 1 where there is one row: the leading layers, a policy without a quantile layer; with
// J < 256 units the 256 threads split into 256 / roundup(J, 64) row groups), walks k = 0 .. K-1 in ascending order with one float32 multiply and one add per term
// (the library builds with -ffp-contract=off: no fused multiply-add) and reads the rows' inputs from LDS at an address
// the whole wave shares (a broadcast: no bank conflict).  The weights come from a TRANSPOSED copy wT[k][j] in global
// memory, staged through LDS in tiles of up to 4096 floats (whole k rows of the pass's columns): all 256 threads fetch a
// tile with 16 independent, coalesced loads each — consecutive lanes, consecutive units — and the fetch of tile t + 1 is
// in flight while tile t is multiplied, so a product waits for ONE memory round trip, not for one per k.  (A first form
// read wT[k][j] straight from global memory inside the k loop: the loads of one thread were served one after the other
// and the shipped IQN vector step measured 86.9 us as rollouts against 48.8 us now.)  From the tile a wave's lanes read consecutive floats: no bank
// conflict.  No atomics, no cross-thread sums before the final mean over the quantile rows, which is k_actor_head's wave
// reduction: a rerun repeats to the bit.
//
// LDS (dynamic, floats): 2 x 256 ping-pong rows of the leading layers, 64 fractions, the 4096-float weight tile, then per
// chunk of CH quantile rows phi [CH][D], x [CH][W], hid [CH][HID], and out [N][NO] for all rows.  The launcher takes
// CH = 32 when that fits the 64 KB a kernel gets unasked and 16 otherwise: the shipped IQN shape (W = 64, HID = 128,
// N = 32, D = 64) is 51 KB with all 32 rows in one chunk, the shipped DQN shape 18.6 KB; at every limit at once (W = 256,
// HID = 512, N = D = 64, NO = 33) CH = 16 is 2 + 0.25 + 16 + 4 + 16 + 32 + 8.25 = 78.5 KB of the CU's 160 KB, the one
// case that has the limit raised.  Nothing but actions, qvalues and taus_out is written to HBM.
//
// Occupancy: the grid is E workgroups — 16 on a chip of 256 CUs for the shipped configs — so a CU never holds two of
// them and neither the LDS block nor the register count (16 accumulators + 16 prefetched weights) limits
// anything.  The kernel is a latency chain of four or five products; what a workgroup waits for is the first tile of
// each (served by L2 after the first workgroup touched it: the shipped IQN weights are 50 KB) and the LDS reads of the
// k loop (one weight + RB broadcast inputs per RB multiply-adds), not HBM bandwidth.
//
// The actor-critic form (mirl_act_mlp_ac_fwd, k_act_mlp<true>; cartpole_ppo / cartpole_a2c: 4 -> 64 -> 64 -> [2 logits | value],
// rltime/policies/torch/actor_critic.py:37-71) is the same trunk with N = 1, D = 0 — every product dense_rb<1>, as a policy
// without a quantile layer runs it — one dense output product [logits | value] (NO = A + 1), and as its tail the sampling head
// of k_actor_head_ac_rng (ac_head.hpp: one statement for both) on the LDS row, by thread 0.  One row: the LDS block is
// 4.6 K floats + W + HID + A + 1, under 22 KB at every limit; the occupancy and latency reasoning above carries over unchanged
// (E workgroups on 256 CUs, a chain of three or four products).
#include "common.hpp"
#include "philox.hpp"
#include "ac_head.hpp"

namespace mirl {

struct ActMlpArgs {
  const float* obs;
  const float* lwT[2]; const float* lb[2];
  const float* freq; const float* taus; const float* wqT; const float* bq;
  const float* fcT; const float* fcb; const float* outT; const float* outb;
  const double* eps; const double* expo; double eps_min;
  uint64_t seed; const uint64_t* step;
  int32_t* actions; float* qvalues; float* taus_out;
  // the actor-critic tail (k_act_mlp<true>): qvalues is the [log-probability | value] block, out_pitch floats per env
  float* logits_out; int greedy, out_pitch;
  int E, O, L, w0, w1, W, N, D, HID, NO, A, hid_run, no_run, CH, has_val;
};

constexpr int ACT_MLP_TILE = 4096;       // floats of the weight tile in LDS

// this thread's 16 floats of the tile that holds rows k0 .. k0 + tk - 1, columns j0 .. j0 + Jt - 1 of wT
__device__ __forceinline__ void fetch_tile(float (&pf)[16], const float* __restrict__ wT, int w_pitch, int k0, int tk, int j0, int Jt) {
  const int n = tk * Jt;
  const float* src = wT + (int64_t)k0 * w_pitch + j0;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int idx = (int)threadIdx.x + 256 * i;
    if (idx < n) { const int kk = idx / Jt; pf[i] = src[(int64_t)kk * w_pitch + (idx - kk * Jt)]; }
  }
}

// out(r, j) = sum_k in[r][k] * wT[k][j], k ascending, for r < R and j < J; `epi(r, j, sum)` stores it.  Called by all
// 256 threads (barriers inside); the caller's barrier after it makes the stored rows visible.  RB rows per thread.
template <int RB, class Epi>
__device__ __forceinline__ void dense_rb(const float* in, int in_pitch, int R, int K, const float* __restrict__ wT, int w_pitch, int J,
                                         float* tile, Epi epi) {
  const int tid = threadIdx.x;
  const int JP = J >= 256 ? 256 : (J + 63) & ~63;
  const int G = 256 / JP;
  const int g = tid / JP, jl = tid - g * JP;
  for (int j0 = 0; j0 < J; j0 += JP) {
    const int Jt = J - j0 < JP ? J - j0 : JP;          // this pass's columns
    const int TK = ACT_MLP_TILE / Jt;                  // whole k rows per tile
    const bool live = jl < Jt;
    const int jc = live ? jl : Jt - 1;                 // (a lane past the columns reads the last one: dropped)
    for (int rp = 0; rp < R; rp += G * RB) {           // one pass for the shipped shapes
      const int r0 = rp + g * RB;
      const bool rows_here = g < G && r0 < R;          // wave-uniform: JP is a multiple of the wave
      int ri[RB];                                      // a row past R reads row R - 1: in bounds, dropped
#pragma unroll
      for (int i = 0; i < RB; ++i) ri[i] = (r0 + i < R ? r0 + i : R - 1) * in_pitch;
      float acc[RB];
#pragma unroll
      for (int i = 0; i < RB; ++i) acc[i] = 0.f;
      float pf[16];
      fetch_tile(pf, wT, w_pitch, 0, K < TK ? K : TK, j0, Jt);
      for (int k0 = 0; k0 < K; k0 += TK) {
        const int tk = K - k0 < TK ? K - k0 : TK;
        __syncthreads();                               // the previous tile (and whatever used these rows before) was read
#pragma unroll
        for (int i = 0; i < 16; ++i) if (tid + 256 * i < tk * Jt) tile[tid + 256 * i] = pf[i];
        __syncthreads();
        const int kn = k0 + TK;                        // the next tile is in flight while this one is multiplied
        if (kn < K) fetch_tile(pf, wT, w_pitch, kn, K - kn < TK ? K - kn : TK, j0, Jt);
        if (rows_here) {
          const float* x = in + k0;
          const float* w = tile + jc;
#pragma unroll 4
          for (int kk = 0; kk < tk; ++kk) {
            const float wv = w[kk * Jt];
#pragma unroll
            for (int i = 0; i < RB; ++i) acc[i] = acc[i] + x[ri[i] + kk] * wv;
          }
        }
      }
      if (rows_here && live) {
#pragma unroll
        for (int i = 0; i < RB; ++i)
          if (r0 + i < R) epi(r0 + i, j0 + jl, acc[i]);
      }
    }
  }
}

// AC = false: the Q-learning tail below (dueling combine, mean over the quantile rows, first maximum, epsilon-greedy).
// AC = true: the actor-critic tail — the one row [logits | value] goes through ac_head_row (ac_head.hpp), the statement
// k_actor_head_ac and k_actor_head_ac_rng share.  Everything before the tail is the same code for both.
template <bool AC>
__global__ void __launch_bounds__(256)
k_act_mlp(ActMlpArgs a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* fa = lds;                       // [256]
  float* fb = fa + 256;                  // [256]
  float* tau = fb + 256;                 // [64]
  float* tile = tau + 64;                // [ACT_MLP_TILE]
  float* phi = tile + ACT_MLP_TILE;      // [CH][D]
  float* xq = phi + a.CH * a.D;          // [CH][W]
  float* hid = xq + a.CH * a.W;          // [CH][HID]
  float* outs = hid + a.CH * a.HID;      // [N][NO]
  const int tid = threadIdx.x, e = blockIdx.x;
  const bool quant = a.D > 0;

  // the observation and the quantile fractions
  if (tid < a.O) fa[tid] = a.obs[(int64_t)e * a.O + tid];
  if (quant && tid < a.N) {
    const int m = e * a.N + tid;
    float t;
    if (a.taus) t = a.taus[m];
    else { uint32_t rn[4]; philox_4x32(a.seed ^ 0x7A5ull, *a.step, (uint32_t)m, rn); t = (float)(rn[0] >> 8) * (1.0f / 16777216.0f); }
    tau[tid] = t;
    if (a.taus_out) a.taus_out[m] = t;
  }
  __syncthreads();

  // leading layers: f = relu(f . w^T + b)
  float* f = fa;
  int K = a.O;
  for (int l = 0; l < a.L; ++l) {
    float* dst = f == fa ? fb : fa;
    const float* b = a.lb[l];
    const int J = l == 0 ? a.w0 : a.w1;
    dense_rb<1>(f, K, 1, K, a.lwT[l], J, J, tile, [&](int, int j, float s) { s = s + b[j]; dst[j] = s > 0.f ? s : 0.f; });
    __syncthreads();
    f = dst; K = J;
  }
  const int W = a.W;                     // == K

  for (int n0 = 0; n0 < a.N; n0 += a.CH) {
    const int R = a.N - n0 < a.CH ? a.N - n0 : a.CH;
    const float* x = f;                  // without a quantile product the one row is the feature row itself
    if (quant) {
      for (int idx = tid; idx < R * a.D; idx += 256) {
        const int r = idx / a.D, i = idx - r * a.D;
        phi[idx] = cosf(a.freq[i] * tau[n0 + r]);
      }
      __syncthreads();
      const float* bq = a.bq;
      dense_rb<16>(phi, a.D, R, a.D, a.wqT, W, W, tile, [&](int r, int j, float s) { s = s + bq[j]; xq[r * W + j] = (s > 0.f ? s : 0.f) * f[j]; });
      __syncthreads();
      x = xq;
    }
    {
      const float* b = a.fcb;
      const int HID = a.HID;
      const float* bo = a.outb;
      const int NO = a.NO;
      auto epi_h = [&](int r, int j, float s) { s = s + b[j]; hid[r * HID + j] = s > 0.f ? s : 0.f; };
      auto epi_o = [&](int r, int j, float s) { outs[(n0 + r) * NO + j] = s + bo[j]; };
      if (quant) {                          // 16 rows per thread; one row without a quantile layer
        dense_rb<16>(x, W, R, W, a.fcT, HID, a.hid_run, tile, epi_h);
        __syncthreads();
        dense_rb<16>(hid, HID, R, a.hid_run, a.outT, NO, a.no_run, tile, epi_o);
      } else {
        dense_rb<1>(x, W, R, W, a.fcT, HID, a.hid_run, tile, epi_h);
        __syncthreads();
        dense_rb<1>(hid, HID, R, a.hid_run, a.outT, NO, a.no_run, tile, epi_o);
      }
      __syncthreads();
    }
  }

  if constexpr (AC) {
    // k_actor_head_ac_rng (actor_critic.hip) on the LDS row [A logits | value]: the raw row for whoever asked, then thread 0
    // draws the block (seed, *step, e), samples (or takes the first maximum) and writes the action and the policy pair
    const int A = a.A, NO = a.NO;
    if (a.logits_out && tid < NO) a.logits_out[(int64_t)e * NO + tid] = outs[tid];
    if (tid != 0) return;
    uint32_t r[4] = {0u, 0u, 0u, 0u};
    if (!a.greedy || a.eps) philox_4x32(a.seed, *a.step, (uint32_t)e, r);
    const float u = a.greedy ? 0.f : (float)(r[0] >> 8) * (1.0f / 16777216.0f);
    float lp;
    int act = ac_head_row(outs, A, u, a.greedy, &lp);
    if (a.eps) {
      // the evaluation's epsilon remap on words 2 and 3 of the same block; the log-probability stays the sampled action's
      const double pe = pow(*a.eps, a.expo ? a.expo[e] : 1.0);
      const float per = (float)(pe > a.eps_min ? pe : a.eps_min);
      const float uf = (float)(r[2] >> 8) * (1.0f / 16777216.0f);
      if (uf < per) act = (int)(((uint64_t)r[3] * (uint64_t)A) >> 32);
    }
    a.actions[e] = act;
    a.qvalues[(int64_t)e * a.out_pitch] = lp;
    a.qvalues[(int64_t)e * a.out_pitch + 1] = outs[A];
    return;
  }
  // k_actor_head (acting.hip) on the LDS rows, by the first wave: V + A - mean_a A, mean over the rows, first maximum,
  // epsilon-greedy on one Philox block per (step, env)
  if (tid >= 64) return;
  const int lane = tid, A = a.A, N = a.N, NO = a.NO;
  float best = 0.f; int arg = 0;
  for (int a0 = 0; a0 < A; a0 += 8) {
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
    for (int n = lane; n < N; n += 64) {
      const float* row = outs + n * NO;
      float off = 0.f;
      if (a.has_val) {
        float m = 0.f;
        for (int q = 0; q < A; ++q) m = m + row[q];
        off = row[A] - m / (float)A;
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) if (a0 + k < A) acc[k] = acc[k] + (row[a0 + k] + off);
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float s = acc[k];
      for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o);
      if (a0 + k < A) {
        const float q = s / (float)N;
        if (lane == 0) a.qvalues[(int64_t)e * A + a0 + k] = q;
        if ((a0 + k == 0) || q > best) { best = q; arg = a0 + k; }
      }
    }
  }
  if (lane == 0) {
    int act = arg;
    if (a.eps) {
      const double pe = pow(*a.eps, a.expo ? a.expo[e] : 1.0);
      const float per = (float)(pe > a.eps_min ? pe : a.eps_min);
      uint32_t r[4];
      philox_4x32(a.seed, *a.step, (uint32_t)e, r);
      const float uf = (float)(r[0] >> 8) * (1.0f / 16777216.0f);
      if (uf < per) act = (int)(((uint64_t)r[1] * (uint64_t)A) >> 32);
    }
    a.actions[e] = act;
  }
}

static int64_t act_mlp_lds_floats(int W, int N, int D, int HID, int NO, int CH) {
  return 256 + 256 + 64 + ACT_MLP_TILE + (int64_t)CH * (D + W + HID) + (int64_t)N * NO;
}

static int act_mlp_chunk(int W, int N, int D, int HID, int NO) {
  return 4 * act_mlp_lds_floats(W, N, D, HID, NO, 32) <= 65536 ? 32 : 16;
}

}  // namespace mirl

using namespace mirl;

extern "C" int mirl_act_mlp_supported(int32_t E, int32_t O, int32_t L, const int32_t* widths, int32_t N, int32_t D, int32_t HID,
                                      int32_t NO, int32_t A) {
  if (E <= 0 || O <= 0 || O > 64 || L < 0 || L > 2 || (L && !widths)) return 0;
  for (int l = 0; l < L; ++l) if (widths[l] <= 0 || widths[l] > 256) return 0;
  if (N <= 0 || N > 64 || D < 0 || D > 64 || (D % 4) || (D == 0 && N != 1)) return 0;
  if (HID <= 0 || HID > 512 || A <= 0 || A > 32 || (NO != A && NO != A + 1)) return 0;
  return (int64_t)E * N <= (1 << 24);
}

extern "C" int mirl_act_mlp_lds_bytes(int32_t O, int32_t L, const int32_t* widths, int32_t N, int32_t D, int32_t HID, int32_t NO,
                                      int32_t A, int64_t* bytes) {
  if (!bytes || !mirl_act_mlp_supported(1, O, L, widths, N, D, HID, NO, A)) return fail(MIRL_ERR_ARG, "bad act_mlp_lds_bytes arguments");
  const int W = L ? widths[L - 1] : O;
  *bytes = 4 * act_mlp_lds_floats(W, N, D, HID, NO, act_mlp_chunk(W, N, D, HID, NO));
  return MIRL_OK;
}

extern "C" int mirl_act_mlp_fwd(int32_t E, int32_t O, int32_t L, const int32_t* widths, int32_t N, int32_t D, int32_t HID, int32_t NO,
                                int32_t A, int32_t H1, int32_t need_q, const float* obs, const float* lw0T, const float* lb0,
                                const float* lw1T, const float* lb1, const float* freq, const float* taus, const float* wqT,
                                const float* bq, const float* fcT, const float* fcb, const float* outT, const float* outb,
                                const double* eps, const double* expo, double eps_min, uint64_t seed, const uint64_t* rng_step,
                                int32_t* actions, float* qvalues, float* taus_out, void* stream) {
  if (!mirl_act_mlp_supported(E, O, L, widths, N, D, HID, NO, A))
    return fail(MIRL_ERR_ARG, "act_mlp_fwd: unsupported shape (O <= 64, L <= 2 layers of <= 256, N <= 64, D <= 64 and D % 4 == 0, "
                              "HID <= 512, A <= 32, NO in {A, A + 1})");
  const bool dueling = NO == A + 1;
  if (H1 <= 0 || H1 > HID || (!dueling && H1 != HID)) return fail(MIRL_ERR_ARG, "act_mlp_fwd: H1 (the advantage stream's hidden width) in 1 .. HID, = HID without a value stream");
  if (!obs || !fcT || !fcb || !outT || !outb || !actions || !qvalues || (L >= 1 && (!lw0T || !lb0)) || (L >= 2 && (!lw1T || !lb1)) ||
      (D > 0 && (!freq || !wqT || !bq || (!taus && !rng_step))) || (eps && !rng_step))
    return fail(MIRL_ERR_ARG, "act_mlp_fwd: null operand (taus or a step word with a quantile layer; a step word with eps)");
  ActMlpArgs a;
  a.obs = obs; a.lwT[0] = lw0T; a.lb[0] = lb0; a.lwT[1] = lw1T; a.lb[1] = lb1;
  a.freq = freq; a.taus = taus; a.wqT = wqT; a.bq = bq; a.fcT = fcT; a.fcb = fcb; a.outT = outT; a.outb = outb;
  a.eps = eps; a.expo = expo; a.eps_min = eps_min; a.seed = seed; a.step = rng_step;
  a.actions = actions; a.qvalues = qvalues; a.taus_out = D > 0 ? taus_out : nullptr;
  a.logits_out = nullptr; a.greedy = 0; a.out_pitch = 0;
  a.E = E; a.O = O; a.L = L; a.w0 = L >= 1 ? widths[0] : 0; a.w1 = L >= 2 ? widths[1] : 0;
  a.W = L ? widths[L - 1] : O; a.N = N; a.D = D; a.HID = HID; a.NO = NO; a.A = A;
  // need_q = 0 under a dueling head: the value stream's hidden units and its output column are not evaluated (out_w is
  // block-diagonal, so the advantage columns lose only terms that are exactly zero)
  const bool full = need_q || !dueling;
  a.hid_run = full ? HID : H1;
  a.no_run = full ? NO : A;
  a.has_val = (dueling && full) ? 1 : 0;
  a.CH = act_mlp_chunk(a.W, N, D, HID, NO);
  const size_t lds = 4 * (size_t)act_mlp_lds_floats(a.W, N, D, HID, NO, a.CH);
  hipStream_t st = (hipStream_t)stream;
  const double wfloats = (double)O * a.w0 + (double)a.w0 * a.w1 + (double)D * a.W + (double)a.W * HID + (double)HID * NO;
  if (lds > 65536) { int rc = raise_lds_limit(k_act_mlp<false>, lds); if (rc) return rc; }
  ProfScope ps("k_act_mlp", 4.0 * (wfloats + (double)E * (O + A + 1)), st);
  hipLaunchKernelGGL(k_act_mlp<false>, dim3(E), dim3(256), lds, st, a);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

// ---- the actor-critic form: the same trunk, [logits | value] as the one output product, the sampling head on its row -------
extern "C" int mirl_act_mlp_ac_supported(int32_t E, int32_t O, int32_t L, const int32_t* widths, int32_t HID, int32_t A) {
  return mirl_act_mlp_supported(E, O, L, widths, 1, 0, HID, A + 1, A);
}

extern "C" int mirl_act_mlp_ac_fwd(int32_t E, int32_t O, int32_t L, const int32_t* widths, int32_t HID, int32_t A, const float* obs,
                                   const float* lw0T, const float* lb0, const float* lw1T, const float* lb1, const float* fcT,
                                   const float* fcb, const float* outT, const float* outb, const double* eps, const double* expo,
                                   double eps_min, uint64_t rng_seed, const uint64_t* rng_step, int32_t greedy, int32_t* actions,
                                   float* policy, int32_t out_pitch, float* logits_out, void* stream) {
  if (!mirl_act_mlp_ac_supported(E, O, L, widths, HID, A))
    return fail(MIRL_ERR_ARG, "act_mlp_ac_fwd: unsupported shape (O <= 64, L <= 2 layers of <= 256, HID <= 512, 1 <= A <= 32)");
  if ((greedy != 0 && greedy != 1) || out_pitch < 2) return fail(MIRL_ERR_ARG, "act_mlp_ac_fwd: greedy 0 | 1, out_pitch >= 2");
  if (!obs || !fcT || !fcb || !outT || !outb || !rng_step || !actions || !policy || (L >= 1 && (!lw0T || !lb0)) ||
      (L >= 2 && (!lw1T || !lb1)))
    return fail(MIRL_ERR_ARG, "act_mlp_ac_fwd: null operand (the step word is required, also with greedy)");
  ActMlpArgs a;
  a.obs = obs; a.lwT[0] = lw0T; a.lb[0] = lb0; a.lwT[1] = lw1T; a.lb[1] = lb1;
  a.freq = nullptr; a.taus = nullptr; a.wqT = nullptr; a.bq = nullptr; a.fcT = fcT; a.fcb = fcb; a.outT = outT; a.outb = outb;
  a.eps = eps; a.expo = expo; a.eps_min = eps_min; a.seed = rng_seed; a.step = rng_step;
  a.actions = actions; a.qvalues = policy; a.taus_out = nullptr;
  a.logits_out = logits_out; a.greedy = greedy; a.out_pitch = out_pitch;
  a.E = E; a.O = O; a.L = L; a.w0 = L >= 1 ? widths[0] : 0; a.w1 = L >= 2 ? widths[1] : 0;
  a.W = L ? widths[L - 1] : O; a.N = 1; a.D = 0; a.HID = HID; a.NO = A + 1; a.A = A;
  a.hid_run = HID; a.no_run = A + 1; a.has_val = 0;
  a.CH = 1;                                // one row: 4.6 K floats + W + HID + A + 1, under 22 KB at every limit
  const size_t lds = 4 * (size_t)act_mlp_lds_floats(a.W, 1, 0, HID, A + 1, a.CH);
  hipStream_t st = (hipStream_t)stream;
  const double wfloats = (double)O * a.w0 + (double)a.w0 * a.w1 + (double)a.W * HID + (double)HID * (A + 1);
  ProfScope ps("k_act_mlp_ac", 4.0 * (wfloats + (double)E * (O + 3 + (logits_out ? A + 1 : 0))), st);
  hipLaunchKernelGGL(k_act_mlp<true>, dim3(E), dim3(256), lds, st, a);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}
