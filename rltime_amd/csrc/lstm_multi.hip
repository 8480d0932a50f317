// lstm_multi.hip — the multi-sample LSTM sequence (IQN before the LSTM, merge mode "inner") as step kernels.
//
// With IQNPolicy(injection_layer=1) on CNN -> LSTM -> FC the quantile layer sits in front of the LSTM: B stored states,
// B N input rows, rows ordered (t, b, n).  The reference (rltime/models/torch/modules/lstm.py:83-116, inner mode) repeats
// the merged state N times before every step and takes the mean over the N samples after it:
//
//     hin_b = h_b keep[t,b] ; cin_b = c_b keep[t,b] ; r_b = hin_b W_hh^T
//     for n:  a = gx[t,b,n] + r_b ; c_n = sig(a_f) cin_b + sig(a_i) tanh(a_g) ; h_n = sig(a_o) tanh(c_n) ; out[t,b,n] = h_n
//     h_b = mean_n h_n ; c_b = mean_n c_n
//
// The N samples of a sequence enter a step with the SAME state, so the recurrent product has B rows, not B N; only the
// cell runs over B N rows, and the mean over n never leaves a lane.
//
// One launch per time step and direction, ordered by the stream: no persistent sweep, no spin, no arrival counter,
// hence no residency assumption (csrc/lstm_seq.hip has one) and nothing a captured graph could not replay.
//
//   * unit of work: one wave on 16 hidden units x 16 sequences.  The products are formed TRANSPOSED,
//     D[unit][sequence] = W_slab[unit][k] hin^T[k][sequence], with v_mfma_f32_16x16x4_f32 (exact f32 products): lane l
//     ends up with units j0 + 4 (l / 16) + 0..3 of sequence b0 + l % 16, i.e. four CONSECUTIVE hidden units, so every
//     access of the cell loop (gx, out, gates, hm, cm, d_out, S) is one 16-byte load or store per lane;
//   * the waves of a workgroup (MS_WAVES, one per SIMD) own neighbouring unit slabs of the same 16 sequences and
//     share the state tile: hin (16 x H) forward, S(t+1) (16 x 4H, in chunks of MS_KC columns) backward, staged in
//     LDS once per workgroup with rows past B zero-filled; row pitch + 4 floats keeps the 16-byte operand reads
//     conflict-free.  W_hh comes straight from L2: no two waves of a workgroup read the same element of it;
//   * k is permuted inside each group of 16 (MFMA jj of lane group kg takes k = 16 c + 4 kg + jj) so that a lane's
//     four operands of four MFMAs are one 16-byte read — both operands use the same permutation, the sum is the same;
//   * forward: four accumulators (gates i, f, g, o) over K = H, W rows read along k as 16-byte loads;
//     backward: dh_b[unit] = S(t+1)[b, :] W_hh[:, unit] over K = 4H into four accumulators interleaved over k (four
//     independent chains), joined in a fixed order; W is read down its columns, 64 contiguous bytes per 16 lanes;
//   * the per-lane loop over n rebuilds c_n and tanh(c_n) from the stored activated gates and cm[t] in the backward:
//     no (T, B, N, H) cell history exists.  Sums over n (state means, S, dcin) stay in the lane, ascending n, no atomics.
#include "common.hpp"

namespace mirl {

typedef float ms_f4 __attribute__((ext_vector_type(4)));

#define MS_WAVES 4        // waves per workgroup: one per SIMD (docs/kernels.md)
#define MS_KC 512         // columns of S(t+1) staged per LDS chunk in the backward step
#define MS_PRE 8          // samples whose cell operands are loaded ahead of the MFMA chain (N = 8 is the recommended count)

// v_exp_f32 / v_rcp_f32 forms, as the persistent sweeps use (absolute error of a gate ~1e-7)
__device__ __forceinline__ float ms_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
__device__ __forceinline__ float ms_tanh(float x) { return 1.0f - 2.0f * __builtin_amdgcn_rcpf(__expf(2.0f * x) + 1.0f); }

__device__ __forceinline__ ms_f4 ms_ld4(const float* p) { return *reinterpret_cast<const ms_f4*>(p); }
__device__ __forceinline__ void ms_st4(float* p, ms_f4 v) { *reinterpret_cast<ms_f4*>(p) = v; }

// rows b0 .. b0 + 15, `cols` columns from column c0 of src [B][ld] (times keep[b] when keep) -> tile [16][pitch];
// rows past B are zero.  All threads of the workgroup.
__device__ __forceinline__ void ms_stage(float* tile, int pitch, const float* __restrict__ src, int ld, int c0, int cols,
                                         const float* __restrict__ keep, int b0, int B) {
  const int q = cols >> 2;
  for (int idx = (int)threadIdx.x; idx < 16 * q; idx += (int)blockDim.x) {
    const int row = idx / q, c4 = idx - row * q, b = b0 + row;
    ms_f4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (b < B) {
      v = ms_ld4(src + (size_t)b * ld + c0 + 4 * c4);
      if (keep) v *= keep[b];
    }
    ms_st4(tile + row * pitch + 4 * c4, v);
  }
}

// One forward step.  grid (ceil(B / 16), ceil(H / 16 / MS_WAVES)), MS_WAVES x 64 threads, 16 (H + 4) floats of LDS.
// h_src / c_src [B][H]: the state entering the step — already masked (hm[t] / cm[t]) when keep_in is null, else the
// raw initial state, masked here with keep_in [B] and written to hm_t / cm_t.
__global__ void __launch_bounds__(MS_WAVES * 64)
k_lstm_ms_fwd(int B, int N, int H, float* __restrict__ gx, const float* __restrict__ w, const float* __restrict__ h_src,
              const float* __restrict__ c_src, const float* __restrict__ keep_in, float* __restrict__ hm_t,
              float* __restrict__ cm_t, const float* __restrict__ keep_next, float* __restrict__ out,
              float* __restrict__ hm_next, float* __restrict__ cm_next, float* __restrict__ h_last,
              float* __restrict__ c_last, int save) {
  extern __shared__ float ms_lds[];
  const int pitch = H + 4;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int bl = lane & 15, kg = lane >> 4;
  const int b0 = (int)blockIdx.x * 16, b = b0 + bl;
  const int j0 = ((int)blockIdx.y * MS_WAVES + wave) * 16;
  ms_stage(ms_lds, pitch, h_src, H, 0, H, keep_in, b0, B);
  __syncthreads();
  if (j0 >= H) return;                     // a slab past the layer: this wave only helped to stage
  const bool valid = b < B;
  const int j4 = j0 + 4 * kg;              // this lane: units j4 .. j4 + 3 of sequence b
  float* grow = gx + (valid ? (size_t)b * N * 4 * H + j4 : 0);
  // the pre-activations of the first MS_PRE samples do not depend on the product: their loads fly under the chain
  ms_f4 pre[MS_PRE][4];
#pragma unroll
  for (int n = 0; n < MS_PRE; ++n)
    if (valid && n < N) {
#pragma unroll
      for (int g = 0; g < 4; ++g) pre[n][g] = ms_ld4(grow + (size_t)n * 4 * H + g * H);
    }
  ms_f4 acc[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) acc[g] = ms_f4{0.0f, 0.0f, 0.0f, 0.0f};
  const float* hrow = ms_lds + bl * pitch + 4 * kg;
  const float* wrow = w + (size_t)(j0 + bl) * H + 4 * kg;          // gate g: + g H H
  const size_t gate = (size_t)H * H;
  // 64 k per round: the W operands of the next round (16 x 16-byte loads) are in flight under the 64 MFMAs of this one
  ms_f4 nxt[4][4] = {};
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (16 * i < H) {
#pragma unroll
      for (int g = 0; g < 4; ++g) nxt[i][g] = ms_ld4(wrow + g * gate + 16 * i);
    }
  for (int k = 0; k < H; k += 64) {
    ms_f4 cur[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int g = 0; g < 4; ++g) cur[i][g] = nxt[i][g];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (k + 64 + 16 * i < H) {
#pragma unroll
        for (int g = 0; g < 4; ++g) nxt[i][g] = ms_ld4(wrow + g * gate + k + 64 + 16 * i);
      }
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (k + 16 * i < H) {
        const ms_f4 hv = ms_ld4(hrow + k + 16 * i);
#pragma unroll
        for (int jj = 0; jj < 4; ++jj)
#pragma unroll
          for (int g = 0; g < 4; ++g) acc[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[i][g][jj], hv[jj], acc[g], 0, 0, 0);
      }
  }
  if (!valid) return;
  ms_f4 cin = ms_ld4(c_src + (size_t)b * H + j4);
  if (keep_in) {
    const float k0 = keep_in[b];
    cin *= k0;
    ms_st4(cm_t + (size_t)b * H + j4, cin);
    ms_st4(hm_t + (size_t)b * H + j4, ms_ld4(h_src + (size_t)b * H + j4) * k0);
  }
  ms_f4 sh = {0.0f, 0.0f, 0.0f, 0.0f}, sc = {0.0f, 0.0f, 0.0f, 0.0f};
  float* orow = out + (size_t)b * N * H + j4;
  auto cell = [&](int n, const ms_f4 (&a)[4]) {
    float* gp = grow + (size_t)n * 4 * H;
    ms_f4 gi, gf, gg, go, c, h;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      gi[r] = ms_sigmoid(a[0][r] + acc[0][r]); gf[r] = ms_sigmoid(a[1][r] + acc[1][r]);
      gg[r] = ms_tanh(a[2][r] + acc[2][r]); go[r] = ms_sigmoid(a[3][r] + acc[3][r]);
      c[r] = gf[r] * cin[r] + gi[r] * gg[r];
      h[r] = go[r] * ms_tanh(c[r]);
    }
    ms_st4(orow + (size_t)n * H, h);
    if (save) { ms_st4(gp, gi); ms_st4(gp + H, gf); ms_st4(gp + 2 * H, gg); ms_st4(gp + 3 * H, go); }
    sh += h; sc += c;
  };
#pragma unroll
  for (int n = 0; n < MS_PRE; ++n)
    if (n < N) cell(n, pre[n]);
  for (int n = MS_PRE; n < N; ++n) {
    ms_f4 a[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) a[g] = ms_ld4(grow + (size_t)n * 4 * H + g * H);
    cell(n, a);
  }
  const float inv = 1.0f / (float)N;
  sh *= inv; sc *= inv;
  if (h_last) { ms_st4(h_last + (size_t)b * H + j4, sh); ms_st4(c_last + (size_t)b * H + j4, sc); }
  const float kn = keep_next ? keep_next[b] : 1.0f;
  ms_st4(hm_next + (size_t)b * H + j4, sh * kn);
  ms_st4(cm_next + (size_t)b * H + j4, sc * kn);
}

// One backward step.  Same grid.  gates [B][N][4H]: activated gates in, d loss / d pre-activation out.  s_next
// [B][4H] = S(t+1), null at the last step (then nothing flows back from the future).  dc_ws [B][H]: d loss / d cin of
// step t+1 in, of this step out (the same lane reads and writes an element).  dh_ws [B][H] receives the masked
// d loss / d (merged h) that the prologue formed.
__global__ void __launch_bounds__(MS_WAVES * 64)
k_lstm_ms_bwd(int B, int N, int H, float* __restrict__ gates, const float* __restrict__ w, const float* __restrict__ cm_t,
              const float* __restrict__ d_out, const float* __restrict__ s_next, const float* __restrict__ keep_next,
              float* __restrict__ s_t, float* __restrict__ dh_ws, float* __restrict__ dc_ws) {
  __shared__ float tile[16 * (MS_KC + 4)];
  const int pitch = MS_KC + 4;
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  const int bl = lane & 15, kg = lane >> 4;
  const int b0 = (int)blockIdx.x * 16, b = b0 + bl;
  const int j0 = ((int)blockIdx.y * MS_WAVES + wave) * 16;
  const bool active = j0 < H;
  const int j4 = j0 + 4 * kg;
  const bool valid = active && b < B;
  float* grow = gates + (valid ? (size_t)b * N * 4 * H + j4 : 0);
  const float* drow = d_out + (valid ? (size_t)b * N * H + j4 : 0);
  // activated gates and output gradients of the first MS_PRE samples: loaded before the prologue, used after it
  ms_f4 pre[MS_PRE][5];
#pragma unroll
  for (int n = 0; n < MS_PRE; ++n)
    if (valid && n < N) {
#pragma unroll
      for (int g = 0; g < 4; ++g) pre[n][g] = ms_ld4(grow + (size_t)n * 4 * H + g * H);
      pre[n][4] = ms_ld4(drow + (size_t)n * H);
    }
  ms_f4 dhb = {0.0f, 0.0f, 0.0f, 0.0f}, dcb = {0.0f, 0.0f, 0.0f, 0.0f};
  if (s_next) {
    ms_f4 acc[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) acc[a] = ms_f4{0.0f, 0.0f, 0.0f, 0.0f};
    const int K = 4 * H;                   // a multiple of 64, and so is every chunk
    for (int k0 = 0; k0 < K; k0 += MS_KC) {
      const int kc = K - k0 < MS_KC ? K - k0 : MS_KC;
      if (k0) __syncthreads();             // every wave has read the previous chunk
      ms_stage(tile, pitch, s_next, K, k0, kc, nullptr, b0, B);
      __syncthreads();
      if (active) {
        const float* srow = tile + bl * pitch + 4 * kg;
        const float* wcol = w + (size_t)(k0 + 4 * kg) * H + j0 + bl;
        // 64 k per round: the 16 W operands of the next round are in flight under the 16 MFMAs of this one
        float nxt[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) nxt[i] = wcol[(size_t)(16 * (i >> 2) + (i & 3)) * H];
        for (int k = 0; k < kc; k += 64) {
          float cur[16];
#pragma unroll
          for (int i = 0; i < 16; ++i) cur[i] = nxt[i];
          if (k + 64 < kc) {
#pragma unroll
            for (int i = 0; i < 16; ++i) nxt[i] = wcol[(size_t)(k + 64 + 16 * (i >> 2) + (i & 3)) * H];
          }
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const ms_f4 sv = ms_ld4(srow + k + 16 * i);
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) acc[jj] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur[4 * i + jj], sv[jj], acc[jj], 0, 0, 0);
          }
        }
      }
    }
    dhb = (acc[0] + acc[1]) + (acc[2] + acc[3]);
  }
  if (!valid) return;
  if (s_next) {
    const float kn = keep_next[b];
    dhb *= kn;
    dcb = ms_ld4(dc_ws + (size_t)b * H + j4) * kn;
  }
  ms_st4(dh_ws + (size_t)b * H + j4, dhb);
  const float inv = 1.0f / (float)N;
  dhb *= inv; dcb *= inv;
  const ms_f4 cin = ms_ld4(cm_t + (size_t)b * H + j4);
  ms_f4 si = {0.0f, 0.0f, 0.0f, 0.0f}, sf = si, sg = si, so = si, dcin = si;
  auto cell = [&](int n, const ms_f4 (&a)[5]) {
    float* gp = grow + (size_t)n * 4 * H;
    ms_f4 di, df, dg, dd;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float gi = a[0][r], gf = a[1][r], gg = a[2][r], go = a[3][r];
      const float c = gf * cin[r] + gi * gg;                   // the forward's own expression: the same bits
      const float tc = ms_tanh(c);
      const float dh = a[4][r] + dhb[r];
      const float dc = dcb[r] + dh * go * (1.0f - tc * tc);
      di[r] = dc * gg * gi * (1.0f - gi);
      df[r] = dc * cin[r] * gf * (1.0f - gf);
      dg[r] = dc * gi * (1.0f - gg * gg);
      dd[r] = dh * tc * go * (1.0f - go);
      dcin[r] += dc * gf;
    }
    ms_st4(gp, di); ms_st4(gp + H, df); ms_st4(gp + 2 * H, dg); ms_st4(gp + 3 * H, dd);
    si += di; sf += df; sg += dg; so += dd;
  };
#pragma unroll
  for (int n = 0; n < MS_PRE; ++n)
    if (n < N) cell(n, pre[n]);
  for (int n = MS_PRE; n < N; ++n) {
    ms_f4 a[5];
#pragma unroll
    for (int g = 0; g < 4; ++g) a[g] = ms_ld4(grow + (size_t)n * 4 * H + g * H);
    a[4] = ms_ld4(drow + (size_t)n * H);
    cell(n, a);
  }
  float* sp = s_t + (size_t)b * 4 * H + j4;
  ms_st4(sp, si); ms_st4(sp + H, sf); ms_st4(sp + 2 * H, sg); ms_st4(sp + 3 * H, so);
  ms_st4(dc_ws + (size_t)b * H + j4, dcin);
}

static bool ms_shape_ok(int32_t T, int32_t B, int32_t N, int32_t H) {
  return T >= 1 && B >= 1 && N >= 2 && N <= 64 && H >= 16 && H <= 1024 && H % 16 == 0;
}
static bool ms_aligned(const void* p) { return ((uintptr_t)p & 15u) == 0; }
static dim3 ms_grid(int32_t B, int32_t H) { return dim3((unsigned)((B + 15) / 16), (unsigned)((H / 16 + MS_WAVES - 1) / MS_WAVES)); }

}  // namespace mirl

using namespace mirl;

extern "C" int mirl_lstm_ms_supported(int32_t T, int32_t B, int32_t N, int32_t H) { return ms_shape_ok(T, B, N, H) ? 1 : 0; }

extern "C" int mirl_lstm_ms_fwd(int32_t T, int32_t B, int32_t N, int32_t H, float* gates, const float* w_hh, const float* h0,
                                const float* c0, const float* keep, float* out, float* hm, float* cm, float* h_last,
                                float* c_last, int32_t need_grad, void* stream) {
  if (!ms_shape_ok(T, B, N, H)) return fail(MIRL_ERR_ARG, "lstm_ms_fwd: unsupported shape (mirl_lstm_ms_supported)");
  if (!gates || !w_hh || !h0 || !c0 || !keep || !out || !hm || !cm || (!h_last != !c_last))
    return fail(MIRL_ERR_ARG, "bad lstm_ms_fwd arguments");
  if (!ms_aligned(gates) || !ms_aligned(w_hh) || !ms_aligned(h0) || !ms_aligned(c0) || !ms_aligned(out) || !ms_aligned(hm) ||
      !ms_aligned(cm) || !ms_aligned(h_last) || !ms_aligned(c_last))
    return fail(MIRL_ERR_ARG, "lstm_ms_fwd: operands must be 16-byte aligned");
  const size_t lds = (size_t)16 * (H + 4) * sizeof(float);
  if (lds > 65536) { int rc = raise_lds_limit(k_lstm_ms_fwd, lds); if (rc != MIRL_OK) return rc; }
  hipStream_t st = (hipStream_t)stream;
  const size_t BH = (size_t)B * H, row = (size_t)B * N;
  ProfScope ps("k_lstm_ms_fwd", (double)T * 4.0 * (row * H * (need_grad ? 9.0 : 5.0) + 4.0 * H * H * ((B + 15) / 16) + 4.0 * BH), st,
               (double)T * 2.0 * 16.0 * ((B + 15) / 16) * H * 4.0 * H);
  const dim3 grid = ms_grid(B, H);
  for (int32_t t = 0; t < T; ++t) {
    const bool last = t == T - 1;
    hipLaunchKernelGGL(k_lstm_ms_fwd, grid, dim3(MS_WAVES * 64), lds, st, (int)B, (int)N, (int)H, gates + (size_t)t * row * 4 * H, w_hh,
                       t ? hm + t * BH : h0, t ? cm + t * BH : c0, t ? (const float*)nullptr : keep, hm, cm,
                       last ? (const float*)nullptr : keep + (size_t)(t + 1) * B, out + (size_t)t * row * H, hm + (t + 1) * BH,
                       cm + (t + 1) * BH, last ? h_last : (float*)nullptr, last ? c_last : (float*)nullptr, need_grad ? 1 : 0);
    MIRL_LAUNCH_CHECK();
  }
  return MIRL_OK;
}

extern "C" int mirl_lstm_ms_bwd(int32_t T, int32_t B, int32_t N, int32_t H, float* gates, const float* w_hh, const float* cm,
                                const float* d_out, const float* keep, float* S, float* dh_ws, float* dc_ws, void* stream) {
  if (!ms_shape_ok(T, B, N, H)) return fail(MIRL_ERR_ARG, "lstm_ms_bwd: unsupported shape (mirl_lstm_ms_supported)");
  if (!gates || !w_hh || !cm || !d_out || !keep || !S || !dh_ws || !dc_ws) return fail(MIRL_ERR_ARG, "bad lstm_ms_bwd arguments");
  if (!ms_aligned(gates) || !ms_aligned(w_hh) || !ms_aligned(cm) || !ms_aligned(d_out) || !ms_aligned(S) || !ms_aligned(dh_ws) ||
      !ms_aligned(dc_ws))
    return fail(MIRL_ERR_ARG, "lstm_ms_bwd: operands must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const size_t BH = (size_t)B * H, row = (size_t)B * N;
  ProfScope ps("k_lstm_ms_bwd", (double)T * 4.0 * (row * H * 9.0 + 4.0 * H * H * ((B + 15) / 16) + 8.0 * BH), st,
               (double)(T - 1) * 2.0 * 16.0 * ((B + 15) / 16) * H * 4.0 * H);
  const dim3 grid = ms_grid(B, H);
  for (int32_t t = T - 1; t >= 0; --t) {
    const bool last = t == T - 1;
    hipLaunchKernelGGL(k_lstm_ms_bwd, grid, dim3(MS_WAVES * 64), 0, st, (int)B, (int)N, (int)H, gates + (size_t)t * row * 4 * H, w_hh,
                       cm + t * BH, d_out + (size_t)t * row * H, last ? (const float*)nullptr : S + (size_t)(t + 1) * 4 * BH,
                       last ? (const float*)nullptr : keep + (size_t)(t + 1) * B, S + (size_t)t * 4 * BH, dh_ws, dc_ws);
    MIRL_LAUNCH_CHECK();
  }
  return MIRL_OK;
}
