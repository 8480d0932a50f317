// lstm_extras.hip — the extra-feature columns of the LSTM's input projection without the concatenation.
//
// The reference appends X floats (one-hot last action, scaled timestep, clipped last reward:
// rltime/env_wrappers/common.py ExtraFeaturesEnvWrapper) to the conv features and multiplies the concatenated row with
// W_ih (rltime/models/torch/sequential.py:155-166, modules/lstm.py:60-81).  The product splits:
//
//     [f | e] W_ih^T = f W_ih[:, :F]^T + e W_ih[:, F:]^T
//
// the first term is the K = F product the split-bf16 GEMM runs (and can be shared between passes), the second a rank-X
// correction, X <= 32, that needs no matrix pipe:
//
//   k_lstm_extras_add     dst[r][n] = src[r][n] + sum_x e[r][x] wx[n][x]   one read and one write of the gates block
//   k_lstm_extras_wgrad   dwx[n][x] = sum_r g[r][n] e[r][x]                one read of the gate gradients
//
// Both give every lane one float4 of columns (a wave = one 256-column strip) and read a row's X extras as wave-uniform
// scalars; neither uses atomics, so reruns are bit-identical.
#include "common.hpp"

namespace mirl {

typedef float xf4 __attribute__((ext_vector_type(4)));

static const int kXMax = 32;          // extras per row the kernels take
static const int kStrip = 256;        // columns per wave: 64 lanes x one float4
static const int kAddRows = 4;        // rows a wave carries per pass over its weights
static const int kWgradChunk = 256;   // rows per workgroup of the weight gradient: 4 waves x 64 rows

// Workgroup (strip, range of rows): the strip's 256 x X weights are staged once in LDS, x-major, so a lane's float4 of
// one x is a conflict-free 16-byte read; every wave then walks its share of the rows four at a time, so one read of the
// weights serves four rows.  Per element: acc = src, then for x ascending acc = acc + (e * w), product and sum each
// rounded (the build has -ffp-contract=off) — restated by tests/lstm_extras_restate.py.
__global__ void __launch_bounds__(256)
k_lstm_extras_add(int64_t M, int64_t N, int X, const float* src, int64_t ldsrc, const float* __restrict__ e, int64_t lde,
                  const float* __restrict__ wx, int64_t ldwx, float* dst, int64_t lddst, int64_t rows_per_wg) {
  __shared__ xf4 s_w[kXMax * 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t n0 = (int64_t)blockIdx.y * kStrip;
  float* s_wf = (float*)s_w;
  for (int i = tid; i < kStrip * X; i += 256) {
    int c = i / X, x = i - c * X;
    s_wf[x * kStrip + c] = n0 + c < N ? wx[(n0 + c) * ldwx + x] : 0.f;
  }
  __syncthreads();
  const int64_t col = n0 + 4 * lane;
  const bool live = col < N;           // N % 4 == 0: a lane's four columns are all inside or all outside
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
  int64_t r1 = r0 + rows_per_wg; if (r1 > M) r1 = M;
  for (int64_t r = r0 + (int64_t)wave * kAddRows; r < r1; r += 4 * kAddRows) {
    xf4 acc[kAddRows];
#pragma unroll
    for (int k = 0; k < kAddRows; ++k) {
      acc[k] = (xf4){0.f, 0.f, 0.f, 0.f};
      if (live && r + k < r1) acc[k] = *(const xf4*)(src + (r + k) * ldsrc + col);
    }
    for (int x = 0; x < X; ++x) {
      xf4 w = s_w[x * 64 + lane];
#pragma unroll
      for (int k = 0; k < kAddRows; ++k) {
        float ev = r + k < r1 ? e[(r + k) * lde + x] : 0.f;        // wave-uniform: a scalar load
        xf4 p = w * ev;
        acc[k] = acc[k] + p;
      }
    }
#pragma unroll
    for (int k = 0; k < kAddRows; ++k)
      if (live && r + k < r1) *(xf4*)(dst + (r + k) * lddst + col) = acc[k];
  }
}

// Workgroup (chunk of 256 rows, strip): wave w takes rows [64 w, 64 w + 64) of the chunk in ascending order with 4 x XP
// accumulators per lane (XP = X rounded up to a multiple of 4; the padding columns multiply zeros), the four waves' sums
// are then added in LDS in the fixed order ((w0 + w3) + w2) + w1 and the chunk's partial goes to out[chunk][n][x].
template <int XP>
__global__ void __launch_bounds__(256)
k_lstm_extras_wgrad(int64_t M, int64_t N, int X, const float* __restrict__ g, int64_t ldg, const float* __restrict__ e,
                    int64_t lde, float* __restrict__ out) {
  __shared__ float s_red[4 * XP * 64];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t col = (int64_t)blockIdx.y * kStrip + 4 * lane;
  const bool live = col < N;
  const int64_t r0 = (int64_t)blockIdx.x * kWgradChunk + (int64_t)wave * 64;
  int64_t r1 = r0 + 64; if (r1 > M) r1 = M;
  float acc[4][XP];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int x = 0; x < XP; ++x) acc[j][x] = 0.f;
  if (live) {
#pragma unroll XP <= 12 ? 2 : 1       // two rows of scalars in flight where they fit the scalar registers
    for (int64_t r = r0; r < r1; ++r) {
      xf4 gv = *(const xf4*)(g + r * ldg + col);
#pragma unroll
      for (int x = 0; x < XP; ++x) {
        float ev = x < X ? e[r * lde + x] : 0.f;                    // wave-uniform: a scalar load
        acc[0][x] = __builtin_fmaf(gv.x, ev, acc[0][x]);
        acc[1][x] = __builtin_fmaf(gv.y, ev, acc[1][x]);
        acc[2][x] = __builtin_fmaf(gv.z, ev, acc[2][x]);
        acc[3][x] = __builtin_fmaf(gv.w, ev, acc[3][x]);
      }
    }
  }
  for (int w = 3; w >= 1; --w) {
    if (wave == w) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int x = 0; x < XP; ++x) s_red[(j * XP + x) * 64 + lane] = acc[j][x];
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int x = 0; x < XP; ++x) acc[j][x] = acc[j][x] + s_red[(j * XP + x) * 64 + lane];
    }
    __syncthreads();
  }
  if (wave == 0 && live) {
    float* o = out + ((int64_t)blockIdx.x * N + col) * X;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int x = 0; x < XP; ++x)
        if (x < X) o[j * X + x] = acc[j][x];
  }
}

// dwx[i] = sum over the chunks, ascending, of partial[chunk][i]
__global__ void __launch_bounds__(256)
k_lstm_extras_wgrad_sum(int64_t n, int64_t chunks, const float* __restrict__ partial, float* __restrict__ dwx) {
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = partial[i];
  for (int64_t c = 1; c < chunks; ++c) s = s + partial[c * n + i];
  dwx[i] = s;
}

static inline int64_t wgrad_chunks(int64_t M) { return (M + kWgradChunk - 1) / kWgradChunk; }

}  // namespace mirl

using namespace mirl;

extern "C" int mirl_lstm_extras_supported(int64_t M, int64_t N, int32_t X) {
  return M >= 1 && N >= 4 && N % 4 == 0 && X >= 1 && X <= kXMax ? 1 : 0;
}

extern "C" int mirl_lstm_extras_add(int64_t M, int64_t N, int32_t X, const float* src, int64_t ldsrc, const float* e, int64_t lde,
                                    const float* wx, int64_t ldwx, float* dst, int64_t lddst, void* stream) {
  if (!mirl_lstm_extras_supported(M, N, X) || !src || !e || !wx || !dst) return fail(MIRL_ERR_ARG, "bad lstm_extras_add arguments");
  if (ldsrc < N || lddst < N || ldsrc % 4 || lddst % 4 || !aligned16(src, dst) || lde < X || ldwx < X)
    return fail(MIRL_ERR_ARG, "lstm_extras_add: src / dst must be 16-byte aligned with leading dimensions >= N that are multiples of 4; lde, ldwx >= X");
  const int64_t strips = (N + kStrip - 1) / kStrip;
  if (strips > 65535) return fail(MIRL_ERR_ARG, "lstm_extras_add: N too large");
  // ~2048 workgroups at the most (8 per compute unit), each walking a multiple of the 16 rows its four waves take per pass
  int64_t groups = (M + 4 * kAddRows - 1) / (4 * kAddRows);
  int64_t cap = 2048 / strips > 0 ? 2048 / strips : 1;
  int64_t wgs = groups < cap ? groups : cap;
  int64_t rows_per_wg = (groups + wgs - 1) / wgs * (4 * kAddRows);
  wgs = (M + rows_per_wg - 1) / rows_per_wg;
  ProfScope ps("k_lstm_extras_add", 4.0 * ((double)M * N * 2 + (double)M * X + (double)N * X), (hipStream_t)stream);
  hipLaunchKernelGGL(k_lstm_extras_add, dim3((unsigned)wgs, (unsigned)strips), dim3(256), 0, (hipStream_t)stream, M, N, (int)X, src, ldsrc,
                     e, lde, wx, ldwx, dst, lddst, rows_per_wg);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_lstm_extras_wgrad_workspace_bytes(int64_t M, int64_t N, int32_t X, int64_t* bytes) {
  if (!bytes || !mirl_lstm_extras_supported(M, N, X)) return fail(MIRL_ERR_ARG, "bad lstm_extras_wgrad_workspace_bytes arguments");
  const int64_t chunks = wgrad_chunks(M);
  *bytes = chunks > 1 ? chunks * N * X * 4 : 0;          // one chunk writes dwx itself
  return MIRL_OK;
}

extern "C" int mirl_lstm_extras_wgrad(int64_t M, int64_t N, int32_t X, const float* g, int64_t ldg, const float* e, int64_t lde,
                                      float* dwx, void* ws, int64_t ws_bytes, void* stream) {
  if (!mirl_lstm_extras_supported(M, N, X) || !g || !e || !dwx) return fail(MIRL_ERR_ARG, "bad lstm_extras_wgrad arguments");
  if (ldg < N || ldg % 4 || !aligned16(g) || lde < X)
    return fail(MIRL_ERR_ARG, "lstm_extras_wgrad: g must be 16-byte aligned with a leading dimension >= N that is a multiple of 4; lde >= X");
  const int64_t chunks = wgrad_chunks(M), strips = (N + kStrip - 1) / kStrip;
  if (strips > 65535) return fail(MIRL_ERR_ARG, "lstm_extras_wgrad: N too large");
  const int64_t need = chunks > 1 ? chunks * N * X * 4 : 0;
  if (need && (!ws || ws_bytes < need || ((uintptr_t)ws % 4))) return fail(MIRL_ERR_ARG, "lstm_extras_wgrad: workspace too small (mirl_lstm_extras_wgrad_workspace_bytes)");
  float* out = chunks > 1 ? (float*)ws : dwx;
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)chunks, (unsigned)strips);
  {
    ProfScope ps("k_lstm_extras_wgrad", 4.0 * ((double)M * N + (double)M * X + (double)chunks * N * X), st);
    switch ((X + 3) / 4) {
#define MIRL_XW(q) case q: hipLaunchKernelGGL(k_lstm_extras_wgrad<4 * q>, grid, dim3(256), 0, st, M, N, (int)X, g, ldg, e, lde, out); break;
      MIRL_XW(1) MIRL_XW(2) MIRL_XW(3) MIRL_XW(4) MIRL_XW(5) MIRL_XW(6) MIRL_XW(7) MIRL_XW(8)
#undef MIRL_XW
    }
    MIRL_LAUNCH_CHECK();
  }
  if (chunks > 1) {
    const int64_t n = N * X;
    ProfScope ps("k_lstm_extras_wgrad_sum", 4.0 * ((double)chunks * n + (double)n), st);
    hipLaunchKernelGGL(k_lstm_extras_wgrad_sum, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, chunks, (const float*)ws, dwx);
    MIRL_LAUNCH_CHECK();
  }
  return MIRL_OK;
}
