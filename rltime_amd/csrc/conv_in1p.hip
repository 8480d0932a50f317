// conv_in1p.hip — the input layer from ONE-plane uint8 frames: the second kernel family next to csrc/conv_in.hip.
//
// Reference: rltime/configs/atari_iqn_lstm.json with env_wrappers/atari_lstm.json trains on unstacked frames
// ("stack": 1, observations (1, 84, 84) uint8): the LSTM carries the history, and one plane per step makes the replay
// and every frame transfer four times smaller.  The layer is cnn.py:44-49 as in conv_in.hip — `x.float() * scale`,
// `F.relu(conv(x))` — at Conv2d(1 -> 32, kernel 8, stride 4).  conv_in.hip's kernels give one MFMA k-group to one
// PLANE; with a single plane three quarters of every instruction would multiply zeros, so this family turns the
// operand around: a k-group is one KERNEL ROW.
//
// Forward (k_conv1p_u8_fwd), bf16 matrix pipe, f32 result.  A uint8 pixel is exact in bf16 and w * scale is split
// exactly into three bf16 parts (g3_split4), so every product is exact in the MFMA's f32 accumulator.
//   contraction   v_mfma_f32_16x16x32_bf16, filters as rows, 16 output positions as columns; k group lane >> 4 = kernel
//                 row kh (mod 4), a lane's 8 k-elements = the 8 bytes x[4 oh + kh][4 ow .. 4 ow + 7] of that row: one
//                 instruction covers kh = 0..3, a second one kh = 4..7.  2 x 2 filter halves x 3 parts = 12 MFMAs per
//                 16-position tile (the 4-plane kernel: 48).
//   operands      all 12 weight operands of a lane stay in registers (48 VGPRs): no weight LDS.  The three parts run on
//                 separate accumulator chains and are added smallest first, then the bias: an output's summation order
//                 does not depend on N, the split or the frames per fill.
//   work split    persistent workgroups (4 waves); a work unit stages up to 4 consecutive frames (raw bytes, one
//                 contiguous run of 16 B vectors) and walks their tiles, one per wave at a time; at small N `split`
//                 workgroups share one frame's tiles so that acting batches fill the chip.
//   epilogue      + bias, ReLU, two 16 B stores per lane; a wave writes 2 KiB of contiguous NHWC rows.
//   HBM traffic   7 KB in + 51 KB out per 84 x 84 frame: the kernel is bound by its output stores.
//
// Weight gradient (k_conv1p_u8_wrw), bf16 pipe with the exact three-way split of g, as k_conv1_u8_wrw_b3: rows = 16
// filters, columns = 16 taps, K = 32 positions walked in octets of 8 consecutive ow (the tail octet carries g = 0), the
// frame staged once as bf16, 64 taps = 4 tap groups x 2 filter halves: the whole 32 x 64 result stays in registers as 8
// accumulator tiles, the three parts enter smallest first.  Per-workgroup slabs are summed in slab order by
// k_conv1p_wrw_reduce: fixed partition, fixed order, no float atomics.  The masked form applies y > 0 while dy is
// loaded and carries the bias gradient behind the slab's 2048 weight sums.
// Autograd wiring: rltime_amd/models/torch/fused.py:_ConvU8P1BiasReLU.
#include "common.hpp"
#include "split3.hpp"
#include <unordered_set>

namespace mirl {

constexpr int C1P_K = 8, C1P_S = 4, C1P_F = 32, C1P_TAPS = C1P_K * C1P_K;
constexpr int C1P_WPK = 3 * 2 * 2 * 64 * 4;    // packed weight image in floats: [part][kh half][filter half][lane] x 16 B
constexpr int C1P_LD = 7;                      // staging loads in flight per lane (four 84x84 frames = 6.9 x 256 vectors)
constexpr int C1P_FPI = 4;                     // most frames per LDS fill
constexpr int C1P_DW = C1P_F * C1P_TAPS;       // 2048 weight-gradient elements
constexpr int C1P_SLAB = C1P_DW + C1P_F;       // floats per workgroup slab: weight sums, then the bias sums (masked form)
constexpr int C1P_WGS = 1024;                  // weight gradient: most workgroups = slabs (4 per CU)
constexpr int C1P_FWD_WGS = 1024;              // forward: most resident workgroups

// wpk3[((part*2 + hh)*2 + m)*64 + lane] = 8 bf16 (kw = 0..7) of part `part` of w[f][0][kh][kw] * scale with the A-operand
// lane map row i = lane & 15 -> filter f = (i>>2)*8 + m*4 + (i&3) (the 4 accumulator rows a lane owns are 4 CONSECUTIVE
// filters, as k_conv1_pack_w), k group lane >> 4 -> kernel row kh = 4 hh + (lane >> 4)
__global__ void __launch_bounds__(256)
k_conv1p_pack_w(const float* __restrict__ w, int64_t so, int64_t sh, int64_t sw, float scale, uint4* __restrict__ wpk3) {
  const int t = threadIdx.x;
  const int lane = t & 63, m = (t >> 6) & 1, hh = t >> 7;
  const int i = lane & 15, kh = 4 * hh + (lane >> 4);
  const int f = (i >> 2) * 8 + m * 4 + (i & 3);
  float v[2][4];
#pragma unroll
  for (int kw = 0; kw < C1P_K; ++kw) v[kw >> 2][kw & 3] = w[f * so + kh * sh + kw * sw] * scale;   // x*scale*w summed as x*(scale*w)
  uint2 h0, m0, l0, h1, m1, l1;
  g3_split4(v[0], h0, m0, l0);
  g3_split4(v[1], h1, m1, l1);
  const int o = (hh * 2 + m) * 64 + lane;
  wpk3[o] = make_uint4(h0.x, h0.y, h1.x, h1.y);
  wpk3[4 * 64 + o] = make_uint4(m0.x, m0.y, m1.x, m1.y);
  wpk3[8 * 64 + o] = make_uint4(l0.x, l0.y, l1.x, l1.y);
}

__device__ __forceinline__ g3_bf16x8 c1p_as_bf8(uint4 v) { return __builtin_bit_cast(g3_bf16x8, v); }
__device__ __forceinline__ float c1p_byte(uint32_t v, int b) { return (float)((v >> (8 * b)) & 0xffu); }
// bytes (2e, 2e+1) of v -> two bf16 in one dword (the upper half of float(byte) is the exact bf16)
__device__ __forceinline__ unsigned c1p_bytes_bf(uint32_t v, int e) {
  return __builtin_amdgcn_perm(__float_as_uint(c1p_byte(v, 2 * e + 1)), __float_as_uint(c1p_byte(v, 2 * e)), 0x07060302u);
}
// 8 consecutive bytes (two dwords) -> the lane's 8 bf16 k-elements
__device__ __forceinline__ g3_bf16x8 c1p_row_bf(uint32_t a, uint32_t b) {
  return c1p_as_bf8(make_uint4(c1p_bytes_bf(a, 0), c1p_bytes_bf(a, 1), c1p_bytes_bf(b, 0), c1p_bytes_bf(b, 1)));
}
__device__ __forceinline__ g3_f32x4 c1p_relu(g3_f32x4 o) {
  o.x = o.x > 0.f ? o.x : 0.f; o.y = o.y > 0.f ? o.y : 0.f; o.z = o.z > 0.f ? o.z : 0.f; o.w = o.w > 0.f ? o.w : 0.f;
  return o;
}

// x: uint8 [N][1][H][W]; y: float [N][OH][OW][32].  Work unit u = (frame group, part): a group is `fpi` consecutive
// frames, `split` parts share a group's tiles (split > 1 only with fpi = 1).  Plain (cached) output stores: measured
// 0.61 against 0.83 ms per 41 472 frames with non-temporal ones (docs/measurement.md).
__global__ void __launch_bounds__(256, 4)
k_conv1p_u8_fwd(int N, int W, int OW, int HW, int OHW, int tiles, unsigned ow_magic, unsigned tiles_magic, int fpi, int split,
                const uint8_t* __restrict__ x, const uint4* __restrict__ wpk3, const float* __restrict__ bias,
                float* __restrict__ y) {
  extern __shared__ __align__(16) uint8_t c1p_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, kq = lane >> 4;
  g3_bf16x8 wt[3][2][2];                            // [part][kh half][filter half]
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
      for (int m = 0; m < 2; ++m) wt[p][hh][m] = c1p_as_bf8(wpk3[((p * 2 + hh) * 2 + m) * 64 + lane]);
  const g3_f32x4 b0 = *reinterpret_cast<const g3_f32x4*>(bias + kq * 8), b1 = *reinterpret_cast<const g3_f32x4*>(bias + kq * 8 + 4);
  const int hw16 = HW >> 4, row_off = kq * W;
  const int groups = (N + fpi - 1) / fpi, units = groups * split, step = 4 * split;
  bool first = true;
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int group = split == 1 ? u : u / split, part = u - group * split;
    const int n0 = group * fpi;
    const int frames = N - n0 < fpi ? N - n0 : fpi;
    if (!first) __syncthreads();                    // every wave is done reading the previous frames
    first = false;
    {
      // `frames` one-plane frames are one contiguous run of 16 B vectors, in HBM and in LDS
      const int vecs = frames * hw16;
      const uint4* s4 = reinterpret_cast<const uint4*>(x + (int64_t)n0 * HW);
      uint4* d4 = reinterpret_cast<uint4*>(c1p_lds);
      for (int o0 = tid; o0 < vecs; o0 += 256 * C1P_LD) {
        uint4 v[C1P_LD];
#pragma unroll
        for (int k = 0; k < C1P_LD; ++k) { const int o = o0 + k * 256; v[k] = s4[o < vecs ? o : vecs - 1]; }
#pragma unroll
        for (int k = 0; k < C1P_LD; ++k) { const int o = o0 + k * 256; if (o < vecs) d4[o] = v[k]; }
      }
    }
    __syncthreads();
    const int tend = frames * tiles;
    int tt = part * 4 + wave;                       // this wave's tiles: tt, + step, ... < frames * tiles
    if (tt >= tend) continue;
    // tile -> (frame f, position p); the lane's two pixel rows kh = kq and kq + 4, 8 bytes each
    int f, p;
    uint32_t px[4];
#define C1P_TILE_READ(tt_, f_, p_, px_)                                                         \
    {                                                                                           \
      f_ = tiles == 1 ? tt_ : (int)__umulhi((unsigned)(tt_), tiles_magic);                      \
      p_ = (tt_ - f_ * tiles) * 16 + j;                                                         \
      const int pc_ = p_ < OHW ? p_ : OHW - 1;                                                  \
      const int oh_ = OW == 1 ? pc_ : (int)__umulhi((unsigned)pc_, ow_magic);                   \
      const uint8_t* base_ = c1p_lds + f_ * HW + (oh_ * C1P_S) * W + (pc_ - oh_ * OW) * C1P_S + row_off; \
      px_[0] = *reinterpret_cast<const uint32_t*>(base_);                                       \
      px_[1] = *reinterpret_cast<const uint32_t*>(base_ + 4);                                   \
      px_[2] = *reinterpret_cast<const uint32_t*>(base_ + 4 * W);                               \
      px_[3] = *reinterpret_cast<const uint32_t*>(base_ + 4 * W + 4);                           \
    }
    C1P_TILE_READ(tt, f, p, px);
    for (;;) {
      const int tn = tt + step;
      int fn = 0, pn = 0;
      uint32_t pxn[4] = {0u, 0u, 0u, 0u};
      if (tn < tend) C1P_TILE_READ(tn, fn, pn, pxn);   // the next tile's LDS words in flight before this tile's chain
      const g3_bf16x8 ba = c1p_row_bf(px[0], px[1]), bb = c1p_row_bf(px[2], px[3]);
      const g3_f32x4 z = {0.f, 0.f, 0.f, 0.f};
      g3_f32x4 l0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[2][0][0], ba, z, 0, 0, 0);
      g3_f32x4 l1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[2][0][1], ba, z, 0, 0, 0);
      g3_f32x4 m0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[1][0][0], ba, z, 0, 0, 0);
      g3_f32x4 m1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[1][0][1], ba, z, 0, 0, 0);
      g3_f32x4 h0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[0][0][0], ba, z, 0, 0, 0);
      g3_f32x4 h1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[0][0][1], ba, z, 0, 0, 0);
      l0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[2][1][0], bb, l0, 0, 0, 0);
      l1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[2][1][1], bb, l1, 0, 0, 0);
      m0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[1][1][0], bb, m0, 0, 0, 0);
      m1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[1][1][1], bb, m1, 0, 0, 0);
      h0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[0][1][0], bb, h0, 0, 0, 0);
      h1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[0][1][1], bb, h1, 0, 0, 0);
      if (p < OHW) {
        const g3_f32x4 o0 = c1p_relu(((l0 + m0) + h0) + b0), o1 = c1p_relu(((l1 + m1) + h1) + b1);
        g3_f32x4* dst = reinterpret_cast<g3_f32x4*>(y + ((n0 + f) * (int64_t)OHW + p) * C1P_F + kq * 8);
        dst[0] = o0; dst[1] = o1;
      }
      if (tn >= tend) break;
      tt = tn; f = fn; p = pn;
#pragma unroll
      for (int k = 0; k < 4; ++k) px[k] = pxn[k];
    }
#undef C1P_TILE_READ
  }
}

// LDS halfwords of the bf16 frame: the frame, the over-read of a row's tail octet (its positions beyond OW carry g = 0 but
// are still read: the last index is (H - 1) W + 32 ceil(OW / 8) + 3), rounded to 16 bytes
static int c1p_bf_pitch(int HW, int OW) { return (HW + 4 * (8 * ((OW + 7) / 8) - OW) + 8 + 7) / 8 * 8; }

// dW[f][0][kh][kw] = scale * sum over (n, oh, ow) of g[n][oh][ow][f] * float(x[n][0][4 oh + kh][4 ow + kw]).  Lane (j, kq) of a
// K-step owns octet 4 ks + kq: its 8 A values are g[oh][ow0 .. ow0 + 7][filter j + 16 m], its 8 B values for tap
// (kh, kw) the pixels x[4 oh + kh][4 (ow0 + e) + kw], e < 8.  Tap group t < 4: kh = 2 t + (j >> 3), kw = j & 7, so that
// t * 16 + j IS the flattened (kh, kw) index.  Frame n goes to workgroup n % gridDim.x.
template <bool MASK>
__global__ void __launch_bounds__(256, 2)
k_conv1p_u8_wrw(int N, int H, int W, int OH, int OW, int Pd, const uint8_t* __restrict__ x, const float* __restrict__ g,
                float* __restrict__ partial, const float* __restrict__ yv) {
  extern __shared__ __align__(16) uint8_t c1p_lds[];
  uint16_t* px = reinterpret_cast<uint16_t*>(c1p_lds);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, kq = lane >> 4;
  const int HW = H * W, OHW = OH * OW, hw16 = HW >> 4;
  const int no = (OW + 7) >> 3, octets = OH * no, ksteps = (octets + 3) >> 2;
  const int tap_off = (j >> 3) * W + (j & 7);
  float dbs[2] = {0.f, 0.f};
  g3_f32x4 acc0[4], acc1[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) { acc0[t] = g3_f32x4{0.f, 0.f, 0.f, 0.f}; acc1[t] = g3_f32x4{0.f, 0.f, 0.f, 0.f}; }
  // the slack behind the frame is read (tail octets) but never staged: zero it once — any finite value would do, times g = 0
  for (int i = HW + tid; i < Pd; i += 256) px[i] = 0;
  bool first = true;
  for (int n = blockIdx.x; n < N; n += gridDim.x) {
    if (!first) __syncthreads();                  // every wave is done reading the previous frame
    first = false;
    {
      // 16 pixels -> 16 bf16 = two 16 B LDS stores
      const uint4* s4 = reinterpret_cast<const uint4*>(x + (int64_t)n * HW);
      for (int o0 = tid; o0 < hw16; o0 += 256 * 2) {
        uint4 v[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) { const int o = o0 + k * 256; v[k] = s4[o < hw16 ? o : hw16 - 1]; }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int o = o0 + k * 256;
          if (o < hw16) {
            const uint32_t wv[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
            uint32_t h[8];
#pragma unroll
            for (int d = 0; d < 4; ++d) { h[2 * d] = c1p_bytes_bf(wv[d], 0); h[2 * d + 1] = c1p_bytes_bf(wv[d], 1); }
            uint4* d4 = reinterpret_cast<uint4*>(px + o * 16);
            d4[0] = make_uint4(h[0], h[1], h[2], h[3]);
            d4[1] = make_uint4(h[4], h[5], h[6], h[7]);
          }
        }
      }
    }
    __syncthreads();
    const float* gf = g + (int64_t)n * OHW * C1P_F + j;
    // the NEXT K-step's g (and y) values are requested before this K-step's split and MFMAs
    float gn[2][8], yn[2][8];
    auto request = [&](int ks) {
      const int o = ks * 4 + kq;
      const int ohr = o / no, ow0 = (o - ohr * no) * 8;
      const int oh = ohr < OH ? ohr : OH - 1;
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const int ow = ow0 + e;
          const int off = (oh * OW + (ow < OW ? ow : OW - 1)) * C1P_F + 16 * m;
          gn[m][e] = gf[off];
          if (MASK) yn[m][e] = yv[(gf - g) + off];
        }
    };
    if (wave < ksteps) request(wave);
    for (int ks = wave; ks < ksteps; ks += 4) {
      // this lane's octet: 8 consecutive ow of output row oh
      const int o = ks * 4 + kq;
      const int ohr = o / no, ow0 = (o - ohr * no) * 8;
      const bool row_ok = ohr < OH;
      const int oh = row_ok ? ohr : OH - 1;
      float gc[2][8];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float t = gn[m][e];
          if (MASK) t = yn[m][e] > 0.f ? t : 0.f;                 // the layer's ReLU
          gc[m][e] = (row_ok && ow0 + e < OW) ? t : 0.f;          // the tail octet carries g = 0
        }
      if (ks + 4 < ksteps) request(ks + 4);
      uint4 ap[2][3];                               // [filter half][part] = 8 bf16 along k
#pragma unroll
      for (int m = 0; m < 2; ++m) {
        float gv[2][4];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          gv[e >> 2][e & 3] = gc[m][e];
          if (MASK) dbs[m] += gc[m][e];
        }
        uint2 h0, m0, l0, h1, m1, l1;
        g3_split4(gv[0], h0, m0, l0);
        g3_split4(gv[1], h1, m1, l1);
        ap[m][0] = make_uint4(h0.x, h0.y, h1.x, h1.y);
        ap[m][1] = make_uint4(m0.x, m0.y, m1.x, m1.y);
        ap[m][2] = make_uint4(l0.x, l0.y, l1.x, l1.y);
      }
      const uint16_t* pb = px + (oh * C1P_S) * W + ow0 * C1P_S + tap_off;
      // all four tap groups' halfwords first (32 LDS reads in flight), then the 24 MFMAs
      uint32_t raw[4][8];
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) raw[t][e] = pb[t * 2 * W + 4 * e];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const uint32_t* rw = raw[t];
        const g3_bf16x8 bv = c1p_as_bf8(make_uint4(rw[0] | (rw[1] << 16), rw[2] | (rw[3] << 16), rw[4] | (rw[5] << 16), rw[6] | (rw[7] << 16)));
#pragma unroll
        for (int p = 2; p >= 0; --p) {              // smallest part of g first
          acc0[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(c1p_as_bf8(ap[0][p]), bv, acc0[t], 0, 0, 0);
          acc1[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(c1p_as_bf8(ap[1][p]), bv, acc1[t], 0, 0, 0);
        }
      }
    }
  }
  // workgroup partial: waves add up in LDS in wave order.  Accumulator tile (half m, tap group t): row 4 kq + r <-> filter
  // 16 m + 4 kq + r, column j <-> tap t * 16 + j
  __syncthreads();
  float* red = reinterpret_cast<float*>(c1p_lds);
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i0 = (4 * kq + r) * C1P_TAPS + t * 16 + j, i1 = i0 + 16 * C1P_TAPS;
          red[i0] = (w ? red[i0] : 0.f) + acc0[t][r];
          red[i1] = (w ? red[i1] : 0.f) + acc1[t][r];
        }
      }
    }
    __syncthreads();
  }
  if (MASK) {
    // bias gradient: lane (j, kq) summed filters j and 16 + j over its octets; the four kq in a fixed butterfly, the four
    // waves in wave order behind the slab's 2048 weight-gradient sums
#pragma unroll
    for (int m = 0; m < 2; ++m) { dbs[m] += __shfl_xor(dbs[m], 16); dbs[m] += __shfl_xor(dbs[m], 32); }
    for (int w = 0; w < 4; ++w) {
      if (wave == w && kq == 0) {
        red[C1P_DW + j] = (w ? red[C1P_DW + j] : 0.f) + dbs[0];
        red[C1P_DW + 16 + j] = (w ? red[C1P_DW + 16 + j] : 0.f) + dbs[1];
      }
      __syncthreads();
    }
  }
  float* out = partial + (int64_t)blockIdx.x * C1P_SLAB;
  for (int k = tid; k < (MASK ? C1P_SLAB : C1P_DW); k += 256) out[k] = red[k];
}

// dw[f][0][kh][kw] (element strides so, sh, sw) = scale * sum of the slabs in a fixed order: a block owns 64 consecutive
// sums, its wave w adds the w-th quarter of the slabs in slab order on four interleaved chains, the four waves' sums are
// added in wave order.  The order depends on `parts` alone.
__global__ void __launch_bounds__(256)
k_conv1p_wrw_reduce(const float* __restrict__ partial, int parts, float scale, float* __restrict__ dw, int64_t so, int64_t sh,
                    int64_t sw, float* __restrict__ db) {
  __shared__ float red[4][64];
  const int c = threadIdx.x & 63, w = threadIdx.x >> 6, t = blockIdx.x * 64 + c;
  const int total = C1P_DW + (db ? C1P_F : 0);
  const int quarter = (parts + 3) >> 2, pend = (w + 1) * quarter < parts ? (w + 1) * quarter : parts;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (t < total) {
    int p = w * quarter;
    for (; p + 4 <= pend; p += 4) {
      s0 += partial[(int64_t)p * C1P_SLAB + t]; s1 += partial[(int64_t)(p + 1) * C1P_SLAB + t];
      s2 += partial[(int64_t)(p + 2) * C1P_SLAB + t]; s3 += partial[(int64_t)(p + 3) * C1P_SLAB + t];
    }
    for (; p < pend; ++p) s0 += partial[(int64_t)p * C1P_SLAB + t];
  }
  red[w][c] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (w != 0 || t >= total) return;
  const float s = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
  if (t >= C1P_DW) { db[t - C1P_DW] = s; return; }                     // the bias gradient takes no input scale
  const int f = t >> 6, tap = t & 63;
  dw[f * so + (tap >> 3) * sh + (tap & 7) * sw] = s * scale;
}

// checked arguments in; MASK: g is the gradient w.r.t. the layer's output, masked by y > 0 while it is loaded, db its column sums
template <bool MASK>
static int c1p_wrw(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* g, const float* y, float scale, float* scratch,
                   float* dw, int64_t ws_o, int64_t ws_h, int64_t ws_w, float* db, hipStream_t st) {
  const int OH = (H - C1P_K) / C1P_S + 1, OW = (W - C1P_K) / C1P_S + 1, HW = H * W, Pd = c1p_bf_pitch(HW, OW);
  size_t lds = (size_t)Pd * 2;
  if (lds < (size_t)C1P_SLAB * 4) lds = (size_t)C1P_SLAB * 4;       // the workgroup's partial is reduced there
  const unsigned grid = capped_grid(N, C1P_WGS);
  {
    ProfScope ps("k_conv1p_u8_wrw", (double)N * (HW + (MASK ? 2.0 : 1.0) * OH * OW * C1P_F * 4), st,
                 (double)N * OH * OW * 2.0 * C1P_TAPS * C1P_F);
    hipLaunchKernelGGL((k_conv1p_u8_wrw<MASK>), dim3(grid), dim3(256), lds, st, (int)N, H, W, OH, OW, Pd, x, g, scratch, y);
    MIRL_LAUNCH_CHECK();
  }
  const int total = C1P_DW + (MASK ? C1P_F : 0);
  ProfScope ps("k_conv1p_wrw_reduce", (double)grid * total * 4, st);
  hipLaunchKernelGGL(k_conv1p_wrw_reduce, dim3((total + 63) / 64), dim3(256), 0, st, scratch, (int)grid, scale, dw, ws_o, ws_h, ws_w, db);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

}  // namespace mirl

extern "C" int mirl_conv1p_u8_supported(int32_t H, int32_t W, int32_t F, int32_t K, int32_t S) {
  using namespace mirl;
  if (F != C1P_F || K != C1P_K || S != C1P_S) return 0;
  if (H < C1P_K || W < C1P_K || H > 4096 || W > 4096 || (W % 4) != 0 || ((H * W) % 16) != 0) return 0;
  // the LDS plan: the weight gradient stages one frame as bf16 (with its tail over-read) in the 64 KiB a kernel gets unasked;
  // the forward's raw bytes are half of that
  return (size_t)c1p_bf_pitch(H * W, (W - C1P_K) / C1P_S + 1) * 2 <= 64 * 1024 ? 1 : 0;
}

extern "C" int mirl_conv1p_u8_wpk_floats(int64_t* out) {
  if (!out) return mirl::fail(MIRL_ERR_ARG, "null out");
  *out = mirl::C1P_WPK;
  return MIRL_OK;
}

// flags: bit 3 = skip the weight packing (wpk was packed by an earlier call with the same weights and scale)
extern "C" int mirl_conv1p_u8_fwd(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* weight, int64_t ws_o,
                                  int64_t ws_h, int64_t ws_w, const float* bias, float scale, float* wpk, float* y,
                                  int32_t flags, void* stream) {
  using namespace mirl;
  if (N <= 0 || N >= (1LL << 30) || !x || !weight || !bias || !wpk || !y) return fail(MIRL_ERR_ARG, "bad conv1p_u8_fwd arguments");
  if (!mirl_conv1p_u8_supported(H, W, C1P_F, C1P_K, C1P_S)) return fail(MIRL_ERR_ARG, "conv1p_u8_fwd: unsupported frame shape");
  if (!aligned16(x, y, bias, wpk)) return fail(MIRL_ERR_ARG, "conv1p_u8_fwd: pointers must be 16-byte aligned");
  if (flags & ~8) return fail(MIRL_ERR_ARG, "conv1p_u8_fwd: unknown flag bits");
  hipStream_t st = (hipStream_t)stream;
  const int OH = (H - C1P_K) / C1P_S + 1, OW = (W - C1P_K) / C1P_S + 1, HW = H * W, OHW = OH * OW;
  const int tiles = (OHW + 15) / 16;
  // which scratch blocks this entry point packed (host side, one caller thread per the library's contract)
  static std::unordered_set<const void*> packed_here;
  if (flags & 8) {
    if (!packed_here.count((const void*)wpk))
      return fail(MIRL_ERR_STATE, "conv1p_u8_fwd: flags bit 3 (weights already packed) but this scratch block was not packed by this entry point");
  } else {
    packed_here.insert((const void*)wpk);
    ProfScope ps("k_conv1p_pack_w", C1P_TAPS * C1P_F * 4 + C1P_WPK * 4.0, st);
    hipLaunchKernelGGL(k_conv1p_pack_w, dim3(1), dim3(256), 0, st, weight, ws_o, ws_h, ws_w, scale, (uint4*)wpk);
    MIRL_LAUNCH_CHECK();
  }
  // frames per LDS fill: more only once every resident workgroup has a group of its own, and within 32 KiB
  int fpi_max = 32 * 1024 / HW;
  fpi_max = fpi_max < 1 ? 1 : (fpi_max > C1P_FPI ? C1P_FPI : fpi_max);
  int64_t fpi64 = N / C1P_FWD_WGS;
  const int fpi = fpi64 < 1 ? 1 : (fpi64 > fpi_max ? fpi_max : (int)fpi64);
  // few frames: `split` workgroups share one frame's tiles (at least one tile per wave)
  const int max_split = (tiles + 3) / 4;
  int split = N >= C1P_FWD_WGS ? 1 : (int)((C1P_FWD_WGS + N - 1) / N);
  if (split > max_split) split = max_split;
  const unsigned grid = capped_grid((N + fpi - 1) / fpi * split, C1P_FWD_WGS);
  const size_t lds = (size_t)fpi * HW;
  ProfScope ps("k_conv1p_u8_fwd", (double)N * (HW + (double)OHW * C1P_F * 4), st, (double)N * OHW * 2.0 * C1P_TAPS * C1P_F);
  hipLaunchKernelGGL(k_conv1p_u8_fwd, dim3(grid), dim3(256), lds, st, (int)N, W, OW, HW, OHW, tiles, magic_u32(OW), magic_u32(tiles),
                     fpi, split, x, (const uint4*)wpk, bias, y);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_conv1p_u8_wrw_scratch_floats(int64_t* out) {
  if (!out) return mirl::fail(MIRL_ERR_ARG, "null out");
  *out = (int64_t)mirl::C1P_WGS * mirl::C1P_SLAB;      // per-workgroup slabs: 2048 weight-gradient sums + 32 bias-gradient sums
  return MIRL_OK;
}

extern "C" int mirl_conv1p_u8_wrw(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* g, float scale, float* scratch,
                                  float* dw, int64_t ws_o, int64_t ws_h, int64_t ws_w, void* stream) {
  using namespace mirl;
  if (N <= 0 || N >= (1LL << 30) || !x || !g || !scratch || !dw) return fail(MIRL_ERR_ARG, "bad conv1p_u8_wrw arguments");
  if (!mirl_conv1p_u8_supported(H, W, C1P_F, C1P_K, C1P_S)) return fail(MIRL_ERR_ARG, "conv1p_u8_wrw: unsupported frame shape");
  if (!aligned16(x, g, scratch)) return fail(MIRL_ERR_ARG, "conv1p_u8_wrw: pointers must be 16-byte aligned");
  return c1p_wrw<false>(N, H, W, x, g, nullptr, scale, scratch, dw, ws_o, ws_h, ws_w, nullptr, (hipStream_t)stream);
}

extern "C" int mirl_conv1p_u8_wrw_masked(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* dy, const float* y,
                                         float scale, float* scratch, float* dw, int64_t ws_o, int64_t ws_h, int64_t ws_w,
                                         float* db, void* stream) {
  using namespace mirl;
  if (N <= 0 || N >= (1LL << 30) || !x || !dy || !y || !scratch || !dw || !db) return fail(MIRL_ERR_ARG, "bad conv1p_u8_wrw_masked arguments");
  if (!mirl_conv1p_u8_supported(H, W, C1P_F, C1P_K, C1P_S)) return fail(MIRL_ERR_ARG, "conv1p_u8_wrw: unsupported frame shape");
  if (!aligned16(x, dy, y, scratch)) return fail(MIRL_ERR_ARG, "conv1p_u8_wrw: pointers must be 16-byte aligned");
  return c1p_wrw<true>(N, H, W, x, dy, y, scale, scratch, dw, ws_o, ws_h, ws_w, db, (hipStream_t)stream);
}
