// conv_in_rows.hip — the input layer from ONE-plane and THREE-plane uint8 frames: the kernel family next to
// csrc/conv_in.hip (four planes), written once on the plane count P and instantiated for P = 1 and P = 3.
//
// Reference: rltime/configs/atari_iqn_lstm.json with env_wrappers/atari_lstm.json trains on unstacked frames
// ("stack": 1, observations (1, 84, 84) uint8): the LSTM carries the history, and one plane per step makes the replay
// and every frame transfer four times smaller.  rltime/configs/ple_flappy_bird_iqn_lstm.json trains the same network on
// one RGB frame per step ("warp_size" [80, 120, 3], "stack" 1: observations (3, 120, 80) uint8); the kernels do not care
// what the planes mean: a three-plane history stack takes them too.  The layer is cnn.py:44-49 as in conv_in.hip —
// `x.float() * scale`, `F.relu(conv(x))` — at Conv2d(P -> 32, kernel 8, stride 4).  conv_in.hip's kernels give one MFMA
// k-group to one PLANE; with one plane three quarters of every instruction would multiply zeros, with three a quarter, so
// this family turns the operand around: a k-group is one KERNEL ROW of one plane, and no instruction multiplies zeros.
//
// Forward (k_conv_rows_u8_fwd<P>), bf16 matrix pipe, f32 result.  A uint8 pixel is exact in bf16 and w * scale is split
// exactly into three bf16 parts (g3_split4), so every product is exact in the MFMA's f32 accumulator.
//   contraction   v_mfma_f32_16x16x32_bf16, filters as rows, 16 output positions as columns; the contraction K = P * 8 * 8
//                 is 2 P instructions of four (plane, kernel row) pairs each: instruction q < 2 P, k group lane >> 4 =
//                 plane q >> 1, kernel row kh = 4 (q & 1) + (lane >> 4); a lane's 8 k-elements = the 8 bytes
//                 x[plane][4 oh + kh][4 ow .. 4 ow + 7].  2 P x 2 filter halves x 3 parts MFMAs per 16-position tile:
//                 12 for one plane, 36 for three (the 4-plane kernel: 48).
//   operands      all weight operands of a lane stay in registers: no weight LDS.  The three parts run on separate
//                 accumulator chains (q ascending) and are added smallest first, then the bias: an output's summation
//                 order does not depend on N, the split or the frames per fill.
//     P = 1       12 operands = 48 VGPRs, 116 in all: within the 128 a wave has at FOUR waves per SIMD
//                 (__launch_bounds__(256, 4)), four workgroups per CU behind the store stream that bounds the kernel.
//     P = 3       36 operands = 144 VGPRs and TWO waves per SIMD (__launch_bounds__(256, 2)), not four with part of the
//                 weights in LDS as k_conv1_u8_fwd keeps its low parts.  Why: with weights in LDS every tile re-reads
//                 them — 24 operands x 1 KiB per wave and tile for the mid and low parts against 0.75 KiB of pixels — and
//                 four waves share one LDS port, so the operand reads alone (96 KiB per four tiles at 128 B / clock = 768
//                 clocks) would outlast the tiles' 36 MFMAs on their own SIMD; conv_in.hip pays that for a third of its
//                 operands only because 192 VGPRs of weights cannot be held at any occupancy that leaves room for the
//                 rest.  Here 144 + 24 accumulator + 24 pixel registers fit the 256 a wave has at two per SIMD, a tile
//                 touches LDS for its pixels alone, and the next tile's pixel words are requested before this tile's
//                 chain — which is what the second wave of a SIMD would otherwise be there to cover.  The LDS variant was
//                 not built and timed; the measurement behind the choice is this kernel's own: 1.19 ms per 41 472 frames
//                 of (3, 120, 80) = 3.5 TB/s of algorithmic bytes, bound by its output stores, against 8.1 ms for the
//                 conversion + library convolution it replaces (docs/measurement.md).
//   work split    persistent workgroups (4 waves); a work unit stages up to 4 consecutive frames (raw bytes: the planes
//                 of a frame, and consecutive frames, are one contiguous run of 16 B vectors) and walks their tiles, one
//                 per wave at a time; at small N `split` workgroups share one frame's tiles so that acting batches of
//                 16-32 frames fill the chip.
//   epilogue      + bias, ReLU, two 16 B stores per lane; a wave writes 2 KiB of contiguous NHWC rows.  Plain (cached)
//                 stores: measured 0.61 against 0.83 ms per 41 472 one-plane frames with non-temporal ones
//                 (docs/measurement.md).
//   HBM traffic   one plane: 7 KB in + 51 KB out per 84 x 84 frame; three: 29 KB in + 70 KB out per 120 x 80 frame.  Both
//                 are bound by their output stores.
//
// Weight gradient (k_conv_rows_u8_wrw<P, MASK>), bf16 pipe with the exact three-way split of g, as k_conv1_u8_wrw_b3:
// rows = 16 filters, columns = 16 taps, K = 32 positions walked in octets of 8 consecutive ow (the tail octet carries
// g = 0), the frame's planes staged once as bf16.  64 P taps = 4 P tap groups, x 2 filter halves: ALL 8 P accumulator tiles
// of the 32 x 64 P result stay in registers, the three parts enter smallest first.  For three planes that is 96 of the 256
// registers a wave has at two waves per SIMD, rather than walking the planes in three passes: g (and y in the masked form)
// is the larger HBM stream — 70 KB against 29 KB per 120 x 80 frame — and holding every tile reads and splits it once.
// Per-workgroup slabs are summed in slab order by k_conv_rows_wrw_reduce<P>: fixed partition, fixed order, no float
// atomics.  The masked form applies y > 0 while dy is loaded and carries the bias gradient behind the slab's 2048 P weight
// sums.
// Launch plans, size constants and the per-P launch parameters (CRows<P>): csrc/host_util.hpp; what the families share on
// the device and in the entry points: csrc/conv_u8.hpp.  Autograd wiring: rltime_amd/models/torch/fused.py:_ConvU8 through
// its one-plane and three-plane families.  The entry points keep their two prefixes, mirl_conv1p_u8_* (one plane, no
// channel stride) and mirl_conv1p3_u8_* (three), and the profiler its two sets of names.
#include "conv_u8.hpp"

namespace mirl {

// what an instance is called: by its entry points' messages, by the profiler, and in the table of packed weight blocks
template <int P> struct CRowsNames;
template <> struct CRowsNames<1> {
  static constexpr const char *fwd = "conv1p_u8_fwd", *wrw = "conv1p_u8_wrw", *wrw_masked = "conv1p_u8_wrw_masked";
  static constexpr const char *k_pack = "k_conv1p_pack_w", *k_fwd = "k_conv1p_u8_fwd", *k_wrw = "k_conv1p_u8_wrw",
                              *k_reduce = "k_conv1p_wrw_reduce";
  static constexpr int WPK_TAG = C1_WPK_1P;
};
template <> struct CRowsNames<3> {
  static constexpr const char *fwd = "conv1p3_u8_fwd", *wrw = "conv1p3_u8_wrw", *wrw_masked = "conv1p3_u8_wrw_masked";
  static constexpr const char *k_pack = "k_conv1p3_pack_w", *k_fwd = "k_conv1p3_u8_fwd", *k_wrw = "k_conv1p3_u8_wrw",
                              *k_reduce = "k_conv1p3_wrw_reduce";
  static constexpr int WPK_TAG = C1_WPK_3P;
};

// wpk3[((part*2P + q)*2 + m)*64 + lane] = 8 bf16 (kw = 0..7) of part `part` of w[f][c][kh][kw] * scale with the A-operand
// lane map row i = lane & 15 -> filter f = (i>>2)*8 + m*4 + (i&3) (the 4 accumulator rows a lane owns are 4 CONSECUTIVE
// filters, as k_conv1_pack_w), and instruction q's k group lane >> 4 -> plane c = q >> 1, kernel row kh = 4 (q & 1) +
// (lane >> 4).  One block per plane; one plane: sc = 0.
template <int P>
__global__ void __launch_bounds__(256)
k_conv_rows_pack_w(const float* __restrict__ w, int64_t so, int64_t sc, int64_t sh, int64_t sw, float scale, uint4* __restrict__ wpk3) {
  const int t = threadIdx.x, c = blockIdx.x;
  const int lane = t & 63, m = (t >> 6) & 1, hh = t >> 7;
  const int i = lane & 15, kh = 4 * hh + (lane >> 4);
  const int f = (i >> 2) * 8 + m * 4 + (i & 3);
  float v[2][4];
#pragma unroll
  for (int kw = 0; kw < C1_K; ++kw) v[kw >> 2][kw & 3] = w[f * so + c * sc + kh * sh + kw * sw] * scale;   // x*scale*w summed as x*(scale*w)
  uint2 h0, m0, l0, h1, m1, l1;
  g3_split4(v[0], h0, m0, l0);
  g3_split4(v[1], h1, m1, l1);
  const int o = ((2 * c + hh) * 2 + m) * 64 + lane;
  wpk3[o] = make_uint4(h0.x, h0.y, h1.x, h1.y);
  wpk3[4 * P * 64 + o] = make_uint4(m0.x, m0.y, m1.x, m1.y);
  wpk3[8 * P * 64 + o] = make_uint4(l0.x, l0.y, l1.x, l1.y);
}

// x: uint8 [N][P][H][W]; y: float [N][OH][OW][32].  Work unit u = (frame group, part): a group is `fpi` consecutive
// frames, `split` parts share a group's tiles (split > 1 only with fpi = 1).  HWP = P H W, the bytes of a frame.
template <int P>
__global__ void __launch_bounds__(256, CRows<P>::WAVES)
k_conv_rows_u8_fwd(int N, int W, int OW, int HW, int OHW, int tiles, unsigned ow_magic, unsigned tiles_magic, int fpi, int split,
                   const uint8_t* __restrict__ x, const uint4* __restrict__ wpk3, const float* __restrict__ bias,
                   float* __restrict__ y) {
  constexpr int LD = CRows<P>::LD;                  // staging loads in flight per lane
  extern __shared__ __align__(16) uint8_t crows_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, kq = lane >> 4;
  g3_bf16x8 wt[3][2 * P][2];                        // [part][instruction q][filter half]
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int q = 0; q < 2 * P; ++q)
#pragma unroll
      for (int m = 0; m < 2; ++m) wt[p][q][m] = c1_as_bf8(wpk3[((p * 2 * P + q) * 2 + m) * 64 + lane]);
  const g3_f32x4 b0 = *reinterpret_cast<const g3_f32x4*>(bias + kq * 8), b1 = *reinterpret_cast<const g3_f32x4*>(bias + kq * 8 + 4);
  const int HWP = P * HW, hw16 = HWP >> 4, row_off = kq * W;
  const int groups = (N + fpi - 1) / fpi, units = groups * split, step = 4 * split;
  bool first = true;
  for (int u = blockIdx.x; u < units; u += gridDim.x) {
    const int group = split == 1 ? u : u / split, part = u - group * split;
    const int n0 = group * fpi;
    const int frames = N - n0 < fpi ? N - n0 : fpi;
    if (!first) __syncthreads();                    // every wave is done reading the previous frames
    first = false;
    {
      // `frames` frames of P planes are one contiguous run of 16 B vectors, in HBM and in LDS
      const int vecs = frames * hw16;
      const uint4* s4 = reinterpret_cast<const uint4*>(x + (int64_t)n0 * HWP);
      uint4* d4 = reinterpret_cast<uint4*>(crows_lds);
      for (int o0 = tid; o0 < vecs; o0 += 256 * LD) {
        uint4 v[LD];
#pragma unroll
        for (int k = 0; k < LD; ++k) { const int o = o0 + k * 256; v[k] = s4[o < vecs ? o : vecs - 1]; }
#pragma unroll
        for (int k = 0; k < LD; ++k) { const int o = o0 + k * 256; if (o < vecs) d4[o] = v[k]; }
      }
    }
    __syncthreads();
    const int tend = frames * tiles;
    int tt = part * 4 + wave;                       // this wave's tiles: tt, + step, ... < frames * tiles
    if (tt >= tend) continue;
    // tile -> (frame f, position p); the lane's pixel rows: per plane kh = kq and kq + 4, 8 bytes each
    int f, p;
    uint32_t px[4 * P];
#define CROWS_TILE_READ(tt_, f_, p_, px_)                                                       \
    {                                                                                           \
      f_ = tiles == 1 ? tt_ : (int)__umulhi((unsigned)(tt_), tiles_magic);                      \
      p_ = (tt_ - f_ * tiles) * 16 + j;                                                         \
      const int pc_ = p_ < OHW ? p_ : OHW - 1;                                                  \
      const int oh_ = OW == 1 ? pc_ : (int)__umulhi((unsigned)pc_, ow_magic);                   \
      const uint8_t* base_ = crows_lds + f_ * HWP + (oh_ * C1_S) * W + (pc_ - oh_ * OW) * C1_S + row_off; \
      _Pragma("unroll")                                                                         \
      for (int c_ = 0; c_ < P; ++c_) {                                                          \
        const uint8_t* b_ = base_ + c_ * HW;                                                    \
        px_[4 * c_ + 0] = *reinterpret_cast<const uint32_t*>(b_);                               \
        px_[4 * c_ + 1] = *reinterpret_cast<const uint32_t*>(b_ + 4);                           \
        px_[4 * c_ + 2] = *reinterpret_cast<const uint32_t*>(b_ + 4 * W);                       \
        px_[4 * c_ + 3] = *reinterpret_cast<const uint32_t*>(b_ + 4 * W + 4);                   \
      }                                                                                         \
    }
    CROWS_TILE_READ(tt, f, p, px);
    for (;;) {
      const int tn = tt + step;
      int fn = 0, pn = 0;
      uint32_t pxn[4 * P] = {};                     // an aggregate initialiser: zeroing in a loop costs 2 VGPRs
      if (tn < tend) CROWS_TILE_READ(tn, fn, pn, pxn);   // the next tile's LDS words in flight before this tile's chain
      const g3_f32x4 z = {0.f, 0.f, 0.f, 0.f};
      g3_f32x4 l0 = z, l1 = z, m0 = z, m1 = z, h0 = z, h1 = z;
#pragma unroll
      for (int q = 0; q < 2 * P; ++q) {             // q = 2 plane + kernel-row half: the lane's dwords 2 q, 2 q + 1
        const g3_bf16x8 bq = c1_row_bf(px[2 * q], px[2 * q + 1]);
        l0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[2][q][0], bq, l0, 0, 0, 0);
        l1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[2][q][1], bq, l1, 0, 0, 0);
        m0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[1][q][0], bq, m0, 0, 0, 0);
        m1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[1][q][1], bq, m1, 0, 0, 0);
        h0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[0][q][0], bq, h0, 0, 0, 0);
        h1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[0][q][1], bq, h1, 0, 0, 0);
      }
      if (p < OHW) {
        const g3_f32x4 o0 = c1_relu(((l0 + m0) + h0) + b0), o1 = c1_relu(((l1 + m1) + h1) + b1);
        g3_f32x4* dst = reinterpret_cast<g3_f32x4*>(y + ((n0 + f) * (int64_t)OHW + p) * C1_F + kq * 8);
        dst[0] = o0; dst[1] = o1;
      }
      if (tn >= tend) break;
      tt = tn; f = fn; p = pn;
#pragma unroll
      for (int k = 0; k < 4 * P; ++k) px[k] = pxn[k];
    }
#undef CROWS_TILE_READ
  }
}

// dW[f][c][kh][kw] = scale * sum over (n, oh, ow) of g[n][oh][ow][f] * float(x[n][c][4 oh + kh][4 ow + kw]).  Lane (j, kq) of a
// K-step owns octet 4 ks + kq: its 8 A values are g[oh][ow0 .. ow0 + 7][filter j + 16 m], its 8 B values for tap
// (c, kh, kw) the pixels x[c][4 oh + kh][4 (ow0 + e) + kw], e < 8.  Tap group tg = 4 c + t, t < 4: kh = 2 t + (j >> 3),
// kw = j & 7, so that tg * 16 + j IS the flattened (c, kh, kw) index.  Plane c is staged at halfword c * Pd, its slack
// behind HW zeroed once.  Frame n goes to workgroup n % gridDim.x.
template <int P, bool MASK>
__global__ void __launch_bounds__(256, 2)
k_conv_rows_u8_wrw(int N, int H, int W, int OH, int OW, int Pd, const uint8_t* __restrict__ x, const float* __restrict__ g,
                   float* __restrict__ partial, const float* __restrict__ yv) {
  constexpr int TG = CRows<P>::TG;
  extern __shared__ __align__(16) uint8_t crows_lds[];
  uint16_t* px = reinterpret_cast<uint16_t*>(crows_lds);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, kq = lane >> 4;
  const int HW = H * W, OHW = OH * OW, hw16 = HW >> 4;
  const int no = (OW + 7) >> 3, octets = OH * no, ksteps = (octets + 3) >> 2;
  const int tap_off = (j >> 3) * W + (j & 7);
  float dbs[2] = {0.f, 0.f};
  C1WrwG<MASK> gs;
  g3_f32x4 acc0[TG], acc1[TG];
#pragma unroll
  for (int t = 0; t < TG; ++t) { acc0[t] = g3_f32x4{0.f, 0.f, 0.f, 0.f}; acc1[t] = g3_f32x4{0.f, 0.f, 0.f, 0.f}; }
  // the slack behind each plane is read (tail octets) but never staged: zero it once — any finite value would do, times g = 0
  for (int c = 0; c < P; ++c)
    for (int i = HW + tid; i < Pd; i += 256) px[c * Pd + i] = 0;
  bool first = true;
  for (int n = blockIdx.x; n < N; n += gridDim.x) {
    if (!first) __syncthreads();                  // every wave is done reading the previous frame
    first = false;
#pragma unroll 1
    for (int c = 0; c < P; ++c) {
      // 16 pixels -> 16 bf16 = two 16 B LDS stores
      const uint4* s4 = reinterpret_cast<const uint4*>(x + ((int64_t)n * P + c) * HW);
      uint16_t* pc = px + c * Pd;
      for (int o0 = tid; o0 < hw16; o0 += 256 * 2) {
        uint4 v[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) { const int o = o0 + k * 256; v[k] = s4[o < hw16 ? o : hw16 - 1]; }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int o = o0 + k * 256;
          if (o < hw16) c1_stage16_bf(v[k], pc + o * 16);
        }
      }
    }
    __syncthreads();
    const float* gf = g + (int64_t)n * OHW * C1_F + j;
    const float* yf = MASK ? yv + (gf - g) : nullptr;
    if (wave < ksteps) gs.request(gf, yf, wave, kq, no, OH, OW);
    for (int ks = wave; ks < ksteps; ks += 4) {
      int oh, ow0;                                  // this lane's octet: 8 consecutive ow of output row oh
      uint4 ap[2][3];                               // [filter half][part] = 8 bf16 along k
      gs.take(ks, kq, no, OH, OW, oh, ow0);
      if (ks + 4 < ksteps) gs.request(gf, yf, ks + 4, kq, no, OH, OW);
      gs.split(ap, dbs);
      const uint16_t* pb = px + (oh * C1_S) * W + ow0 * C1_S + tap_off;
#pragma unroll
      for (int c = 0; c < P; ++c) {
        // a plane's four tap groups' halfwords first (32 LDS reads in flight), then its 24 MFMAs
        uint32_t raw[4][8];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int e = 0; e < 8; ++e) raw[t][e] = pb[c * Pd + t * 2 * W + 4 * e];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const uint32_t* rw = raw[t];
          const g3_bf16x8 bv = c1_as_bf8(make_uint4(rw[0] | (rw[1] << 16), rw[2] | (rw[3] << 16), rw[4] | (rw[5] << 16), rw[6] | (rw[7] << 16)));
#pragma unroll
          for (int p = 2; p >= 0; --p) {            // smallest part of g first
            acc0[4 * c + t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(c1_as_bf8(ap[0][p]), bv, acc0[4 * c + t], 0, 0, 0);
            acc1[4 * c + t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(c1_as_bf8(ap[1][p]), bv, acc1[4 * c + t], 0, 0, 0);
          }
        }
      }
    }
  }
  c1_wrw_epilogue<TG, MASK>(reinterpret_cast<float*>(crows_lds), acc0, acc1, dbs, partial + (int64_t)blockIdx.x * CRows<P>::SLAB, tid, wave, j, kq);
}

// dw[f][c][kh][kw] (element strides so, sc, sh, sw; one plane: sc = 0) = scale * sum of the slabs in a fixed order: a block
// owns 64 consecutive sums, its wave w adds the w-th quarter of the slabs in slab order on four interleaved chains, the
// four waves' sums are added in wave order.  The order depends on `parts` alone.
template <int P>
__global__ void __launch_bounds__(256)
k_conv_rows_wrw_reduce(const float* __restrict__ partial, int parts, float scale, float* __restrict__ dw, int64_t so, int64_t sc,
                       int64_t sh, int64_t sw, float* __restrict__ db) {
  constexpr int DW = CRows<P>::DW, SLAB = CRows<P>::SLAB;
  __shared__ float red[4][64];
  const int c = threadIdx.x & 63, w = threadIdx.x >> 6, t = blockIdx.x * 64 + c;
  const int total = DW + (db ? C1_F : 0);
  const int quarter = (parts + 3) >> 2, pend = (w + 1) * quarter < parts ? (w + 1) * quarter : parts;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (t < total) {
    int p = w * quarter;
    for (; p + 4 <= pend; p += 4) {
      s0 += partial[(int64_t)p * SLAB + t]; s1 += partial[(int64_t)(p + 1) * SLAB + t];
      s2 += partial[(int64_t)(p + 2) * SLAB + t]; s3 += partial[(int64_t)(p + 3) * SLAB + t];
    }
    for (; p < pend; ++p) s0 += partial[(int64_t)p * SLAB + t];
  }
  red[w][c] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (w != 0 || t >= total) return;
  const float s = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
  if (t >= DW) { db[t - DW] = s; return; }                             // the bias gradient takes no input scale
  const int f = t / (P * C1_TAPS), tap = t - f * (P * C1_TAPS);
  dw[f * so + (tap >> 6) * sc + ((tap >> 3) & 7) * sh + (tap & 7) * sw] = s * scale;
}

static int c1_query(int64_t* out, int64_t value) {
  if (!out) return fail(MIRL_ERR_ARG, "null out");
  *out = value;
  return MIRL_OK;
}

template <int P>
static int crows_supported(int32_t H, int32_t W, int32_t F, int32_t K, int32_t S) {
  return F == C1_F && K == C1_K && S == C1_S && CRows<P>::shape_ok(H, W) ? 1 : 0;
}

// flags: bit 3 = skip the weight packing (wpk was packed by an earlier call with the same weights and scale)
template <int P>
static int crows_fwd(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* weight, int64_t ws_o, int64_t ws_c, int64_t ws_h,
                     int64_t ws_w, const float* bias, float scale, float* wpk, float* y, int32_t flags, void* stream) {
  using T = CRows<P>;
  using Nm = CRowsNames<P>;
  if (int rc = c1_check_args(Nm::fwd, N, x && weight && bias && wpk && y, T::shape_ok(H, W), aligned16(x, y, bias, wpk))) return rc;
  if (flags & ~8) return fail(MIRL_ERR_ARG, std::string(Nm::fwd) + ": unknown flag bits");
  hipStream_t st = (hipStream_t)stream;
  const int OW = c1_out(W), HW = H * W, OHW = c1_out(H) * OW, tiles = (OHW + 15) / 16;
  if (!c1_wpk_holds(wpk, Nm::WPK_TAG, flags & 8))
    return fail(MIRL_ERR_STATE, std::string(Nm::fwd) + ": flags bit 3 (weights already packed) but this scratch block was not packed by this entry point");
  if (!(flags & 8)) {
    ProfScope ps(Nm::k_pack, P * C1_TAPS * C1_F * 4 + T::WPK * 4.0, st);
    hipLaunchKernelGGL(k_conv_rows_pack_w<P>, dim3(P), dim3(256), 0, st, weight, ws_o, ws_c, ws_h, ws_w, scale, (uint4*)wpk);
    MIRL_LAUNCH_CHECK();
  }
  const C1FwdPlan pl = T::fwd_plan(N, H, W);
  ProfScope ps(Nm::k_fwd, (double)N * (P * HW + (double)OHW * C1_F * 4), st, (double)N * OHW * 2.0 * P * C1_TAPS * C1_F);
  hipLaunchKernelGGL(k_conv_rows_u8_fwd<P>, dim3(pl.grid), dim3(256), pl.lds, st, (int)N, W, OW, HW, OHW, tiles, magic_u32(OW), magic_u32(tiles),
                     pl.fpi, pl.split, x, (const uint4*)wpk, bias, y);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

// MASK: g is the gradient w.r.t. the layer's output, masked by y > 0 while it is loaded, db its column sums.  The masked
// form reports shape and alignment under the unmasked name.
template <int P, bool MASK>
static int crows_wrw(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* g, const float* y, float scale, float* scratch,
                     float* dw, int64_t ws_o, int64_t ws_c, int64_t ws_h, int64_t ws_w, float* db, void* stream) {
  using T = CRows<P>;
  using Nm = CRowsNames<P>;
  if (int rc = c1_check_args(MASK ? Nm::wrw_masked : Nm::wrw, N, x && g && scratch && dw && (!MASK || (y && db)), T::shape_ok(H, W),
                             aligned16(x, g, y, scratch), Nm::wrw))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  const int OH = c1_out(H), OW = c1_out(W), HW = H * W;
  const C1WrwPlan pl = T::wrw_plan(N, H, W);
  {
    ProfScope ps(Nm::k_wrw, (double)N * (P * HW + (MASK ? 2.0 : 1.0) * OH * OW * C1_F * 4), st, (double)N * OH * OW * 2.0 * P * C1_TAPS * C1_F);
    hipLaunchKernelGGL((k_conv_rows_u8_wrw<P, MASK>), dim3(pl.grid), dim3(256), pl.lds, st, (int)N, H, W, OH, OW, pl.pitch, x, g, scratch, y);
    MIRL_LAUNCH_CHECK();
  }
  const int total = T::DW + (MASK ? C1_F : 0);
  ProfScope ps(Nm::k_reduce, (double)pl.grid * total * 4, st);
  hipLaunchKernelGGL(k_conv_rows_wrw_reduce<P>, dim3((total + 63) / 64), dim3(256), 0, st, scratch, (int)pl.grid, scale, dw, ws_o, ws_c, ws_h,
                     ws_w, db);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

}  // namespace mirl

using namespace mirl;

extern "C" int mirl_conv1p_u8_supported(int32_t H, int32_t W, int32_t F, int32_t K, int32_t S) { return crows_supported<1>(H, W, F, K, S); }
extern "C" int mirl_conv1p3_u8_supported(int32_t H, int32_t W, int32_t F, int32_t K, int32_t S) { return crows_supported<3>(H, W, F, K, S); }

extern "C" int mirl_conv1p_u8_wpk_floats(int64_t* out) { return c1_query(out, CRows<1>::WPK); }
extern "C" int mirl_conv1p3_u8_wpk_floats(int64_t* out) { return c1_query(out, CRows<3>::WPK); }

// per-workgroup slabs: 2048 P weight-gradient sums + 32 bias-gradient sums
extern "C" int mirl_conv1p_u8_wrw_scratch_floats(int64_t* out) { return c1_query(out, CRows<1>::SCRATCH_FLOATS); }
extern "C" int mirl_conv1p3_u8_wrw_scratch_floats(int64_t* out) { return c1_query(out, CRows<3>::SCRATCH_FLOATS); }

extern "C" int mirl_conv1p_u8_fwd(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* weight, int64_t ws_o,
                                  int64_t ws_h, int64_t ws_w, const float* bias, float scale, float* wpk, float* y,
                                  int32_t flags, void* stream) {
  return crows_fwd<1>(N, H, W, x, weight, ws_o, 0, ws_h, ws_w, bias, scale, wpk, y, flags, stream);
}
extern "C" int mirl_conv1p3_u8_fwd(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* weight, int64_t ws_o,
                                   int64_t ws_c, int64_t ws_h, int64_t ws_w, const float* bias, float scale, float* wpk, float* y,
                                   int32_t flags, void* stream) {
  return crows_fwd<3>(N, H, W, x, weight, ws_o, ws_c, ws_h, ws_w, bias, scale, wpk, y, flags, stream);
}

extern "C" int mirl_conv1p_u8_wrw(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* g, float scale, float* scratch,
                                  float* dw, int64_t ws_o, int64_t ws_h, int64_t ws_w, void* stream) {
  return crows_wrw<1, false>(N, H, W, x, g, nullptr, scale, scratch, dw, ws_o, 0, ws_h, ws_w, nullptr, stream);
}
extern "C" int mirl_conv1p3_u8_wrw(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* g, float scale, float* scratch,
                                   float* dw, int64_t ws_o, int64_t ws_c, int64_t ws_h, int64_t ws_w, void* stream) {
  return crows_wrw<3, false>(N, H, W, x, g, nullptr, scale, scratch, dw, ws_o, ws_c, ws_h, ws_w, nullptr, stream);
}

extern "C" int mirl_conv1p_u8_wrw_masked(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* dy, const float* y,
                                         float scale, float* scratch, float* dw, int64_t ws_o, int64_t ws_h, int64_t ws_w,
                                         float* db, void* stream) {
  return crows_wrw<1, true>(N, H, W, x, dy, y, scale, scratch, dw, ws_o, 0, ws_h, ws_w, db, stream);
}
extern "C" int mirl_conv1p3_u8_wrw_masked(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* dy, const float* y,
                                          float scale, float* scratch, float* dw, int64_t ws_o, int64_t ws_c, int64_t ws_h,
                                          int64_t ws_w, float* db, void* stream) {
  return crows_wrw<3, true>(N, H, W, x, dy, y, scale, scratch, dw, ws_o, ws_c, ws_h, ws_w, db, stream);
}
