// conv_in_f16.hip — the input layer of the SMALL nature CNN from uint8 frames: Conv2d(P -> 16, kernel 8, stride 4), written
// once on the plane count P and instantiated for P = 1, 3 and 4.
//
// Reference: rltime/configs/models/modules/nature_cnn_small.json (16 k8 s4 -> 32 k4 s2, the 2013 DQN network) next to
// nature_cnn.json, whose 32-filter first layer csrc/conv_in.hip (four planes) and csrc/conv_in_rows.hip (one and three)
// serve.  The layer is cnn.py:44-49 as there: `x.float() * scale`, `F.relu(conv(x))`.  16 filters are exactly ONE row tile
// of v_mfma_f32_16x16x32_bf16, so the two filter halves that shape both 32-filter families are gone: one weight operand
// per (part, instruction), one accumulator per part, and a lane's four accumulator rows are the four consecutive filters
// 4 (lane >> 4) .. + 3 of ONE position: one 16-byte store.  All three plane counts take the rows operand layout of
// conv_in_rows.hip — an MFMA k-group is one (plane, kernel row) pair, K = 64 P is 2 P instructions, none multiplies zeros;
// with the weights of 16 filters in 24 P registers the four-plane case has no reason for conv_in.hip's plane-per-k-group
// layout and its weight LDS.
//
// Forward (k_c16_u8_fwd<P>), bf16 matrix pipe, f32 result.  A uint8 pixel is exact in bf16 and w * scale is split exactly
// into three bf16 parts (g3_split4), so every product is exact in the MFMA's f32 accumulator.
//   contraction   filters as rows (row i = filter i), 16 output positions as columns; instruction q < 2 P: k group
//                 lane >> 4 = plane q >> 1, kernel row kh = 4 (q & 1) + (lane >> 4); a lane's 8 k-elements = the 8 bytes
//                 x[plane][4 oh + kh][4 ow .. 4 ow + 7].  2 P x 3 parts MFMAs per 16-position tile: 6, 18, 24.
//   operands      all 6 P weight operands of a lane stay in registers (24 P VGPRs), no weight LDS.  The three parts run on
//                 separate accumulator chains (q ascending) and are added smallest first, then the bias, then the ReLU:
//                 an output's summation order depends on the shape alone, not on N, the split or the frames per fill.
//   occupancy     the kernel is bound by HBM: per 84 x 84 frame it reads 7 P KB and writes 25.6 KB, half the 32-filter
//                 kernels' output stream, so the staging loads are now 22 % (P = 1) to 52 % (P = 4) of the traffic and a
//                 workgroup spends a comparable time waiting for its fill as writing its tiles.  Nothing inside a
//                 workgroup overlaps the two (one LDS buffer, a barrier after the fill), so what covers a fill is the
//                 OTHER workgroups of the CU: each P takes the most waves per SIMD its registers allow.
//     P = 1       24 weight + 12 accumulator + 8 pixel VGPRs, 62 in all: FOUR waves per SIMD (__launch_bounds__(256, 4)),
//                 not the eight the registers allow — four fills of 28 KiB (four 84 x 84 frames) are 112 of the CU's
//                 160 KiB of LDS.
//     P = 3       72 + 12 + 24 VGPRs, 126 in all: within the 128 of FOUR per SIMD, where conv_in_rows.hip's 144 weight
//                 registers allowed two; four 120 x 80 x 3 frames are 113 KiB of LDS.
//     P = 4       96 + 12 + 32 VGPRs, 158 in all: within the 168 of THREE per SIMD.
//                 The next tile's pixel words are requested before this tile's chain, as in conv_in_rows.hip.
//                 These are register- and LDS-budget choices; lower occupancies were not built and timed against them.
//   work split    persistent workgroups (4 waves); a work unit stages up to 4 consecutive frames within 32 KiB (raw bytes:
//                 planes and consecutive frames are one contiguous run of 16 B vectors) and walks their tiles, one per
//                 wave at a time; at small N `split` workgroups share one frame's tiles so that acting batches of 16-32
//                 frames fill the chip.
//   epilogue      + bias, ReLU, ONE 16 B store per lane; a wave writes 1 KiB of contiguous NHWC rows, plain (cached)
//                 stores as conv_in_rows.hip measured them.
//
// Weight gradient (k_c16_u8_wrw<P, MASK>), bf16 pipe with the exact three-way split of g, after k_conv_rows_u8_wrw: rows =
// the 16 filters, columns = 16 taps, K = 32 positions walked in octets of 8 consecutive ow (the tail octet carries g = 0).
// ALL 4 P accumulator tiles of the 16 x 64 P result stay in registers (64 VGPRs at P = 4), so g (and y in the masked form)
// is read and split once; the three parts enter smallest first.  With one filter half a K-step has half the MFMAs of the
// 32-filter kernel per pixel operand, so building that operand from 8 two-byte LDS reads (the pixels of one tap over 8
// consecutive ow are 4 pixels apart) would bound the kernel.  The frame's planes are therefore staged once as bf16 in
// FOUR sub-planes by column residue: pixel index i of a plane -> sub-plane i & 3, halfword i >> 2 (W % 4 == 0, so i & 3 is
// the column residue and i >> 2 = row * W / 4 + column / 4).  Tap (kh, kw) over positions (oh, ow0 .. ow0 + 7) is then 8
// CONSECUTIVE halfwords of sub-plane kw & 3 from (4 oh + kh) W / 4 + ow0 + (kw >> 2): five dwords from the dword below and
// four v_alignbit by the start's parity instead of eight reads and four packs.
// Per-workgroup slabs are summed in slab order by k_c16_wrw_reduce<P>: fixed partition, fixed order, no float atomics, a
// rerun repeats to the bit.  The masked form applies y > 0 while dy is loaded and carries the bias gradient behind the
// slab's 1024 P weight sums.
// Launch plans, size constants and the per-P launch parameters (CF16<P>): csrc/host_util.hpp; the byte -> bf16 helpers,
// argument checks and packed-block table shared with the 32-filter families: csrc/conv_u8.hpp.  Autograd wiring:
// rltime_amd/models/torch/fused.py:_ConvU8 through conv_u8_family(planes, 16).  Entry points: mirl_conv1f16p_u8_* (one
// plane, no channel stride), mirl_conv1f16p3_u8_* and mirl_conv1f16p4_u8_*, argument lists as the rows family's.
#include "conv_u8.hpp"

namespace mirl {

// what an instance is called: by its entry points' messages, by the profiler, and in the table of packed weight blocks
template <int P> struct CF16Names;
template <> struct CF16Names<1> {
  static constexpr const char *fwd = "conv1f16p_u8_fwd", *wrw = "conv1f16p_u8_wrw", *wrw_masked = "conv1f16p_u8_wrw_masked";
  static constexpr const char *k_pack = "k_conv1f16p_pack_w", *k_fwd = "k_conv1f16p_u8_fwd", *k_wrw = "k_conv1f16p_u8_wrw",
                              *k_reduce = "k_conv1f16p_wrw_reduce";
};
template <> struct CF16Names<3> {
  static constexpr const char *fwd = "conv1f16p3_u8_fwd", *wrw = "conv1f16p3_u8_wrw", *wrw_masked = "conv1f16p3_u8_wrw_masked";
  static constexpr const char *k_pack = "k_conv1f16p3_pack_w", *k_fwd = "k_conv1f16p3_u8_fwd", *k_wrw = "k_conv1f16p3_u8_wrw",
                              *k_reduce = "k_conv1f16p3_wrw_reduce";
};
template <> struct CF16Names<4> {
  static constexpr const char *fwd = "conv1f16p4_u8_fwd", *wrw = "conv1f16p4_u8_wrw", *wrw_masked = "conv1f16p4_u8_wrw_masked";
  static constexpr const char *k_pack = "k_conv1f16p4_pack_w", *k_fwd = "k_conv1f16p4_u8_fwd", *k_wrw = "k_conv1f16p4_u8_wrw",
                              *k_reduce = "k_conv1f16p4_wrw_reduce";
};
// the packed-block tags of this file, behind conv_u8.hpp's C1_WPK_*
template <int P> constexpr int C16_WPK_TAG = 16 + P;

// wpk3[(part*2P + q)*64 + lane] = 8 bf16 (kw = 0..7) of part `part` of w[f][c][kh][kw] * scale in A-operand lane order: row
// lane & 15 = filter f, instruction q's k group lane >> 4 -> plane c = q >> 1, kernel row kh = 4 (q & 1) + (lane >> 4).
// One block of 128 threads per plane; one plane: sc = 0.
template <int P>
__global__ void __launch_bounds__(128)
k_c16_pack_w(const float* __restrict__ w, int64_t so, int64_t sc, int64_t sh, int64_t sw, float scale, uint4* __restrict__ wpk3) {
  const int t = threadIdx.x, c = blockIdx.x;
  const int lane = t & 63, hh = t >> 6;
  const int f = lane & 15, kh = 4 * hh + (lane >> 4);
  float v[2][4];
#pragma unroll
  for (int kw = 0; kw < C1_K; ++kw) v[kw >> 2][kw & 3] = w[f * so + c * sc + kh * sh + kw * sw] * scale;   // x*scale*w summed as x*(scale*w)
  uint2 h0, m0, l0, h1, m1, l1;
  g3_split4(v[0], h0, m0, l0);
  g3_split4(v[1], h1, m1, l1);
  const int o = (2 * c + hh) * 64 + lane;
  wpk3[o] = make_uint4(h0.x, h0.y, h1.x, h1.y);
  wpk3[2 * P * 64 + o] = make_uint4(m0.x, m0.y, m1.x, m1.y);
  wpk3[4 * P * 64 + o] = make_uint4(l0.x, l0.y, l1.x, l1.y);
}

// x: uint8 [N][P][H][W]; y: float [N][OH][OW][16].  Work unit u = (frame group, part): a group is `fpi` consecutive frames,
// `split` parts share a group's tiles (split > 1 only with fpi = 1).  HWP = P H W, the bytes of a frame.
template <int P>
__global__ void __launch_bounds__(256, CF16<P>::WAVES)
k_c16_u8_fwd(int N, int W, int OW, int HW, int OHW, int tiles, unsigned ow_magic, unsigned tiles_magic, int fpi, int split,
             const uint8_t* __restrict__ x, const uint4* __restrict__ wpk3, const float* __restrict__ bias, float* __restrict__ y) {
  constexpr int LD = CF16<P>::LD;                   // staging loads in flight per lane
  extern __shared__ __align__(16) uint8_t c16_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, kq = lane >> 4;
  g3_bf16x8 wt[3][2 * P];                           // [part][instruction q]
#pragma unroll
  for (int p = 0; p < 3; ++p)
#pragma unroll
    for (int q = 0; q < 2 * P; ++q) wt[p][q] = c1_as_bf8(wpk3[(p * 2 * P + q) * 64 + lane]);
  const g3_f32x4 b4 = *reinterpret_cast<const g3_f32x4*>(bias + kq * 4);    // the lane's rows: filters 4 kq .. 4 kq + 3
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
      uint4* d4 = reinterpret_cast<uint4*>(c16_lds);
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
#define C16_TILE_READ(tt_, f_, p_, px_)                                                         \
    {                                                                                           \
      f_ = tiles == 1 ? tt_ : (int)__umulhi((unsigned)(tt_), tiles_magic);                      \
      p_ = (tt_ - f_ * tiles) * 16 + j;                                                         \
      const int pc_ = p_ < OHW ? p_ : OHW - 1;                                                  \
      const int oh_ = OW == 1 ? pc_ : (int)__umulhi((unsigned)pc_, ow_magic);                   \
      const uint8_t* base_ = c16_lds + f_ * HWP + (oh_ * C1_S) * W + (pc_ - oh_ * OW) * C1_S + row_off; \
      _Pragma("unroll")                                                                         \
      for (int c_ = 0; c_ < P; ++c_) {                                                          \
        const uint8_t* b_ = base_ + c_ * HW;                                                    \
        px_[4 * c_ + 0] = *reinterpret_cast<const uint32_t*>(b_);                               \
        px_[4 * c_ + 1] = *reinterpret_cast<const uint32_t*>(b_ + 4);                           \
        px_[4 * c_ + 2] = *reinterpret_cast<const uint32_t*>(b_ + 4 * W);                       \
        px_[4 * c_ + 3] = *reinterpret_cast<const uint32_t*>(b_ + 4 * W + 4);                   \
      }                                                                                         \
    }
    C16_TILE_READ(tt, f, p, px);
    for (;;) {
      const int tn = tt + step;
      int fn = 0, pn = 0;
      uint32_t pxn[4 * P] = {};
      if (tn < tend) C16_TILE_READ(tn, fn, pn, pxn);   // the next tile's LDS words in flight before this tile's chain
      const g3_f32x4 z = {0.f, 0.f, 0.f, 0.f};
      g3_f32x4 lo = z, mi = z, hi = z;
#pragma unroll
      for (int q = 0; q < 2 * P; ++q) {             // q = 2 plane + kernel-row half: the lane's dwords 2 q, 2 q + 1
        const g3_bf16x8 bq = c1_row_bf(px[2 * q], px[2 * q + 1]);
        lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[2][q], bq, lo, 0, 0, 0);
        mi = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[1][q], bq, mi, 0, 0, 0);
        hi = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[0][q], bq, hi, 0, 0, 0);
      }
      if (p < OHW)                                  // the position's 64-byte row, this lane's quarter
        *reinterpret_cast<g3_f32x4*>(y + ((n0 + f) * (int64_t)OHW + p) * C16_F + kq * 4) = c1_relu(((lo + mi) + hi) + b4);
      if (tn >= tend) break;
      tt = tn; f = fn; p = pn;
#pragma unroll
      for (int k = 0; k < 4 * P; ++k) px[k] = pxn[k];
    }
#undef C16_TILE_READ
  }
}

// weight-gradient staging: 16 consecutive pixels of a plane (index 16 o ..) -> halfwords 4 o .. 4 o + 3 of each of the four
// sub-planes (pitch Pd4 halfwords): byte s of the vector's four dwords, one 8 B LDS store per sub-plane
__device__ __forceinline__ void c16_stage16(uint4 v, uint16_t* dst, int Pd4) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const unsigned lo = __builtin_amdgcn_perm(__float_as_uint(c1_byte(v.y, s)), __float_as_uint(c1_byte(v.x, s)), 0x07060302u);
    const unsigned hi = __builtin_amdgcn_perm(__float_as_uint(c1_byte(v.w, s)), __float_as_uint(c1_byte(v.z, s)), 0x07060302u);
    *reinterpret_cast<uint2*>(dst + s * Pd4) = make_uint2(lo, hi);
  }
}

// The g side of the weight gradient, C1WrwG (conv_u8.hpp) at one filter tile: lane (j, kq) of K-step ks owns octet 4 ks + kq
// (8 consecutive ow of one output row, `no` octets per row) and filter j.  gf = g + frame offset + j; MASK: yf = the forward
// output at the same place.  Per K-step: take(ks), then request(ks + 4) if there is one, then split() — the next K-step's
// values are requested before this K-step's split and MFMAs.
template <bool MASK>
struct C16WrwG {
  float gn[8], yn[8], gc[8];              // [position of the octet]: requested g, requested y, g as it enters the product
  __device__ __forceinline__ void request(const float* gf, const float* yf, int ks, int kq, int no, int OH, int OW) {
    const int o = ks * 4 + kq;
    const int ohr = o / no, ow0 = (o - ohr * no) * 8;
    const int oh = ohr < OH ? ohr : OH - 1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int ow = ow0 + e;
      const int off = (oh * OW + (ow < OW ? ow : OW - 1)) * C16_F;
      gn[e] = gf[off];
      if (MASK) yn[e] = yf[off];
    }
  }
  // the requested values of K-step ks, masked by the layer's ReLU (MASK) and zeroed beyond the row / the last row: the tail
  // octet carries g = 0.  (oh, ow0): the lane's octet.
  __device__ __forceinline__ void take(int ks, int kq, int no, int OH, int OW, int& oh, int& ow0) {
    const int o = ks * 4 + kq;
    const int ohr = o / no;
    ow0 = (o - ohr * no) * 8;
    const bool row_ok = ohr < OH;
    oh = row_ok ? ohr : OH - 1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float t = gn[e];
      if (MASK) t = yn[e] > 0.f ? t : 0.f;
      gc[e] = (row_ok && ow0 + e < OW) ? t : 0.f;
    }
  }
  // those values summed into dbs (MASK) and split three ways: ap[part] = 8 bf16 along k
  __device__ __forceinline__ void split(uint4 (&ap)[3], float& dbs) const {
    float gv[2][4];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      gv[e >> 2][e & 3] = gc[e];
      if (MASK) dbs += gc[e];
    }
    uint2 h0, m0, l0, h1, m1, l1;
    g3_split4(gv[0], h0, m0, l0);
    g3_split4(gv[1], h1, m1, l1);
    ap[0] = make_uint4(h0.x, h0.y, h1.x, h1.y);
    ap[1] = make_uint4(m0.x, m0.y, m1.x, m1.y);
    ap[2] = make_uint4(l0.x, l0.y, l1.x, l1.y);
  }
};

// dW[f][c][kh][kw] = scale * sum over (n, oh, ow) of g[n][oh][ow][f] * float(x[n][c][4 oh + kh][4 ow + kw]).  Lane (j, kq) of a
// K-step owns octet 4 ks + kq: its 8 A values are g[oh][ow0 .. ow0 + 7][filter j], its 8 B values for tap (c, kh, kw) the
// pixels x[c][4 oh + kh][4 (ow0 + e) + kw], e < 8.  Tap group tg = 4 c + t, t < 4: kh = 2 t + (j >> 3), kw = j & 7, so that
// tg * 16 + j IS the flattened (c, kh, kw) index.  Sub-plane s of plane c lies at halfword (4 c + s) Pd4, its slack behind
// H W / 4 zeroed once.  Frame n goes to workgroup n % gridDim.x.
template <int P, bool MASK>
__global__ void __launch_bounds__(256, CF16<P>::WRW_WAVES)
k_c16_u8_wrw(int N, int H, int W, int OH, int OW, int Pd4, const uint8_t* __restrict__ x, const float* __restrict__ g,
             float* __restrict__ partial, const float* __restrict__ yv) {
  constexpr int TG = CF16<P>::TG;
  extern __shared__ __align__(16) uint8_t c16_lds[];
  uint16_t* px = reinterpret_cast<uint16_t*>(c16_lds);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, kq = lane >> 4;
  const int HW = H * W, OHW = OH * OW, hw16 = HW >> 4, HW4 = HW >> 2, W4 = W >> 2;
  const int no = (OW + 7) >> 3, octets = OH * no, ksteps = (octets + 3) >> 2;
  const int tap_off = (j & 3) * Pd4 + (j >> 3) * W4 + ((j >> 2) & 1);     // sub-plane kw & 3, kernel row parity, kw >> 2
  float dbs = 0.f;
  C16WrwG<MASK> gs;
  g3_f32x4 acc[TG];
#pragma unroll
  for (int t = 0; t < TG; ++t) acc[t] = g3_f32x4{0.f, 0.f, 0.f, 0.f};
  // the slack behind each sub-plane is read (tail octets, the widened dword) but never staged: zero it once — any finite
  // value would do, times g = 0
  for (int sp = 0; sp < 4 * P; ++sp)
    for (int i = HW4 + tid; i < Pd4; i += 256) px[sp * Pd4 + i] = 0;
  bool first = true;
  for (int n = blockIdx.x; n < N; n += gridDim.x) {
    if (!first) __syncthreads();                  // every wave is done reading the previous frame
    first = false;
#pragma unroll 1
    for (int c = 0; c < P; ++c) {
      const uint4* s4 = reinterpret_cast<const uint4*>(x + ((int64_t)n * P + c) * HW);
      uint16_t* pc = px + c * 4 * Pd4;
      for (int o0 = tid; o0 < hw16; o0 += 256 * 2) {
        uint4 v[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) { const int o = o0 + k * 256; v[k] = s4[o < hw16 ? o : hw16 - 1]; }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
          const int o = o0 + k * 256;
          if (o < hw16) c16_stage16(v[k], pc + o * 4, Pd4);
        }
      }
    }
    __syncthreads();
    const float* gf = g + (int64_t)n * OHW * C16_F + j;
    const float* yf = MASK ? yv + (gf - g) : nullptr;
    if (wave < ksteps) gs.request(gf, yf, wave, kq, no, OH, OW);
    for (int ks = wave; ks < ksteps; ks += 4) {
      int oh, ow0;                                  // this lane's octet: 8 consecutive ow of output row oh
      uint4 ap[3];                                  // [part] = 8 bf16 along k
      gs.take(ks, kq, no, OH, OW, oh, ow0);
      if (ks + 4 < ksteps) gs.request(gf, yf, ks + 4, kq, no, OH, OW);
      gs.split(ap, dbs);
      // tap (c, 2 t + (j >> 3), j & 7): halfwords a .. a + 7 with a = a0 + c 4 Pd4 + 2 t W4; both steps are even, so the parity
      // of a is a0's and the dword below a is p0 + c 2 Pd4 + t W4
      const int a0 = tap_off + (oh * C1_S) * W4 + ow0;
      const unsigned sh = (unsigned)(a0 & 1) << 4;
      const uint32_t* p0 = reinterpret_cast<const uint32_t*>(c16_lds) + (a0 >> 1);
#pragma unroll
      for (int c = 0; c < P; ++c) {
        // a plane's four tap groups' dwords first (20 LDS reads in flight), then its 12 MFMAs
        uint32_t raw[4][5];
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int e = 0; e < 5; ++e) raw[t][e] = p0[c * 2 * Pd4 + t * W4 + e];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          const uint32_t* rw = raw[t];
          const g3_bf16x8 bv = c1_as_bf8(make_uint4(__builtin_amdgcn_alignbit(rw[1], rw[0], sh), __builtin_amdgcn_alignbit(rw[2], rw[1], sh),
                                                    __builtin_amdgcn_alignbit(rw[3], rw[2], sh), __builtin_amdgcn_alignbit(rw[4], rw[3], sh)));
#pragma unroll
          for (int p = 2; p >= 0; --p)              // smallest part of g first
            acc[4 * c + t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(c1_as_bf8(ap[p]), bv, acc[4 * c + t], 0, 0, 0);
        }
      }
    }
  }
  // Epilogue: the four waves add up in LDS (every wave done with the frame) in wave order.  Accumulator tile t: row
  // 4 kq + r <-> filter 4 kq + r, column j <-> tap t * 16 + j.  MASK: the bias gradient — lane (j, kq) summed filter j over
  // its octets — the four kq in a fixed butterfly, the four waves in wave order behind the 16 x 64 P weight sums.
  constexpr int ROW = TG * 16, DW = CF16<P>::DW;
  float* red = reinterpret_cast<float*>(c16_lds);
  __syncthreads();
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int t = 0; t < TG; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i0 = (4 * kq + r) * ROW + t * 16 + j;
          red[i0] = (w ? red[i0] : 0.f) + acc[t][r];
        }
    }
    __syncthreads();
  }
  if (MASK) {
    dbs += __shfl_xor(dbs, 16);
    dbs += __shfl_xor(dbs, 32);
    for (int w = 0; w < 4; ++w) {
      if (wave == w && kq == 0) red[DW + j] = (w ? red[DW + j] : 0.f) + dbs;
      __syncthreads();
    }
  }
  float* out = partial + (int64_t)blockIdx.x * CF16<P>::SLAB;
  for (int k = tid; k < (MASK ? DW + C16_F : DW); k += 256) out[k] = red[k];
}

// dw[f][c][kh][kw] (element strides so, sc, sh, sw; one plane: sc = 0) = scale * sum of the slabs in a fixed order: a block
// owns 64 consecutive sums, its wave w adds the w-th quarter of the slabs in slab order on four interleaved chains, the
// four waves' sums are added in wave order.  The order depends on `parts` alone.
template <int P>
__global__ void __launch_bounds__(256)
k_c16_wrw_reduce(const float* __restrict__ partial, int parts, float scale, float* __restrict__ dw, int64_t so, int64_t sc, int64_t sh,
                 int64_t sw, float* __restrict__ db) {
  constexpr int DW = CF16<P>::DW, SLAB = CF16<P>::SLAB;
  __shared__ float red[4][64];
  const int c = threadIdx.x & 63, w = threadIdx.x >> 6, t = blockIdx.x * 64 + c;
  const int total = DW + (db ? C16_F : 0);
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

static int c16_query(int64_t* out, int64_t value) {
  if (!out) return fail(MIRL_ERR_ARG, "null out");
  *out = value;
  return MIRL_OK;
}

template <int P>
static int c16_supported(int32_t H, int32_t W, int32_t F, int32_t K, int32_t S) {
  return F == C16_F && K == C1_K && S == C1_S && CF16<P>::shape_ok(H, W) ? 1 : 0;
}

// flags: bit 3 = skip the weight packing (wpk was packed by an earlier call with the same weights and scale)
template <int P>
static int c16_fwd(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* weight, int64_t ws_o, int64_t ws_c, int64_t ws_h,
                   int64_t ws_w, const float* bias, float scale, float* wpk, float* y, int32_t flags, void* stream) {
  using T = CF16<P>;
  using Nm = CF16Names<P>;
  if (int rc = c1_check_args(Nm::fwd, N, x && weight && bias && wpk && y, T::shape_ok(H, W), aligned16(x, y, bias, wpk))) return rc;
  if (flags & ~8) return fail(MIRL_ERR_ARG, std::string(Nm::fwd) + ": unknown flag bits");
  hipStream_t st = (hipStream_t)stream;
  const int OW = c1_out(W), HW = H * W, OHW = c1_out(H) * OW, tiles = (OHW + 15) / 16;
  if (!c1_wpk_holds(wpk, C16_WPK_TAG<P>, flags & 8))
    return fail(MIRL_ERR_STATE, std::string(Nm::fwd) + ": flags bit 3 (weights already packed) but this scratch block was not packed by this entry point");
  if (!(flags & 8)) {
    ProfScope ps(Nm::k_pack, P * C1_TAPS * C16_F * 4 + T::WPK * 4.0, st);
    hipLaunchKernelGGL(k_c16_pack_w<P>, dim3(P), dim3(128), 0, st, weight, ws_o, ws_c, ws_h, ws_w, scale, (uint4*)wpk);
    MIRL_LAUNCH_CHECK();
  }
  const C1FwdPlan pl = T::fwd_plan(N, H, W);
  ProfScope ps(Nm::k_fwd, (double)N * (P * HW + (double)OHW * C16_F * 4), st, (double)N * OHW * 2.0 * P * C1_TAPS * C16_F);
  hipLaunchKernelGGL(k_c16_u8_fwd<P>, dim3(pl.grid), dim3(256), pl.lds, st, (int)N, W, OW, HW, OHW, tiles, magic_u32(OW), magic_u32(tiles),
                     pl.fpi, pl.split, x, (const uint4*)wpk, bias, y);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

// MASK: g is the gradient w.r.t. the layer's output, masked by y > 0 while it is loaded, db its column sums.  The masked
// form reports shape and alignment under the unmasked name.
template <int P, bool MASK>
static int c16_wrw(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* g, const float* y, float scale, float* scratch,
                   float* dw, int64_t ws_o, int64_t ws_c, int64_t ws_h, int64_t ws_w, float* db, void* stream) {
  using T = CF16<P>;
  using Nm = CF16Names<P>;
  if (int rc = c1_check_args(MASK ? Nm::wrw_masked : Nm::wrw, N, x && g && scratch && dw && (!MASK || (y && db)), T::shape_ok(H, W),
                             aligned16(x, g, y, scratch), Nm::wrw))
    return rc;
  hipStream_t st = (hipStream_t)stream;
  const int OH = c1_out(H), OW = c1_out(W), HW = H * W;
  const C1WrwPlan pl = T::wrw_plan(N, H, W);
  {
    ProfScope ps(Nm::k_wrw, (double)N * (P * HW + (MASK ? 2.0 : 1.0) * OH * OW * C16_F * 4), st, (double)N * OH * OW * 2.0 * P * C1_TAPS * C16_F);
    hipLaunchKernelGGL((k_c16_u8_wrw<P, MASK>), dim3(pl.grid), dim3(256), pl.lds, st, (int)N, H, W, OH, OW, pl.pitch, x, g, scratch, y);
    MIRL_LAUNCH_CHECK();
  }
  const int total = T::DW + (MASK ? C16_F : 0);
  ProfScope ps(Nm::k_reduce, (double)pl.grid * total * 4, st);
  hipLaunchKernelGGL(k_c16_wrw_reduce<P>, dim3((total + 63) / 64), dim3(256), 0, st, scratch, (int)pl.grid, scale, dw, ws_o, ws_c, ws_h, ws_w,
                     db);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

}  // namespace mirl

using namespace mirl;

// One plane: no channel stride.  Three and four planes: the rows family's three-plane argument lists.
#define MIRL_C16_ENTRY_POINTS(PFX, P)                                                                                                   \
  extern "C" int PFX##supported(int32_t H, int32_t W, int32_t F, int32_t K, int32_t S) { return c16_supported<P>(H, W, F, K, S); }      \
  extern "C" int PFX##wpk_floats(int64_t* out) { return c16_query(out, CF16<P>::WPK); }                                                 \
  extern "C" int PFX##wrw_scratch_floats(int64_t* out) { return c16_query(out, CF16<P>::SCRATCH_FLOATS); }                              \
  extern "C" int PFX##fwd(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* weight, int64_t ws_o, int64_t ws_c,           \
                          int64_t ws_h, int64_t ws_w, const float* bias, float scale, float* wpk, float* y, int32_t flags,              \
                          void* stream) {                                                                                               \
    return c16_fwd<P>(N, H, W, x, weight, ws_o, ws_c, ws_h, ws_w, bias, scale, wpk, y, flags, stream);                                  \
  }                                                                                                                                     \
  extern "C" int PFX##wrw(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* g, float scale, float* scratch, float* dw,    \
                          int64_t ws_o, int64_t ws_c, int64_t ws_h, int64_t ws_w, void* stream) {                                       \
    return c16_wrw<P, false>(N, H, W, x, g, nullptr, scale, scratch, dw, ws_o, ws_c, ws_h, ws_w, nullptr, stream);                      \
  }                                                                                                                                     \
  extern "C" int PFX##wrw_masked(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* dy, const float* y, float scale,       \
                                 float* scratch, float* dw, int64_t ws_o, int64_t ws_c, int64_t ws_h, int64_t ws_w, float* db,          \
                                 void* stream) {                                                                                        \
    return c16_wrw<P, true>(N, H, W, x, dy, y, scale, scratch, dw, ws_o, ws_c, ws_h, ws_w, db, stream);                                 \
  }
MIRL_C16_ENTRY_POINTS(mirl_conv1f16p3_u8_, 3)
MIRL_C16_ENTRY_POINTS(mirl_conv1f16p4_u8_, 4)
#undef MIRL_C16_ENTRY_POINTS

extern "C" int mirl_conv1f16p_u8_supported(int32_t H, int32_t W, int32_t F, int32_t K, int32_t S) { return c16_supported<1>(H, W, F, K, S); }
extern "C" int mirl_conv1f16p_u8_wpk_floats(int64_t* out) { return c16_query(out, CF16<1>::WPK); }
extern "C" int mirl_conv1f16p_u8_wrw_scratch_floats(int64_t* out) { return c16_query(out, CF16<1>::SCRATCH_FLOATS); }
extern "C" int mirl_conv1f16p_u8_fwd(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* weight, int64_t ws_o, int64_t ws_h,
                                     int64_t ws_w, const float* bias, float scale, float* wpk, float* y, int32_t flags, void* stream) {
  return c16_fwd<1>(N, H, W, x, weight, ws_o, 0, ws_h, ws_w, bias, scale, wpk, y, flags, stream);
}
extern "C" int mirl_conv1f16p_u8_wrw(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* g, float scale, float* scratch,
                                     float* dw, int64_t ws_o, int64_t ws_h, int64_t ws_w, void* stream) {
  return c16_wrw<1, false>(N, H, W, x, g, nullptr, scale, scratch, dw, ws_o, 0, ws_h, ws_w, nullptr, stream);
}
extern "C" int mirl_conv1f16p_u8_wrw_masked(int64_t N, int32_t H, int32_t W, const uint8_t* x, const float* dy, const float* y,
                                            float scale, float* scratch, float* dw, int64_t ws_o, int64_t ws_h, int64_t ws_w,
                                            float* db, void* stream) {
  return c16_wrw<1, true>(N, H, W, x, dy, y, scale, scratch, dw, ws_o, 0, ws_h, ws_w, db, stream);
}
