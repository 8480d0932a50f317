// conv_small.hip — data and weight gradients of the small nature CNN's second layer on the bf16 matrix pipe, f32 results.
//
// Reference: the backward autograd derives for `F.relu(conv(x))` (rltime/models/torch/modules/cnn.py:47-49) at the second
// layer of configs/models/modules/nature_cnn_small.json: Conv2d(16 -> 32, kernel 4, stride 2), valid padding; NHWC f32
// operands.  Both kernels use csrc/gemm3.hip's arithmetic: every f32 operand is split exactly into three bf16 parts while
// its tile is staged, six part products go through v_mfma_f32_16x16x32_bf16 and are accumulated in f32; no float atomics,
// a fixed reduction order (bit-identical reruns).
//
// The shape has no home in conv_mid.hip / conv_wrw.hip: 32 filters are two MFMA row tiles, 16 channels ONE column tile,
// and a frame is small (20 x 20 x 16 floats in, 9 x 9 x 32 out at Atari size), so the layer moves about as many bytes as
// its six part products cost in matrix time.  Both kernels are therefore laid out around the frame's traffic:
//
// k_conv2s_bwd_data   dx[2u+ph][2v+pw][c] = sum over a, b in {0,1}, f < 32 of g[u-a][v-b][f] * W[f][c][ph+2a][pw+2b]
//   Four parity-class GEMMs (ph, pw) with K = 4 taps x 32 filters = 128 = FOUR K-steps (one tap each) and N = 16 channels:
//   one accumulator per 16-pixel tile.
//   * a workgroup is 4 waves = the 4 classes.  Each wave splits ITS 16 x 128 weights in the prologue, straight from the
//     weight's four strides (32 strided loads per lane, 32 KB that stay in L2), and keeps the 48 VGPRs for the launch: no
//     pack launch, no scratch.
//   * a frame's g is staged ONCE, split into three bf16 parts, inside a zero border (so edge taps need no masks), in the
//     chunk layout of k_conv2_bwd_data_b3: the 16-byte chunk (8 filters) kq of position pos sits at
//     (kq & 1) * HP + (kq >> 1) * S + pos * 16, consecutive positions = consecutive 16-byte units.  All four classes read it.
//     26 KB for a 9 x 9 frame: five workgroups per CU cover each other's load latency.
//   * per 16-pixel tile a wave reads 4 K-steps x 3 parts x 16 B and issues 24 MFMAs on two chains; the epilogue is one
//     16-byte store per lane (4 consecutive channels of one pixel).
//   * input heights / widths the stride leaves partly uncovered (IH = 2 OH + 3) get one more pixel row per class; those
//     pixels are stored as exact zeros whatever the weights hold.
//
// k_conv2s_wrw        dw[f][kh][kw][c] = sum over n, oh, ow of g[n][oh][ow][f] * x[n][2oh+kh][2ow+kw][c]
//   D[32 filters][256 taps], K = positions.  A tap tile of 16 columns is ONE (kh, kw) with the 16 channels as columns.
//   * a workgroup (4 waves) takes a contiguous run of frames and keeps the whole 32 x 256 accumulator in registers across
//     the run: wave kh owns the taps (kh, 0..3) for both filter tiles = 8 tiles = 32 VGPRs.
//   * K runs over OCTETS: 8 consecutive ow of one output row (rows padded to a multiple of 8 with g = 0); a K-step is four
//     octets, one per lane quarter.  g is staged transposed, [octet][filter][8 positions]: an A fragment is one 16-byte read.
//   * x is staged transposed by column parity, [ih][iw & 1][octet of iw >> 1][c][8]: the 8 positions of tap (kh, kw) are the
//     entries ow + (kw >> 1) .. + 7 of row (2 oh + kh, kw & 1, c).  kw = 0 and 1 are aligned 16-byte reads; kw = 2 and 3 are
//     THE SAME reads shifted by one halfword with the first halfword of the next octet (v_alignbit, no second read of the
//     octet): per K-step a wave reads 6 x (16 + 4) bytes of x and 6 x 16 of g for its 48 MFMAs.  A tap's operand is a
//     window of the staged frame, never a gather from HBM.
//   * one slab per workgroup; k_conv2s_wrw_reduce sums the slabs in index order.
#include "common.hpp"
#include "split3.hpp"
#include <stdlib.h>

namespace mirl {

typedef float cs_f4 __attribute__((ext_vector_type(4)));

constexpr int CS_C = 16, CS_F = 32, CS_K = 4, CS_S = 2;
constexpr int CS_DW = CS_F * CS_K * CS_K * CS_C;   // 8192 weight-gradient elements = one slab
constexpr int CS_BWD_WGS = 1280;                   // data gradient: most workgroups (5 per CU: 82 VGPRs, 26 KB of LDS at 9 x 9)
constexpr int CS_WRW_WGS = 256;                    // weight gradient: most workgroups = most slabs (1 per CU: a frame's planes are 120 KB)
constexpr size_t CS_BWD_LDS = 64 * 1024;           // what the data gradient may ask for: the 64 KiB a kernel gets unasked
constexpr size_t CS_WRW_LDS = 150 * 1024;          // the weight gradient's raised limit
constexpr int CS_LD = 3;                           // staging loads (data gradient: 16-byte vectors; weight gradient: items of 8) in flight per lane

__device__ __forceinline__ int cs_div(int n, int d, unsigned magic) { return d == 1 ? n : (int)__umulhi((unsigned)n, magic); }

__device__ __forceinline__ void cs_split8(const float (&q)[8], uint4& h, uint4& m, uint4& l) {
  const float q0[4] = {q[0], q[1], q[2], q[3]}, q1[4] = {q[4], q[5], q[6], q[7]};
  uint2 h0, m0, l0, h1, m1, l1;
  g3_split4(q0, h0, m0, l0);
  g3_split4(q1, h1, m1, l1);
  h = make_uint4(h0.x, h0.y, h1.x, h1.y);
  m = make_uint4(m0.x, m0.y, m1.x, m1.y);
  l = make_uint4(l0.x, l0.y, l1.x, l1.y);
}

// ---------------------------------------------------------------------------------------------------------------
struct CsBwdArgs {
  const float* g; const float* w; float* dx;
  int64_t so, sc, sh, sw;       // the weight's element strides (logical [32][16][4][4])
  int N, OH, OW, IH, IW;
  int U, V;                     // pixels per class: ceil(IH / 2) x ceil(IW / 2)
  unsigned v_magic, ow_magic;
  int S, HP;                    // bytes between the chunk planes of a half / per half plane (see cs_chunk_stride)
};

// bytes between the two chunk planes of a half (16 more than a multiple of 256: the 8-byte staging writes of one position's
// chunks then spread over the banks) and per half plane (a multiple of 256: the 16 positions of a ds_read_b128 group are
// 16 consecutive units whichever lane quarter a lane is in)
inline int cs_chunk_stride(int npos) { return ((npos + 15) / 16) * 256 + 16; }
inline int cs_half_plane(int npos) { return (2 * cs_chunk_stride(npos) + 255) / 256 * 256; }

// g: float [N][OH][OW][32]; dx: float [N][IH][IW][16] (NHWC memory), IH in {2 OH + 2, 2 OH + 3}, IW likewise
__global__ void __launch_bounds__(256)
k_conv2s_bwd_data(CsBwdArgs a) {
  extern __shared__ __align__(16) char cs_lds[];
  const int tid = threadIdx.x, lane = tid & 63, cls = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, kq = lane >> 4;
  const int ph = cls >> 1, pw = cls & 1;
  // this wave's weights: channel j (the MFMA row), K-step s = tap (a, b) = (s >> 1, s & 1), filters 8 kq .. 8 kq + 7
  g3_bf16x8 wr[4][3];
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const int kh = ph + 2 * (s >> 1), kw = pw + 2 * (s & 1);
    float q[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) q[e] = a.w[(8 * kq + e) * a.so + j * a.sc + kh * a.sh + kw * a.sw];
    uint4 h, m, l;
    cs_split8(q, h, m, l);
    wr[s][0] = __builtin_bit_cast(g3_bf16x8, h);
    wr[s][1] = __builtin_bit_cast(g3_bf16x8, m);
    wr[s][2] = __builtin_bit_cast(g3_bf16x8, l);
  }
  // the bordered grid: (U + 1) x (V + 1) positions, g[oh][ow] at (1 + oh, 1 + ow), zero elsewhere
  const int PW = a.V + 1, UV = a.U * a.V, plane = 2 * a.HP;
  const int vecs = a.OH * a.OW * 8;             // 16 B vectors per frame of g
  // zero all three parts once: the border stays zero, the fills only write interiors
  for (int o = tid; o < 3 * plane / 16; o += 256) reinterpret_cast<uint4*>(cs_lds)[o] = make_uint4(0u, 0u, 0u, 0u);
  for (int n = blockIdx.x; n < a.N; n += gridDim.x) {
    __syncthreads();                            // zeroing / every wave done with the previous frame
    {
      const cs_f4* s4 = reinterpret_cast<const cs_f4*>(a.g + (int64_t)n * a.OH * a.OW * CS_F);
      for (int o0 = tid; o0 < vecs; o0 += 256 * CS_LD) {
        cs_f4 v[CS_LD];
#pragma unroll
        for (int k = 0; k < CS_LD; ++k) { const int o = o0 + k * 256; v[k] = s4[o < vecs ? o : vecs - 1]; }
#pragma unroll
        for (int k = 0; k < CS_LD; ++k) {
          const int o = o0 + k * 256;
          if (o < vecs) {
            const int pos = o >> 3, sub = o & 7, chunk = sub >> 1;     // 4 filters of chunk (= reader's lane quarter) sub >> 1
            const int oh2 = cs_div(pos, a.OW, a.ow_magic), ow2 = pos - oh2 * a.OW;
            const float x[4] = {v[k].x, v[k].y, v[k].z, v[k].w};
            uint2 hh, mm, ll;
            g3_split4(x, hh, mm, ll);
            char* d = cs_lds + (chunk & 1) * a.HP + (chunk >> 1) * a.S + ((1 + oh2) * PW + 1 + ow2) * 16 + (sub & 1) * 8;
            *reinterpret_cast<uint2*>(d) = hh;
            *reinterpret_cast<uint2*>(d + plane) = mm;
            *reinterpret_cast<uint2*>(d + 2 * plane) = ll;
          }
        }
      }
    }
    __syncthreads();
    float* dxn = a.dx + (int64_t)n * a.IH * a.IW * CS_C;
    for (int p0 = 0; p0 < UV; p0 += 16) {
      const int p = p0 + j, pc = p < UV ? p : UV - 1;
      const int u = cs_div(pc, a.V, a.v_magic), v = pc - u * a.V;
      // position (u - a, v - b) inside the bordered grid, this lane's filter quarter
      const char* base = cs_lds + (kq & 1) * a.HP + (kq >> 1) * a.S + ((1 + u) * PW + 1 + v) * 16;
      g3_bf16x8 b[4][3];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const char* pb = base - ((s >> 1) * PW + (s & 1)) * 16;
#pragma unroll
        for (int q = 0; q < 3; ++q) b[s][q] = *reinterpret_cast<const g3_bf16x8*>(pb + q * plane);
      }
      // two independent chains (taps a = 0 / a = 1); smallest products first: (lo,hi) (hi,lo) (mid,mid) (mid,hi) (hi,mid) (hi,hi)
      g3_f32x4 acc[2] = {g3_f32x4{0.f, 0.f, 0.f, 0.f}, g3_f32x4{0.f, 0.f, 0.f, 0.f}};
      constexpr int PA[6] = {2, 0, 1, 1, 0, 0};
      constexpr int PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int c = 0; c < 6; ++c)
#pragma unroll
          for (int h = 0; h < 2; ++h)
            acc[h] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wr[2 * h + t][PA[c]], b[2 * h + t][PB[c]], acc[h], 0, 0, 0);
      g3_f32x4 r = acc[0] + acc[1];
      const int ih = 2 * u + ph, iw = 2 * v + pw;
      if (p < UV && ih < a.IH && iw < a.IW) {
        if (u > a.OH || v > a.OW) r = g3_f32x4{0.f, 0.f, 0.f, 0.f};      // a row / column no output position covers
        *reinterpret_cast<g3_f32x4*>(dxn + ((int64_t)ih * a.IW + iw) * CS_C + 4 * kq) = r;
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
struct CsWrwArgs {
  const float* x; const float* g; float* partial;
  int N, H, W, OH, OW;
  int run;                      // frames per workgroup (contiguous)
  int octs;                     // octets per output row: ceil(OW / 8)
  int xo;                       // octets per staged x row: octs + 1 (the shifted taps read the first entry of the next one)
  int xocts;                    // octets of a staged x row that hold pixels: ceil(ceil(W / 2) / 8)
  int Opad;                     // octets per frame, padded to a multiple of 4 (one K-step = 4 octets)
  unsigned octs_magic, xocts_magic;
  int xplane, gplane;           // halfwords per part: H * 2 * xo * 16 * 8 and Opad * 32 * 8
};

__global__ void __launch_bounds__(256)
k_conv2s_wrw(CsWrwArgs a) {
  extern __shared__ __align__(16) char cs_lds[];
  uint16_t* xs = reinterpret_cast<uint16_t*>(cs_lds);                       // [3][H][2][xo][16 c][8]
  uint16_t* gs = xs + 3 * a.xplane;                                         // [3][Opad][32 f][8]
  const int tid = threadIdx.x, lane = tid & 63, kh = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int j = lane & 15, kq = lane >> 4;
  const int fx = a.H * a.W * CS_C, fg = a.OH * a.OW * CS_F, octets = a.OH * a.octs;
  // entries no fill writes (the octet behind a row's last pixel octet) are read by the shifted taps of positions whose g
  // is zero: they must be finite, so the planes are zeroed once
  for (int o = tid; o < 3 * (a.xplane + a.gplane) / 8; o += 256) reinterpret_cast<uint4*>(cs_lds)[o] = make_uint4(0u, 0u, 0u, 0u);
  g3_f32x4 acc[2][4];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[m][t] = g3_f32x4{0.f, 0.f, 0.f, 0.f};

  // x item: the 8 entries iw >> 1 = 8 oct .. 8 oct + 7 of row (ih, par = iw & 1, c).  The 32 lanes (par, c) of an item row read
  // 128 contiguous bytes per load.
  auto load_x8 = [&](float (&q)[8], const float* xf, int it) {
    const int c = it & 15, par = (it >> 4) & 1, r = it >> 5;
    const int ih = cs_div(r, a.xocts, a.xocts_magic), oct = r - ih * a.xocts;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int iw = 2 * (8 * oct + e) + par;
      const float t = xf[(ih * a.W + (iw < a.W ? iw : a.W - 1)) * CS_C + c];
      q[e] = iw < a.W ? t : 0.f;
    }
  };
  auto put_x8 = [&](const float (&q)[8], int it) {
    const int c = it & 15, par = (it >> 4) & 1, r = it >> 5;
    const int ih = cs_div(r, a.xocts, a.xocts_magic), oct = r - ih * a.xocts;
    uint4 h, m, l;
    cs_split8(q, h, m, l);
    uint16_t* d = xs + ((((ih * 2 + par) * a.xo + oct) * 16) + c) * 8;
    *reinterpret_cast<uint4*>(d) = h;
    *reinterpret_cast<uint4*>(d + a.xplane) = m;
    *reinterpret_cast<uint4*>(d + 2 * a.xplane) = l;
  };
  // g item: the 8 positions of octet o = (oh, oct) for filter f; zero beyond the row's OW positions and in the padding octets
  auto load_g8 = [&](float (&q)[8], const float* gf, int it) {
    const int f = it & 31, o = it >> 5;
    const int oh = cs_div(o, a.octs, a.octs_magic), oct = o - oh * a.octs;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int ow = 8 * oct + e;
      const bool ok = o < octets && ow < a.OW;
      const float t = gf[ok ? (oh * a.OW + ow) * CS_F + f : f];
      q[e] = ok ? t : 0.f;
    }
  };
  auto put_g8 = [&](const float (&q)[8], int it) {
    uint4 h, m, l;
    cs_split8(q, h, m, l);
    uint16_t* d = gs + it * 8;                  // (o * 32 + f) * 8
    *reinterpret_cast<uint4*>(d) = h;
    *reinterpret_cast<uint4*>(d + a.gplane) = m;
    *reinterpret_cast<uint4*>(d + 2 * a.gplane) = l;
  };

  const int xitems = a.H * a.xocts * 32, gitems = a.Opad * 32, ksteps = a.Opad >> 2;
  const int n_begin = blockIdx.x * a.run, n_end = n_begin + a.run < a.N ? n_begin + a.run : a.N;
  for (int n = n_begin; n < n_end; ++n) {
    const float* xf = a.x + (int64_t)n * fx;
    const float* gf = a.g + (int64_t)n * fg;
    __syncthreads();                              // zeroing / every wave done with the previous frame
    for (int it0 = tid; it0 < xitems; it0 += 256 * CS_LD) {
      float q[CS_LD][8];
#pragma unroll
      for (int k = 0; k < CS_LD; ++k) { const int it = it0 + k * 256; load_x8(q[k], xf, it < xitems ? it : xitems - 1); }
#pragma unroll
      for (int k = 0; k < CS_LD; ++k) { const int it = it0 + k * 256; if (it < xitems) put_x8(q[k], it); }
    }
    for (int it0 = tid; it0 < gitems; it0 += 256 * CS_LD) {
      float q[CS_LD][8];
#pragma unroll
      for (int k = 0; k < CS_LD; ++k) { const int it = it0 + k * 256; load_g8(q[k], gf, it < gitems ? it : gitems - 1); }
#pragma unroll
      for (int k = 0; k < CS_LD; ++k) { const int it = it0 + k * 256; if (it < gitems) put_g8(q[k], it); }
    }
    __syncthreads();
    for (int ks = 0; ks < ksteps; ++ks) {
      const int o = ks * 4 + kq, oc = o < octets ? o : octets - 1;   // a padding octet (g = 0) reads the last real one's window
      const int oh = cs_div(oc, a.octs, a.octs_magic), oct = oc - oh * a.octs;
      g3_bf16x8 af[2][3];
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int p = 0; p < 3; ++p) af[m][p] = *reinterpret_cast<const g3_bf16x8*>(gs + p * a.gplane + (o * 32 + 16 * m + j) * 8);
      // rows (2 oh + kh, par) of channel j: the octet and the first two entries of the next one
      const uint16_t* xr = xs + (((((2 * oh + kh) * 2) * a.xo + oct) * 16) + j) * 8;
      uint4 lo[3][2];
      uint32_t nx[3][2];
#pragma unroll
      for (int p = 0; p < 3; ++p)
#pragma unroll
        for (int par = 0; par < 2; ++par) {
          const uint16_t* s = xr + p * a.xplane + par * a.xo * 128;
          lo[p][par] = *reinterpret_cast<const uint4*>(s);
          nx[p][par] = *reinterpret_cast<const uint32_t*>(s + 128);
        }
      constexpr int PA[6] = {2, 0, 1, 1, 0, 0};
      constexpr int PB[6] = {0, 2, 1, 0, 1, 0};
#pragma unroll
      for (int kw = 0; kw < 4; ++kw) {
        g3_bf16x8 bf[3];
#pragma unroll
        for (int p = 0; p < 3; ++p) {
          const uint4 v = lo[p][kw & 1];
          const uint32_t t = nx[p][kw & 1];
          // entries ow + 1 .. ow + 8: the octet shifted down by one halfword
          const uint4 sh = make_uint4(__builtin_amdgcn_alignbit(v.y, v.x, 16), __builtin_amdgcn_alignbit(v.z, v.y, 16),
                                      __builtin_amdgcn_alignbit(v.w, v.z, 16), __builtin_amdgcn_alignbit(t, v.w, 16));
          bf[p] = __builtin_bit_cast(g3_bf16x8, (kw >> 1) ? sh : v);
        }
        // smallest products first: (lo,hi) (hi,lo) (mid,mid) (mid,hi) (hi,mid) (hi,hi); the two filter tiles are independent chains
#pragma unroll
        for (int c = 0; c < 6; ++c)
#pragma unroll
          for (int m = 0; m < 2; ++m)
            acc[m][kw] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[m][PA[c]], bf[PB[c]], acc[m][kw], 0, 0, 0);
      }
    }
  }
  // the workgroup's slab [f][kh][kw][c]: accumulator (m, kw): row 4 kq + r <-> filter 16 m + 4 kq + r, column j <-> channel j
  float* out = a.partial + (int64_t)blockIdx.x * CS_DW;
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int kw = 0; kw < 4; ++kw)
#pragma unroll
      for (int r = 0; r < 4; ++r) out[((16 * m + 4 * kq + r) * (CS_K * CS_K) + kh * CS_K + kw) * CS_C + j] = acc[m][kw][r];
}

// dw[i] = sum over the slabs of partial[s][i] in slab order (four floats per thread, four independent partial sums)
__global__ void __launch_bounds__(256)
k_conv2s_wrw_reduce(const cs_f4* __restrict__ partial, int parts, cs_f4* __restrict__ dw) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  constexpr int n4 = CS_DW / 4;
  if (i >= n4) return;
  cs_f4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0, s2 = s0, s3 = s0;
  int p = 0;
  for (; p + 4 <= parts; p += 4) {
    s0 += partial[(int64_t)p * n4 + i]; s1 += partial[(int64_t)(p + 1) * n4 + i];
    s2 += partial[(int64_t)(p + 2) * n4 + i]; s3 += partial[(int64_t)(p + 3) * n4 + i];
  }
  for (; p < parts; ++p) s0 += partial[(int64_t)p * n4 + i];
  dw[i] = (s0 + s1) + (s2 + s3);
}

// ---------------------------------------------------------------------------------------------------------------
// The LDS plans of both kernels for an H x W input frame: what mirl_conv2s_supported() gates and the launchers use.
struct CsPlan {
  int OH, OW, U, V, S, HP;
  size_t bwd_lds;
  int octs, xo, xocts, Opad, xplane, gplane;
  size_t wrw_lds;
};
static bool cs_plan(int H, int W, CsPlan* p) {
  if (H < CS_K || W < CS_K || H > 4096 || W > 4096) return false;
  p->OH = (H - CS_K) / CS_S + 1; p->OW = (W - CS_K) / CS_S + 1;
  p->U = (H + 1) / 2; p->V = (W + 1) / 2;
  const int npos = (p->U + 1) * (p->V + 1);
  p->S = cs_chunk_stride(npos); p->HP = cs_half_plane(npos);
  p->bwd_lds = (size_t)3 * 2 * p->HP;
  p->octs = (p->OW + 7) / 8; p->xo = p->octs + 1; p->xocts = ((W + 1) / 2 + 7) / 8;
  p->Opad = (p->OH * p->octs + 3) / 4 * 4;
  p->xplane = H * 2 * p->xo * 16 * 8; p->gplane = p->Opad * 32 * 8;
  p->wrw_lds = (size_t)3 * 2 * ((size_t)p->xplane + p->gplane);
  return p->bwd_lds <= CS_BWD_LDS && p->wrw_lds <= CS_WRW_LDS;
}

}  // namespace mirl

extern "C" int mirl_conv2s_supported(int32_t C, int32_t F, int32_t K, int32_t S, int32_t H, int32_t W) {
  using namespace mirl;
  if (C != CS_C || F != CS_F || K != CS_K || S != CS_S) return 0;
  CsPlan p;
  return cs_plan(H, W, &p) ? 1 : 0;
}

extern "C" int mirl_conv2s_bwd_data(int64_t N, int32_t IH, int32_t IW, const float* g, const float* weight, int64_t ws_o,
                                    int64_t ws_c, int64_t ws_h, int64_t ws_w, float* dx, void* stream) {
  using namespace mirl;
  if (N <= 0 || N >= (1LL << 30) || !g || !weight || !dx) return fail(MIRL_ERR_ARG, "bad conv2s_bwd_data arguments");
  CsPlan p;
  if (!cs_plan(IH, IW, &p)) return fail(MIRL_ERR_ARG, "conv2s_bwd_data: unsupported shape");
  if (!aligned16(g, dx)) return fail(MIRL_ERR_ARG, "conv2s_bwd_data: pointers must be 16-byte aligned");
  CsBwdArgs a;
  a.g = g; a.w = weight; a.dx = dx; a.so = ws_o; a.sc = ws_c; a.sh = ws_h; a.sw = ws_w;
  a.N = (int)N; a.OH = p.OH; a.OW = p.OW; a.IH = IH; a.IW = IW; a.U = p.U; a.V = p.V;
  a.v_magic = magic_u32(p.V); a.ow_magic = magic_u32(p.OW); a.S = p.S; a.HP = p.HP;
  hipStream_t st = (hipStream_t)stream;
  // flop: the convolution's own 2 * K*K*C*F per output position (the zero border is issued work, not algorithmic work)
  ProfScope ps("k_conv2s_bwd_data", (double)N * 4.0 * ((double)p.OH * p.OW * CS_F + (double)IH * IW * CS_C), st,
               (double)N * p.OH * p.OW * 2.0 * CS_K * CS_K * CS_C * CS_F);
  hipLaunchKernelGGL(k_conv2s_bwd_data, dim3(capped_grid(N, CS_BWD_WGS)), dim3(256), p.bwd_lds, st, a);
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}

extern "C" int mirl_conv2s_wrw_scratch_bytes(int64_t* bytes) {
  if (!bytes) return mirl::fail(MIRL_ERR_ARG, "conv2s_wrw_scratch_bytes: null out");
  *bytes = (int64_t)mirl::CS_WRW_WGS * mirl::CS_DW * (int64_t)sizeof(float);   // one [32][4][4][16] slab per workgroup
  return MIRL_OK;
}

extern "C" int mirl_conv2s_wrw(int64_t N, int32_t H, int32_t W, const float* x, const float* g, void* scratch,
                               int64_t scratch_bytes, float* dw, void* stream) {
  using namespace mirl;
  if (N <= 0 || N >= (1LL << 30) || !x || !g || !scratch || !dw) return fail(MIRL_ERR_ARG, "bad conv2s_wrw arguments");
  CsPlan p;
  if (!cs_plan(H, W, &p)) return fail(MIRL_ERR_ARG, "conv2s_wrw: unsupported shape");
  if (!aligned16(x, g, scratch, dw)) return fail(MIRL_ERR_ARG, "conv2s_wrw: pointers must be 16-byte aligned");
  // a contiguous run of frames per workgroup: one frame each until every CU has a workgroup, then equal runs
  const int run = (int)((N + CS_WRW_WGS - 1) / CS_WRW_WGS);
  const unsigned grid = (unsigned)((N + run - 1) / run);
  if (scratch_bytes < (int64_t)grid * CS_DW * (int64_t)sizeof(float)) return fail(MIRL_ERR_ARG, "conv2s_wrw: scratch too small");
  CsWrwArgs a;
  a.x = x; a.g = g; a.partial = (float*)scratch;
  a.N = (int)N; a.H = H; a.W = W; a.OH = p.OH; a.OW = p.OW; a.run = run;
  a.octs = p.octs; a.xo = p.xo; a.xocts = p.xocts; a.Opad = p.Opad;
  a.octs_magic = magic_u32(p.octs); a.xocts_magic = magic_u32(p.xocts);
  a.xplane = p.xplane; a.gplane = p.gplane;
  hipStream_t st = (hipStream_t)stream;
  if (int rc = raise_lds_limit(k_conv2s_wrw, CS_WRW_LDS)) return rc;
  {
    ProfScope ps("k_conv2s_wrw", 4.0 * (double)N * ((double)H * W * CS_C + (double)p.OH * p.OW * CS_F), st,
                 2.0 * (double)N * p.OH * p.OW * CS_DW);
    hipLaunchKernelGGL(k_conv2s_wrw, dim3(grid), dim3(256), p.wrw_lds, st, a);
    MIRL_LAUNCH_CHECK();
  }
  ProfScope ps("k_conv2s_wrw_reduce", (double)(grid + 1) * CS_DW * 4.0, st);
  hipLaunchKernelGGL(k_conv2s_wrw_reduce, dim3(CS_DW / 4 / 256), dim3(256), 0, st, reinterpret_cast<const cs_f4*>(scratch), (int)grid,
                     reinterpret_cast<cs_f4*>(dw));
  MIRL_LAUNCH_CHECK();
  return MIRL_OK;
}
