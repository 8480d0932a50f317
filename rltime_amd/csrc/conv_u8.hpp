// conv_u8.hpp — what the input-layer families share (csrc/conv_in.hip: four-plane uint8 frames, csrc/conv_in_rows.hip:
// one and three planes): the entry points' argument checks and packed-weights bookkeeping, the byte -> bf16 helpers, and
// of the bf16-pipe weight-gradient kernels everything but the frame staging loop and the tap walk.  Launch plans:
// host_util.hpp.
#pragma once
#include "common.hpp"
#include "split3.hpp"
#include <unordered_map>

namespace mirl {

// What every fwd / wrw / wrw_masked entry point checks first.  `entry` names it in the first message, `stem` in the others
// (the masked weight gradients report shape and alignment under the unmasked name).
inline int c1_check_args(const char* entry, int64_t N, bool pointers, bool shape_ok, bool aligned, const char* stem = nullptr) {
  if (!stem) stem = entry;
  if (N <= 0 || N >= (1LL << 30) || !pointers) return fail(MIRL_ERR_ARG, std::string("bad ") + entry + " arguments");
  if (!shape_ok) return fail(MIRL_ERR_ARG, std::string(stem) + ": unsupported frame shape");
  if (!aligned) return fail(MIRL_ERR_ARG, std::string(stem) + ": pointers must be 16-byte aligned");
  return MIRL_OK;
}

// Which kernel variant's operand order a wpk scratch block holds, remembered per pointer (host side, one caller thread per
// the library's contract).  packed = false: `variant` packs it now.  packed = true (flags bit 3): does it hold `variant`'s
// image?  A block packed by another variant or the other family does not.
enum { C1_WPK_F32 = 1, C1_WPK_BF16 = 2, C1_WPK_1P = 3, C1_WPK_3P = 4 };
inline bool c1_wpk_holds(const void* wpk, int variant, bool packed) {
  static std::unordered_map<const void*, int> packed_by;
  if (!packed) { packed_by[wpk] = variant; return true; }
  const auto it = packed_by.find(wpk);
  return it != packed_by.end() && it->second == variant;
}

__device__ __forceinline__ g3_bf16x8 c1_as_bf8(uint4 v) { return __builtin_bit_cast(g3_bf16x8, v); }
__device__ __forceinline__ float c1_byte(uint32_t v, int b) { return (float)((v >> (8 * b)) & 0xffu); }
// bytes (2e, 2e+1) of v -> two bf16 in one dword: float(byte) has at most 8 significant bits, its upper half IS the bf16
__device__ __forceinline__ unsigned c1_bytes_bf(uint32_t v, int e) {
  const float a = c1_byte(v, 2 * e), b = c1_byte(v, 2 * e + 1);
  return __builtin_amdgcn_perm(__float_as_uint(b), __float_as_uint(a), 0x07060302u);
}
// 8 consecutive bytes (two dwords) -> a lane's 8 bf16 k-elements
__device__ __forceinline__ g3_bf16x8 c1_row_bf(uint32_t a, uint32_t b) {
  return c1_as_bf8(make_uint4(c1_bytes_bf(a, 0), c1_bytes_bf(a, 1), c1_bytes_bf(b, 0), c1_bytes_bf(b, 1)));
}
__device__ __forceinline__ g3_f32x4 c1_relu(g3_f32x4 o) {
  o.x = o.x > 0.f ? o.x : 0.f; o.y = o.y > 0.f ? o.y : 0.f; o.z = o.z > 0.f ? o.z : 0.f; o.w = o.w > 0.f ? o.w : 0.f;
  return o;
}
// weight-gradient staging: 16 pixels -> 16 bf16 = two 16 B LDS stores
__device__ __forceinline__ void c1_stage16_bf(uint4 v, uint16_t* dst) {
  uint4* d4 = reinterpret_cast<uint4*>(dst);
  d4[0] = make_uint4(c1_bytes_bf(v.x, 0), c1_bytes_bf(v.x, 1), c1_bytes_bf(v.y, 0), c1_bytes_bf(v.y, 1));
  d4[1] = make_uint4(c1_bytes_bf(v.z, 0), c1_bytes_bf(v.z, 1), c1_bytes_bf(v.w, 0), c1_bytes_bf(v.w, 1));
}

// The g side of a bf16-pipe weight-gradient kernel.  Positions are walked in octets of 8 consecutive ow of one output row
// (`no` octets per row, the tail octet's positions beyond OW carry g = 0); lane (j, kq) of K-step ks owns octet 4 ks + kq and
// filters j and 16 + j.  gf = g + frame offset + j; MASK: yf = the forward output at the same place.  Per K-step a kernel
// calls take(ks), then request(ks + 4) if there is one, then split(): the NEXT K-step's g (and y) values are requested
// before this K-step's split and MFMAs — with two waves per SIMD nothing else covers a global load's latency.  (The
// masked values are a member between take and split, not a local of one function that does all three: with that the
// compiler copies the 32 requested values once more per K-step.)
template <bool MASK>
struct C1WrwG {
  float gn[2][8], yn[2][8], gc[2][8];     // [filter half][position of the octet]: requested g, requested y, g as it enters the product
  __device__ __forceinline__ void request(const float* gf, const float* yf, int ks, int kq, int no, int OH, int OW) {
    const int o = ks * 4 + kq;
    const int ohr = o / no, ow0 = (o - ohr * no) * 8;
    const int oh = ohr < OH ? ohr : OH - 1;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int ow = ow0 + e;
        const int64_t off = (int64_t)(oh * OW + (ow < OW ? ow : OW - 1)) * C1_F + 16 * m;
        gn[m][e] = gf[off];
        if (MASK) yn[m][e] = yf[off];
      }
  }
  // the requested values of K-step ks, masked by the layer's ReLU (MASK) and zeroed beyond the row / the last row: the tail
  // octet carries g = 0.  (oh, ow0): the lane's octet, 8 consecutive ow of output row oh.
  __device__ __forceinline__ void take(int ks, int kq, int no, int OH, int OW, int& oh, int& ow0) {
    const int o = ks * 4 + kq;
    const int ohr = o / no;
    ow0 = (o - ohr * no) * 8;
    const bool row_ok = ohr < OH;
    oh = row_ok ? ohr : OH - 1;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float t = gn[m][e];
        if (MASK) t = yn[m][e] > 0.f ? t : 0.f;
        gc[m][e] = (row_ok && ow0 + e < OW) ? t : 0.f;
      }
  }
  // those values summed into dbs (MASK) and split three ways: ap[filter half][part] = 8 bf16 along k
  __device__ __forceinline__ void split(uint4 (&ap)[2][3], float (&dbs)[2]) const {
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
  }
};

// Epilogue of a bf16-pipe weight-gradient kernel with TG tap groups (16 TG taps per filter): the four waves add up in LDS
// (red, the workgroup's whole dynamic LDS, every wave done with the frame) in wave order.  Accumulator tile (half m, tap
// group t): row 4 kq + r <-> filter 16 m + 4 kq + r, column j <-> tap t * 16 + j.  MASK: the bias gradient — lane (j, kq)
// summed filters j and 16 + j over its octets — the four kq in a fixed butterfly, the four waves in wave order behind the
// 32 x 16 TG weight sums.  Then the slab goes to `out`.
template <int TG, bool MASK>
__device__ __forceinline__ void c1_wrw_epilogue(float* red, const g3_f32x4 (&acc0)[TG], const g3_f32x4 (&acc1)[TG], float (&dbs)[2],
                                                float* __restrict__ out, int tid, int wave, int j, int kq) {
  constexpr int ROW = TG * 16, DW = C1_F * ROW;
  __syncthreads();
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int t = 0; t < TG; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int i0 = (4 * kq + r) * ROW + t * 16 + j, i1 = i0 + 16 * ROW;
          red[i0] = (w ? red[i0] : 0.f) + acc0[t][r];
          red[i1] = (w ? red[i1] : 0.f) + acc1[t][r];
        }
      }
    }
    __syncthreads();
  }
  if (MASK) {
#pragma unroll
    for (int m = 0; m < 2; ++m) { dbs[m] += __shfl_xor(dbs[m], 16); dbs[m] += __shfl_xor(dbs[m], 32); }
    for (int w = 0; w < 4; ++w) {
      if (wave == w && kq == 0) {
        red[DW + j] = (w ? red[DW + j] : 0.f) + dbs[0];
        red[DW + 16 + j] = (w ? red[DW + 16 + j] : 0.f) + dbs[1];
      }
      __syncthreads();
    }
  }
  for (int k = tid; k < (MASK ? DW + C1_F : DW); k += 256) out[k] = red[k];
}

}  // namespace mirl
