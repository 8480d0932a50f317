// host_util.hpp — the launchers' pure host arithmetic (no HIP headers: tests/test_host_util_cpu.py builds it with the host
// compiler alone).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace mirl {

// ceil(2^32 / d) for d > 1, 0 for d <= 1 (a kernel takes n / 1 = n without the multiply).  For n, d < 2^16
// __umulhi(n, magic_u32(d)) == n / d exactly: magic = (2^32 + e) / d with 0 <= e < d, so the product's high word is
// floor(n / d + n e / (d 2^32)) and n e / (d 2^32) < 2^-16 <= 1 / d cannot carry n / d over the next integer.
inline unsigned magic_u32(int64_t d) { return d > 1 ? (unsigned)(((1ULL << 32) + (uint64_t)d - 1) / (uint64_t)d) : 0u; }

// every pointer 16-byte aligned (a null pointer is)
template <typename... P>
inline bool aligned16(const P*... p) { return ((((uintptr_t)p % 16) == 0) && ...); }

// grid of a persistent kernel: one workgroup per work unit up to `cap` resident ones
inline unsigned capped_grid(int64_t units, int64_t cap) { return (unsigned)(units < cap ? units : cap); }

// ---------------------------------------------------------------------------------------------------------------
// The input layer from uint8 frames, Conv2d(planes -> 32, kernel 8, stride 4): launch plans of csrc/conv_in.hip (four
// planes, C1_*) and csrc/conv_in_rows.hip (one and three planes, CRows<P>).  The entry points take no buffer sizes, so
// the size queries and the launchers both read the constants and plans below: what a query reports is what a launcher
// may write.
constexpr int C1_PLANES = 4, C1_K = 8, C1_S = 4, C1_F = 32, C1_TAPS = C1_K * C1_K;
constexpr int C1_DW = C1_F * C1_PLANES * C1_TAPS;   // 8192 weight-gradient elements
constexpr int C1_WGS = 512;                         // most workgroups of a forward or weight-gradient launch (2 per CU) = most slabs
constexpr int C1_WPK_FLOATS = 3 * 2 * C1_K * 64 * 4;   // wpk scratch: three 16 KB weight parts (the f32 kernel's image is 8192 floats)
constexpr int C1_WLO_BYTES = 2 * C1_K * 64 * 16;    // the bf16 forward keeps the lo weight parts in LDS behind the frames
constexpr size_t C1_LDS = 64 * 1024, C1_LDS_WRW_B3 = 80 * 1024, C1_LDS_FWD_BF = 96 * 1024;   // unasked / raised limits
constexpr int64_t C1_SCRATCH_FLOATS = (int64_t)C1_WGS * (C1_DW + C1_F);

inline int c1_out(int hw) { return (hw - C1_K) / C1_S + 1; }   // output rows / columns of H / W

// LDS plane pitch in bytes of the raw four-plane frame: >= HW, a multiple of 16 B, and 16 (mod 64) in dwords
inline int c1_pitch(int HW) {
  int dw = (HW + 3) / 4;
  dw += ((16 - dw % 64) + 64) % 64;
  return dw * 4;
}

// LDS halfwords per plane of the bf16 frame of the bf16 weight-gradient kernels: the frame, the over-read of a row's tail
// octet (its positions beyond OW carry g = 0 but are still read: the last index is (4 (OH - 1) + 7) W + 32 ceil(OW / 8) + 3),
// rounded to 16 bytes
inline int c1_bf_pitch(int HW, int OW) { return (HW + 4 * (8 * ((OW + 7) / 8) - OW) + 8 + 7) / 8 * 8; }

// frame shapes the kernels take: 16 B vectors never straddle planes, and the LDS plan fits what a kernel gets unasked
inline bool c1_shape_ok(int H, int W) {
  if (H < C1_K || W < C1_K || (W % 4) != 0 || (int64_t)H * W > (int64_t)C1_LDS || ((H * W) % 16) != 0) return false;
  return (size_t)C1_PLANES * c1_pitch(H * W) <= C1_LDS;
}

struct C1FwdPlan { int fpi, split; unsigned grid; size_t lds; };   // frames per LDS fill, workgroups per frame, launch
// four planes; bf: the bf16-pipe kernel; fpi / split: the flags' overrides (anything else = choose)
inline C1FwdPlan c1_fwd_plan(int64_t N, int H, int W, bool bf, int fpi, int split) {
  const int pitch = c1_pitch(H * W), tiles = (c1_out(H) * c1_out(W) + 15) / 16;
  const bool fits2 = (size_t)2 * C1_PLANES * pitch <= C1_LDS;
  if (fpi != 1 && fpi != 2) fpi = (N >= 1024 && fits2) ? 2 : 1;
  if (fpi == 2 && !fits2) fpi = 1;
  // few frames: `split` workgroups share one frame's tiles (at least one tile per wave)
  const int max_split = (tiles + 3) / 4;
  if (split <= 0) split = N >= C1_WGS ? 1 : (int)((C1_WGS + N - 1) / N);
  if (split > max_split) split = max_split;
  if (fpi == 2) split = 1;
  return {fpi, split, capped_grid((N + fpi - 1) / fpi * split, C1_WGS), (size_t)fpi * C1_PLANES * pitch + (bf ? C1_WLO_BYTES : 0)};
}

// bf16: the bf16-pipe kernel (else the f32-pipe one, four planes only, with fpi frames per fill); pitch: halfwords per
// plane (bf16) or bytes per plane (f32 pipe); slab: floats a workgroup writes at scratch + blockIdx.x * slab
struct C1WrwPlan { bool bf16; int fpi, pitch, slab; unsigned grid; size_t lds; };
inline size_t c1_at_least_slab(size_t lds, int slab) { return lds < (size_t)slab * 4 ? (size_t)slab * 4 : lds; }   // the partial is reduced there
// four planes; allow_bf16 = false: the f32-pipe kernel (flags / mirl_conv1_wrw_bf16_set), which is also what takes a bf16
// frame beyond 80 KiB (two workgroups per CU)
inline C1WrwPlan c1_wrw_plan(int64_t N, int H, int W, bool masked, bool allow_bf16) {
  const int HW = H * W, slab = C1_DW + (masked ? C1_F : 0), Pd = c1_bf_pitch(HW, c1_out(W)), pitch = c1_pitch(HW);
  if (allow_bf16 && (size_t)C1_PLANES * Pd * 2 <= C1_LDS_WRW_B3)
    return {true, 1, Pd, slab, capped_grid(N, C1_WGS), c1_at_least_slab((size_t)C1_PLANES * Pd * 2, slab)};
  const int fpi = (N >= 1024 && (size_t)2 * C1_PLANES * pitch <= C1_LDS) ? 2 : 1;
  return {false, fpi, pitch, slab, capped_grid((N + fpi - 1) / fpi, C1_WGS), c1_at_least_slab((size_t)fpi * C1_PLANES * pitch, slab)};
}

// ---------------------------------------------------------------------------------------------------------------
// One-plane and three-plane frames (csrc/conv_in_rows.hip): sizes, launch parameters and launch plans by plane count P.
template <int P>
struct CRows {
  static_assert(P == 1 || P == 3, "instantiated for one and three planes");
  static constexpr int PLANES = P, TG = P * 4;        // tap groups of 16 taps: the weight gradient's accumulator tiles per filter half
  static constexpr int DW = C1_F * P * C1_TAPS;       // 2048 / 6144 weight-gradient elements
  static constexpr int SLAB = DW + C1_F;              // floats per workgroup slab: weight sums, then the bias sums (masked form)
  static constexpr int WAVES = P == 1 ? 4 : 2;        // forward: waves per SIMD = resident workgroups per CU
  static constexpr int LD = P == 1 ? 7 : 8;           // forward: staging loads in flight per lane (four 84x84 frames = 6.9 x 256
                                                      // vectors, one 120x80x3 frame = 7.03 x 256)
  static constexpr int WGS = P == 1 ? 1024 : 512;     // weight gradient: most workgroups = most slabs (4 / 2 per CU)
  static constexpr int FWD_WGS = 256 * WAVES;         // forward: most resident workgroups (1024 / 512)
  static constexpr int FPI = 4;                       // most frames per LDS fill
  static constexpr int FILL = 32 * 1024;              // .. and most bytes of one: more than one frame only within this
  static constexpr int WPK = 3 * 2 * P * 2 * 64 * 4;  // packed weight image in floats: [part][instruction q][filter half][lane] x 16 B
  static constexpr size_t LDS = C1_LDS;               // what a launch may ask for: the 64 KiB a kernel gets unasked
  static constexpr int64_t SCRATCH_FLOATS = (int64_t)WGS * SLAB;

  // the weight gradient stages one frame's planes as bf16, each with its tail over-read, within LDS (64 KiB: (1, 100, 100)
  // takes 20 016 bytes, (3, 100, 100) 60 048, (3, 120, 80) 57 792); the forward's raw bytes are half of that
  static bool shape_ok(int H, int W) {
    if (H < C1_K || W < C1_K || H > 4096 || W > 4096 || (W % 4) != 0 || ((H * W) % 16) != 0) return false;
    return (size_t)P * c1_bf_pitch(H * W, c1_out(W)) * 2 <= LDS;
  }
  static C1FwdPlan fwd_plan(int64_t N, int H, int W) {
    const int HWP = P * H * W, tiles = (c1_out(H) * c1_out(W) + 15) / 16;
    // frames per LDS fill: more only once every resident workgroup has a group of its own, and within FILL
    int fpi_max = FILL / HWP;
    fpi_max = fpi_max < 1 ? 1 : (fpi_max > FPI ? FPI : fpi_max);
    const int64_t fpi64 = N / FWD_WGS;
    const int fpi = fpi64 < 1 ? 1 : (fpi64 > fpi_max ? fpi_max : (int)fpi64);
    // few frames: `split` workgroups share one frame's tiles (at least one tile per wave)
    const int max_split = (tiles + 3) / 4;
    int split = N >= FWD_WGS ? 1 : (int)((FWD_WGS + N - 1) / N);
    if (split > max_split) split = max_split;
    return {fpi, split, capped_grid((N + fpi - 1) / fpi * split, FWD_WGS), (size_t)fpi * HWP};
  }
  static C1WrwPlan wrw_plan(int64_t N, int H, int W) {
    const int Pd = c1_bf_pitch(H * W, c1_out(W));
    return {true, 1, Pd, SLAB, capped_grid(N, WGS), c1_at_least_slab((size_t)P * Pd * 2, SLAB)};
  }
};

// the names tests/host_util_check.cpp and tests/host_util_check3p.cpp hold the plans by
constexpr int C1P_SLAB = CRows<1>::SLAB, C1P_FWD_WGS = CRows<1>::FWD_WGS, C1P_FPI = CRows<1>::FPI, C1P_WPK = CRows<1>::WPK;
constexpr int64_t C1P_SCRATCH_FLOATS = CRows<1>::SCRATCH_FLOATS, C3P_SCRATCH_FLOATS = CRows<3>::SCRATCH_FLOATS;
constexpr int C3P_PLANES = CRows<3>::PLANES, C3P_TG = CRows<3>::TG, C3P_SLAB = CRows<3>::SLAB, C3P_WGS = CRows<3>::WGS;
constexpr int C3P_FPI = CRows<3>::FPI, C3P_FILL = CRows<3>::FILL, C3P_WPK = CRows<3>::WPK;
constexpr size_t C3P_LDS = CRows<3>::LDS;
inline bool c1p_shape_ok(int H, int W) { return CRows<1>::shape_ok(H, W); }
inline bool c3p_shape_ok(int H, int W) { return CRows<3>::shape_ok(H, W); }
inline C1FwdPlan c1p_fwd_plan(int64_t N, int H, int W) { return CRows<1>::fwd_plan(N, H, W); }
inline C1FwdPlan c3p_fwd_plan(int64_t N, int H, int W) { return CRows<3>::fwd_plan(N, H, W); }
inline C1WrwPlan c1p_wrw_plan(int64_t N, int H, int W) { return CRows<1>::wrw_plan(N, H, W); }
inline C1WrwPlan c3p_wrw_plan(int64_t N, int H, int W) { return CRows<3>::wrw_plan(N, H, W); }

}  // namespace mirl
