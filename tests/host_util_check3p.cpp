// Stand-alone check of the three-plane input layer's launch plans (rltime_amd/csrc/host_util.hpp c3p_*; kernels:
// csrc/conv_in3p.hip), no HIP: built with the host compiler under -fsanitize=address,undefined and run by
// tests/test_host_util3p_cpu.py, as tests/host_util_check.cpp is for the other two families.  The forward's work split is
// WALKED here the way k_conv1p3_u8_fwd walks it — workgroup, work unit, wave, tile, with the kernel's multiply-high
// divisions — and every (frame, tile) must be visited exactly once; the weight gradient's frame -> workgroup map likewise.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../rltime_amd/csrc/host_util.hpp"

static int failures = 0;
#define CHECK(cond, ...)                                   \
  do {                                                     \
    if (!(cond)) {                                         \
      if (++failures <= 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                      \
  } while (0)

// what __umulhi(n, m) computes on the device
static unsigned umulhi(unsigned n, unsigned m) { return (unsigned)(((uint64_t)n * (uint64_t)m) >> 32); }

static void check_shape(int H, int W, long long N) {
  using namespace mirl;
  const int OH = c1_out(H), OW = c1_out(W), OHW = OH * OW, HW = H * W, tiles = (OHW + 15) / 16, Pd = c1_bf_pitch(HW, OW);
  CHECK(c3p_shape_ok(H, W), "%d x %d refused", H, W);

  // ---- forward
  const C1FwdPlan p = c3p_fwd_plan(N, H, W);
  CHECK(p.grid >= 1 && p.grid <= (unsigned)C3P_WGS, "fwd %d x %d N %lld: grid %u", H, W, N, p.grid);
  CHECK(p.lds <= C3P_LDS && p.lds == (size_t)p.fpi * C3P_PLANES * HW, "fwd %d x %d N %lld: lds %zu", H, W, N, p.lds);
  CHECK(p.fpi >= 1 && p.fpi <= C3P_FPI && (p.fpi == 1 || p.lds <= (size_t)C3P_FILL), "fwd %d x %d N %lld: fpi %d", H, W, N, p.fpi);
  CHECK(p.split >= 1 && p.split <= (tiles + 3) / 4 && (p.fpi == 1 || p.split == 1), "fwd %d x %d N %lld: split %d fpi %d", H, W, N, p.split, p.fpi);
  CHECK((size_t)(C3P_PLANES * HW) % 16 == 0, "%d x %d: a frame is not a run of 16-byte vectors", H, W);
  std::vector<int> seen((size_t)N * tiles, 0);
  const unsigned tiles_magic = magic_u32(tiles), ow_magic = magic_u32(OW);
  const int groups = (int)((N + p.fpi - 1) / p.fpi), units = groups * p.split, step = 4 * p.split;
  long long highest_byte = -1;
  for (unsigned block = 0; block < p.grid; ++block)
    for (int u = (int)block; u < units; u += (int)p.grid) {
      const int group = p.split == 1 ? u : u / p.split, part = u - group * p.split;
      const int n0 = group * p.fpi;
      const int frames = N - n0 < p.fpi ? (int)(N - n0) : p.fpi;
      CHECK(frames >= 1 && (size_t)frames * C3P_PLANES * HW <= p.lds, "fwd %d x %d N %lld unit %d: %d frames", H, W, N, u, frames);
      const int tend = frames * tiles;
      for (int wave = 0; wave < 4; ++wave)
        for (int tt = part * 4 + wave; tt < tend; tt += step) {
          const int f = tiles == 1 ? tt : (int)umulhi((unsigned)tt, tiles_magic);
          CHECK(f == tt / tiles && f < frames, "tile %d of %d: frame %d", tt, tiles, f);
          seen[(size_t)(n0 + f) * tiles + (tt - f * tiles)] += 1;
          for (int j = 0; j < 16; ++j) {
            const int pos = (tt - f * tiles) * 16 + j, pc = pos < OHW ? pos : OHW - 1;
            const int oh = OW == 1 ? pc : (int)umulhi((unsigned)pc, ow_magic);
            CHECK(oh == pc / OW, "position %d: row %d", pc, oh);
            // the last byte lane (j, kq = 3) reads: plane 2, kernel row 7, bytes 4 .. 7 of the second dword
            const long long last = (long long)f * C3P_PLANES * HW + 2LL * HW + (oh * C1_S + 7) * W + (pc - oh * OW) * C1_S + 7;
            if (last > highest_byte) highest_byte = last;
          }
        }
    }
  for (size_t i = 0; i < seen.size(); ++i)
    if (seen[i] != 1) { CHECK(seen[i] == 1, "fwd %d x %d N %lld: frame %zu tile %zu visited %d times", H, W, N, i / tiles, i % tiles, seen[i]); break; }
  CHECK(highest_byte < (long long)p.lds, "fwd %d x %d N %lld: byte %lld read of %zu staged", H, W, N, highest_byte, p.lds);

  // ---- weight gradient: frame n -> workgroup n % grid, one slab per workgroup, the three bf16 planes and the slab in LDS
  const C1WrwPlan q = c3p_wrw_plan(N, H, W);
  CHECK(q.bf16 && q.fpi == 1 && q.pitch == Pd && q.slab == C3P_SLAB && C3P_SLAB == C1_F * C3P_PLANES * C1_TAPS + C1_F, "wrw %d x %d: pitch %d slab %d", H, W,
        q.pitch, q.slab);
  CHECK(q.grid >= 1 && q.grid <= (unsigned)C3P_WGS && (long long)q.grid <= N && (long long)q.grid * q.slab <= C3P_SCRATCH_FLOATS, "wrw %d x %d N %lld: grid %u",
        H, W, N, q.grid);
  CHECK(q.lds <= C3P_LDS && q.lds >= (size_t)C3P_PLANES * Pd * 2 && q.lds >= (size_t)q.slab * 4, "wrw %d x %d N %lld: lds %zu", H, W, N, q.lds);
  CHECK((4 * (OH - 1) + 7) * W + 32 * ((OW + 7) / 8) + 3 < Pd && HW <= Pd && Pd % 8 == 0, "%d x %d bf16 pitch %d", H, W, Pd);
  std::vector<int> frames_seen((size_t)N, 0);
  for (unsigned block = 0; block < q.grid; ++block)
    for (long long n = block; n < N; n += q.grid) frames_seen[(size_t)n] += 1;
  for (long long n = 0; n < N; ++n)
    if (frames_seen[(size_t)n] != 1) { CHECK(frames_seen[(size_t)n] == 1, "wrw %d x %d N %lld: frame %lld visited %d times", H, W, N, n, frames_seen[(size_t)n]); break; }
}

int main() {
  using namespace mirl;
  const int shapes[][2] = {{8, 8}, {44, 52}, {120, 80}};
  const long long ns[] = {1, 2, 3, 5, 33, 1025};
  for (const auto& s : shapes)
    for (long long N : ns) check_shape(s[0], s[1], N);
  // the acting batch fills the chip (32 frames of the config's shape: 35 tiles, nine workgroups each), a learner batch takes
  // one frame per fill at that size and four small ones
  const C1FwdPlan a = c3p_fwd_plan(32, 120, 80), l = c3p_fwd_plan(704, 120, 80), m = c3p_fwd_plan(41472, 36, 36);
  CHECK(a.fpi == 1 && a.split == 9 && a.grid == 288u && a.lds == 28800u, "acting plan: fpi %d split %d grid %u lds %zu", a.fpi, a.split, a.grid, a.lds);
  CHECK(l.fpi == 1 && l.split == 1 && l.grid == 512u && l.lds == 28800u, "learner plan: fpi %d split %d grid %u lds %zu", l.fpi, l.split, l.grid, l.lds);
  CHECK(m.fpi == 4 && m.split == 1 && m.grid == 512u && m.lds == 4u * 3888u, "small-frame plan: fpi %d split %d grid %u lds %zu", m.fpi, m.split, m.grid, m.lds);
  // the LDS limit: three bf16 planes with their tail over-read within 64 KiB
  CHECK(C3P_LDS == 65536u && c3p_shape_ok(100, 100) && 3u * 2u * c1_bf_pitch(10000, 24) == 60048u, "(3, 100, 100) fits");
  CHECK(c3p_shape_ok(84, 84) && c3p_shape_ok(36, 36) && c3p_shape_ok(12, 16), "shapes the tests use");
  CHECK(!c3p_shape_ok(108, 104) && !c3p_shape_ok(128, 88) && !c3p_shape_ok(7, 84) && !c3p_shape_ok(84, 82) && !c3p_shape_ok(42, 42) && !c3p_shape_ok(4100, 8),
        "refused shapes");
  // every supported shape in 8..128: plan within the limits at the ends of the N range
  int shapes3 = 0;
  for (int H = 8; H <= 128; ++H)
    for (int W = 8; W <= 128; ++W) {
      if (!c3p_shape_ok(H, W)) continue;
      ++shapes3;
      CHECK(c1p_shape_ok(H, W), "%d x %d: three planes fit but one does not", H, W);
      for (long long N : {1LL, 511LL, 512LL, 2048LL, (1LL << 30) - 1}) {
        const C1FwdPlan p = c3p_fwd_plan(N, H, W);
        const C1WrwPlan q = c3p_wrw_plan(N, H, W);
        CHECK(p.lds <= C3P_LDS && p.grid >= 1 && p.grid <= (unsigned)C3P_WGS && q.lds <= C3P_LDS && (long long)q.grid * q.slab <= C3P_SCRATCH_FLOATS,
              "%d x %d N %lld", H, W, N);
      }
    }
  CHECK(shapes3 > 500, "supported shapes: %d", shapes3);
  CHECK(C3P_WPK == 9216 && C3P_SCRATCH_FLOATS == 512LL * 6176 && C3P_TG == 12, "sizes moved");

  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("host_util 3p ok\n");
  return 0;
}
