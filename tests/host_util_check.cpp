// Stand-alone check of rltime_amd/csrc/host_util.hpp (no HIP): built with the host compiler under
// -fsanitize=address,undefined and run by tests/test_host_util_cpu.py.  The input layer's launch plans are checked
// against what their kernels and scratch blocks can take, and pinned at a few shapes to the values the launchers computed
// inline before the plans moved into the header.
#include <stdint.h>
#include <stdio.h>

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

// Launch-plan values of the input layer as the launchers computed them before they became functions (taken from a copy of
// those expressions, not from host_util.hpp).  kind F / f: forward, four planes / one: a = bf16 kernel, b = frames per
// fill, c = split.  kind W / w / p: weight gradient, four planes bf16 / four planes f32 pipe / one plane: a = masked,
// b = bf16 kernel, c = frames per fill, d = pitch, e = slab floats.
struct Pin { char kind; int H, W; long long N; int a, b, c, d, e; unsigned grid; size_t lds; };
static const Pin pins[] = {
  {'F', 84, 84, 3, 1, 1, 7, 0, 0, 21u, 45312u},
  {'F', 84, 84, 3, 0, 1, 7, 0, 0, 21u, 28928u},
  {'W', 84, 84, 3, 0, 1, 1, 7080, 8192, 3u, 56640u},
  {'w', 84, 84, 3, 0, 0, 1, 7232, 8192, 3u, 32768u},
  {'W', 84, 84, 3, 1, 1, 1, 7080, 8224, 3u, 56640u},
  {'w', 84, 84, 3, 1, 0, 1, 7232, 8224, 3u, 32896u},
  {'f', 84, 84, 3, 0, 1, 7, 0, 0, 21u, 7056u},
  {'p', 84, 84, 3, 0, 1, 1, 7080, 2080, 3u, 14160u},
  {'F', 84, 84, 257, 1, 1, 2, 0, 0, 512u, 45312u},
  {'F', 84, 84, 257, 0, 1, 2, 0, 0, 512u, 28928u},
  {'W', 84, 84, 257, 0, 1, 1, 7080, 8192, 257u, 56640u},
  {'w', 84, 84, 257, 0, 0, 1, 7232, 8192, 257u, 32768u},
  {'W', 84, 84, 257, 1, 1, 1, 7080, 8224, 257u, 56640u},
  {'w', 84, 84, 257, 1, 0, 1, 7232, 8224, 257u, 32896u},
  {'f', 84, 84, 257, 0, 1, 4, 0, 0, 1024u, 7056u},
  {'p', 84, 84, 257, 0, 1, 1, 7080, 2080, 257u, 14160u},
  {'F', 84, 84, 1025, 1, 2, 1, 0, 0, 512u, 74240u},
  {'F', 84, 84, 1025, 0, 2, 1, 0, 0, 512u, 57856u},
  {'W', 84, 84, 1025, 0, 1, 1, 7080, 8192, 512u, 56640u},
  {'w', 84, 84, 1025, 0, 0, 2, 7232, 8192, 512u, 57856u},
  {'W', 84, 84, 1025, 1, 1, 1, 7080, 8224, 512u, 56640u},
  {'w', 84, 84, 1025, 1, 0, 2, 7232, 8224, 512u, 57856u},
  {'f', 84, 84, 1025, 0, 1, 1, 0, 0, 1024u, 7056u},
  {'p', 84, 84, 1025, 0, 1, 1, 7080, 2080, 1024u, 14160u},
  {'F', 84, 84, 2050, 1, 2, 1, 0, 0, 512u, 74240u},
  {'F', 84, 84, 2050, 0, 2, 1, 0, 0, 512u, 57856u},
  {'W', 84, 84, 2050, 0, 1, 1, 7080, 8192, 512u, 56640u},
  {'w', 84, 84, 2050, 0, 0, 2, 7232, 8192, 512u, 57856u},
  {'W', 84, 84, 2050, 1, 1, 1, 7080, 8224, 512u, 56640u},
  {'w', 84, 84, 2050, 1, 0, 2, 7232, 8224, 512u, 57856u},
  {'f', 84, 84, 2050, 0, 2, 1, 0, 0, 1024u, 14112u},
  {'p', 84, 84, 2050, 0, 1, 1, 7080, 2080, 1024u, 14160u},
  {'F', 84, 84, 41472, 1, 2, 1, 0, 0, 512u, 74240u},
  {'F', 84, 84, 41472, 0, 2, 1, 0, 0, 512u, 57856u},
  {'W', 84, 84, 41472, 0, 1, 1, 7080, 8192, 512u, 56640u},
  {'w', 84, 84, 41472, 0, 0, 2, 7232, 8192, 512u, 57856u},
  {'W', 84, 84, 41472, 1, 1, 1, 7080, 8224, 512u, 56640u},
  {'w', 84, 84, 41472, 1, 0, 2, 7232, 8224, 512u, 57856u},
  {'f', 84, 84, 41472, 0, 4, 1, 0, 0, 1024u, 28224u},
  {'p', 84, 84, 41472, 0, 1, 1, 7080, 2080, 1024u, 14160u},
  {'F', 44, 52, 3, 1, 1, 2, 0, 0, 6u, 25856u},
  {'F', 44, 52, 3, 0, 1, 2, 0, 0, 6u, 9472u},
  {'W', 44, 52, 3, 0, 1, 1, 2312, 8192, 3u, 32768u},
  {'w', 44, 52, 3, 0, 0, 1, 2368, 8192, 3u, 32768u},
  {'W', 44, 52, 3, 1, 1, 1, 2312, 8224, 3u, 32896u},
  {'w', 44, 52, 3, 1, 0, 1, 2368, 8224, 3u, 32896u},
  {'f', 44, 52, 3, 0, 1, 2, 0, 0, 6u, 2288u},
  {'p', 44, 52, 3, 0, 1, 1, 2312, 2080, 3u, 8320u},
  {'F', 44, 52, 257, 1, 1, 2, 0, 0, 512u, 25856u},
  {'F', 44, 52, 257, 0, 1, 2, 0, 0, 512u, 9472u},
  {'W', 44, 52, 257, 0, 1, 1, 2312, 8192, 257u, 32768u},
  {'w', 44, 52, 257, 0, 0, 1, 2368, 8192, 257u, 32768u},
  {'W', 44, 52, 257, 1, 1, 1, 2312, 8224, 257u, 32896u},
  {'w', 44, 52, 257, 1, 0, 1, 2368, 8224, 257u, 32896u},
  {'f', 44, 52, 257, 0, 1, 2, 0, 0, 514u, 2288u},
  {'p', 44, 52, 257, 0, 1, 1, 2312, 2080, 257u, 8320u},
  {'F', 44, 52, 1025, 1, 2, 1, 0, 0, 512u, 35328u},
  {'F', 44, 52, 1025, 0, 2, 1, 0, 0, 512u, 18944u},
  {'W', 44, 52, 1025, 0, 1, 1, 2312, 8192, 512u, 32768u},
  {'w', 44, 52, 1025, 0, 0, 2, 2368, 8192, 512u, 32768u},
  {'W', 44, 52, 1025, 1, 1, 1, 2312, 8224, 512u, 32896u},
  {'w', 44, 52, 1025, 1, 0, 2, 2368, 8224, 512u, 32896u},
  {'f', 44, 52, 1025, 0, 1, 1, 0, 0, 1024u, 2288u},
  {'p', 44, 52, 1025, 0, 1, 1, 2312, 2080, 1024u, 8320u},
  {'F', 44, 52, 2050, 1, 2, 1, 0, 0, 512u, 35328u},
  {'F', 44, 52, 2050, 0, 2, 1, 0, 0, 512u, 18944u},
  {'W', 44, 52, 2050, 0, 1, 1, 2312, 8192, 512u, 32768u},
  {'w', 44, 52, 2050, 0, 0, 2, 2368, 8192, 512u, 32768u},
  {'W', 44, 52, 2050, 1, 1, 1, 2312, 8224, 512u, 32896u},
  {'w', 44, 52, 2050, 1, 0, 2, 2368, 8224, 512u, 32896u},
  {'f', 44, 52, 2050, 0, 2, 1, 0, 0, 1024u, 4576u},
  {'p', 44, 52, 2050, 0, 1, 1, 2312, 2080, 1024u, 8320u},
  {'F', 44, 52, 41472, 1, 2, 1, 0, 0, 512u, 35328u},
  {'F', 44, 52, 41472, 0, 2, 1, 0, 0, 512u, 18944u},
  {'W', 44, 52, 41472, 0, 1, 1, 2312, 8192, 512u, 32768u},
  {'w', 44, 52, 41472, 0, 0, 2, 2368, 8192, 512u, 32768u},
  {'W', 44, 52, 41472, 1, 1, 1, 2312, 8224, 512u, 32896u},
  {'w', 44, 52, 41472, 1, 0, 2, 2368, 8224, 512u, 32896u},
  {'f', 44, 52, 41472, 0, 4, 1, 0, 0, 1024u, 9152u},
  {'p', 44, 52, 41472, 0, 1, 1, 2312, 2080, 1024u, 8320u},
  {'F', 100, 100, 1025, 1, 1, 1, 0, 0, 512u, 56576u},
  {'F', 100, 100, 1025, 0, 1, 1, 0, 0, 512u, 40192u},
  {'W', 100, 100, 1025, 0, 1, 1, 10008, 8192, 512u, 80064u},
  {'w', 100, 100, 1025, 0, 0, 1, 10048, 8192, 512u, 40192u},
  {'W', 100, 100, 1025, 1, 1, 1, 10008, 8224, 512u, 80064u},
  {'w', 100, 100, 1025, 1, 0, 1, 10048, 8224, 512u, 40192u},
  {'f', 100, 100, 1025, 0, 1, 1, 0, 0, 1024u, 10000u},
  {'p', 100, 100, 1025, 0, 1, 1, 10008, 2080, 1024u, 20016u},
};

static const long long plan_ns[] = {1, 2, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 41472, (1LL << 30) - 1};

// every check the plans of one supported (H, W) must pass, for a family with `planes` planes
static void check_plans(int planes, int H, int W) {
  using namespace mirl;
  const int OH = c1_out(H), OW = c1_out(W), HW = H * W, tiles = (OH * OW + 15) / 16, Pd = c1_bf_pitch(HW, OW);
  // the highest halfword a bf16 weight-gradient kernel reads in a plane lies inside the pitch, and the frame does
  CHECK((4 * (OH - 1) + 7) * W + 32 * ((OW + 7) / 8) + 3 < Pd && HW <= Pd && Pd % 8 == 0, "%d x %d bf16 pitch %d", H, W, Pd);
  CHECK(c1_pitch(HW) >= HW && c1_pitch(HW) % 16 == 0 && (c1_pitch(HW) / 4) % 64 == 16, "%d x %d pitch %d", H, W, c1_pitch(HW));
  for (long long N : plan_ns) {
    // forward: every variant and every flags override of the four-plane entry point
    for (int v = 0; v < (planes == 4 ? 2 * 3 * 4 : 1); ++v) {
      const bool bf = v & 1;
      const int fpi_flag = (v >> 1) % 3, split_flags[] = {0, 1, 7, 255}, split_flag = split_flags[v / 6];
      const C1FwdPlan p = planes == 4 ? c1_fwd_plan(N, H, W, bf, fpi_flag, split_flag) : c1p_fwd_plan(N, H, W);
      const size_t frame = planes == 4 ? (size_t)C1_PLANES * c1_pitch(HW) : (size_t)HW, limit = planes == 4 && bf ? C1_LDS_FWD_BF : C1_LDS;
      const long long cap = planes == 4 ? C1_WGS : C1P_FWD_WGS;
      CHECK(p.lds <= limit, "fwd %d planes %d x %d N %lld variant %d: lds %zu", planes, H, W, N, v, p.lds);
      CHECK(p.fpi >= 1 && p.fpi <= (planes == 4 ? 2 : C1P_FPI) && (size_t)p.fpi * frame <= p.lds, "fwd %d planes %d x %d N %lld variant %d: fpi %d lds %zu",
            planes, H, W, N, v, p.fpi, p.lds);
      if (planes == 4) CHECK(p.lds == (size_t)p.fpi * frame + (bf ? 16384 : 0), "fwd %d x %d N %lld variant %d: lds %zu", H, W, N, v, p.lds);
      CHECK(p.split >= 1 && p.split <= (tiles + 3) / 4 && (p.fpi == 1 || p.split == 1), "fwd %d planes %d x %d N %lld variant %d: split %d fpi %d",
            planes, H, W, N, v, p.split, p.fpi);
      const long long units = (N + p.fpi - 1) / p.fpi * p.split;
      CHECK(p.grid >= 1 && p.grid <= cap && p.grid == (units < cap ? units : cap), "fwd %d planes %d x %d N %lld variant %d: grid %u", planes, H, W, N, v, p.grid);
    }
    // weight gradient: masked and unmasked, bf16 allowed or not; grid x slab inside what the scratch query reports
    for (int v = 0; v < (planes == 4 ? 4 : 1); ++v) {
      const bool masked = v & 1, allow = !(v & 2);
      const C1WrwPlan p = planes == 4 ? c1_wrw_plan(N, H, W, masked, allow) : c1p_wrw_plan(N, H, W);
      const long long scratch = planes == 4 ? C1_SCRATCH_FLOATS : C1P_SCRATCH_FLOATS;
      const size_t limit = planes == 4 && p.bf16 ? C1_LDS_WRW_B3 : C1_LDS;
      CHECK(p.lds <= limit && p.lds >= (size_t)p.slab * 4, "wrw %d planes %d x %d N %lld variant %d: lds %zu", planes, H, W, N, v, p.lds);
      CHECK(p.grid >= 1 && (long long)p.grid * p.slab <= scratch, "wrw %d planes %d x %d N %lld variant %d: grid %u slab %d", planes, H, W, N, v, p.grid, p.slab);
      CHECK((long long)p.grid <= (N + p.fpi - 1) / p.fpi, "wrw %d planes %d x %d N %lld variant %d: grid %u", planes, H, W, N, v, p.grid);
      if (p.bf16) {
        CHECK(p.fpi == 1 && p.pitch == Pd && (size_t)planes * Pd * 2 <= p.lds, "wrw %d planes %d x %d N %lld variant %d: bf16 pitch %d lds %zu", planes, H, W,
              N, v, p.pitch, p.lds);
        CHECK(p.slab == (planes == 4 ? C1_DW + (masked ? C1_F : 0) : C1P_SLAB), "wrw %d planes slab %d", planes, p.slab);
      } else {
        CHECK(planes == 4 && (p.fpi == 1 || p.fpi == 2) && p.pitch == c1_pitch(HW) && (size_t)p.fpi * C1_PLANES * p.pitch <= p.lds,
              "wrw f32 %d x %d N %lld variant %d: fpi %d pitch %d lds %zu", H, W, N, v, p.fpi, p.pitch, p.lds);
        CHECK(!allow || (size_t)C1_PLANES * Pd * 2 > C1_LDS_WRW_B3, "wrw %d x %d N %lld: f32 pipe although the bf16 frame fits", H, W, N);
      }
    }
  }
}

int main() {
  using namespace mirl;
  // magic_u32: ceil(2^32 / d) for d > 1, 0 for d <= 1; exact n / d by multiply-high for every n < 2^16
  const unsigned ds[] = {1, 2, 3, 7, 19, 20, 21, 84, 85, 65535};
  for (unsigned d : ds) {
    const unsigned m = magic_u32(d);
    if (d <= 1) { CHECK(m == 0u, "d = %u magic = %u", d, m); continue; }
    CHECK((uint64_t)m == ((1ULL << 32) + d - 1) / d, "d = %u magic = %u", d, m);
    for (unsigned n = 0; n < (1u << 16); ++n) CHECK(umulhi(n, m) == n / d, "n = %u d = %u got %u", n, d, umulhi(n, m));
  }
  CHECK(magic_u32(0) == 0u && magic_u32(-3) == 0u, "d <= 0");

  // aligned16: every pointer, variadic; a null pointer counts as aligned
  alignas(16) static char buf[64];
  const float* f = reinterpret_cast<const float*>(buf);
  const uint8_t* b = reinterpret_cast<const uint8_t*>(buf);
  CHECK(aligned16(buf), "base");
  CHECK(aligned16(buf + 16, f, b + 32), "three aligned pointers of different types");
  CHECK(!aligned16(buf + 4), "off by 4");
  CHECK(!aligned16(buf + 8), "off by 8");
  CHECK(!aligned16(f + 1), "float off by 4");
  CHECK(!aligned16(buf, buf + 8, buf + 16), "off by 8 in the middle");
  CHECK(!aligned16(buf, buf + 16, b + 4), "off by 4 at the end");
  CHECK(!aligned16(buf + 4, buf, buf + 16), "off by 4 at the front");
  CHECK(aligned16((const float*)nullptr, buf), "null counts as aligned");
  CHECK(aligned16(), "no pointers");

  // capped_grid: units below the cap, the cap above
  const int64_t caps[] = {1, 256, 512, 4096};
  for (int64_t cap : caps) {
    CHECK(capped_grid(0, cap) == 0u, "0 of %lld", (long long)cap);
    CHECK(capped_grid(cap - 1, cap) == (unsigned)(cap - 1), "cap - 1 of %lld", (long long)cap);
    CHECK(capped_grid(cap, cap) == (unsigned)cap, "cap of %lld", (long long)cap);
    CHECK(capped_grid(cap + 1, cap) == (unsigned)cap, "cap + 1 of %lld", (long long)cap);
  }
  CHECK(capped_grid((int64_t)1 << 40, 512) == 512u, "units beyond 32 bits");

  // the input layer's launch plans at every frame shape a family supports in 8..128 (and 100 x 100)
  int shapes4 = 0, shapes1 = 0;
  for (int H = 8; H <= 128; ++H)
    for (int W = 8; W <= 128; ++W) {
      const bool grid16 = W % 4 == 0 && (H * W) % 16 == 0;
      CHECK(grid16 || (!c1_shape_ok(H, W) && !c1p_shape_ok(H, W)), "%d x %d off the 16-byte grid but supported", H, W);
      if (c1_shape_ok(H, W)) { ++shapes4; check_plans(4, H, W); }
      if (c1p_shape_ok(H, W)) { ++shapes1; check_plans(1, H, W); }
    }
  CHECK(shapes4 > 1000 && shapes1 >= shapes4, "supported shapes: %d four-plane, %d one-plane", shapes4, shapes1);
  CHECK(c1_shape_ok(100, 100) && c1p_shape_ok(100, 100) && c1_shape_ok(84, 84) && c1_shape_ok(8, 8) && c1p_shape_ok(8, 8), "shapes the tests use");
  check_plans(4, 100, 100);
  check_plans(1, 100, 100);
  CHECK(!c1_shape_ok(7, 84) && !c1_shape_ok(84, 7) && !c1_shape_ok(84, 82) && !c1_shape_ok(10, 12) && !c1_shape_ok(128, 132), "refused four-plane shapes");
  CHECK(!c1_shape_ok(65536, 65536) && !c1_shape_ok(1 << 30, 8) && !c1p_shape_ok(4100, 8) && !c1p_shape_ok(8, 4100) && !c1p_shape_ok(256, 256),
        "refused large shapes");
  CHECK(c1p_shape_ok(180, 180) && !c1_shape_ok(180, 180), "one plane takes frames four planes cannot");
  // the size queries' constants against the kernels' layouts
  CHECK(C1_WPK_FLOATS == 12288 && C1_SCRATCH_FLOATS == 512LL * 8224 && C1P_WPK == 3072 && C1P_SCRATCH_FLOATS == 1024LL * 2080, "scratch sizes moved");
  for (const Pin& q : pins) {
    if (q.kind == 'F' || q.kind == 'f') {
      const C1FwdPlan p = q.kind == 'F' ? c1_fwd_plan(q.N, q.H, q.W, q.a, 0, 0) : c1p_fwd_plan(q.N, q.H, q.W);
      CHECK(p.fpi == q.b && p.split == q.c && p.grid == q.grid && p.lds == q.lds, "pinned %c %d x %d N %lld bf %d: fpi %d split %d grid %u lds %zu", q.kind,
            q.H, q.W, q.N, q.a, p.fpi, p.split, p.grid, p.lds);
    } else {
      const C1WrwPlan p = q.kind == 'p' ? c1p_wrw_plan(q.N, q.H, q.W) : c1_wrw_plan(q.N, q.H, q.W, q.a, q.kind == 'W');
      CHECK(p.bf16 == (bool)q.b && p.fpi == q.c && p.pitch == q.d && p.slab == q.e && p.grid == q.grid && p.lds == q.lds,
            "pinned %c %d x %d N %lld masked %d: bf16 %d fpi %d pitch %d slab %d grid %u lds %zu", q.kind, q.H, q.W, q.N, q.a, (int)p.bf16, p.fpi,
            p.pitch, p.slab, p.grid, p.lds);
    }
  }

  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("host_util ok\n");
  return 0;
}
