// Stand-alone check of rltime_amd/csrc/host_util.hpp (no HIP): built with the host compiler under
// -fsanitize=address,undefined and run by tests/test_host_util_cpu.py.
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

  if (failures) { printf("%d checks failed\n", failures); return 1; }
  printf("host_util ok\n");
  return 0;
}
