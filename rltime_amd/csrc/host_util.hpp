// host_util.hpp — the launchers' pure host arithmetic (no HIP headers: tests/test_host_util_cpu.py builds it with the host
// compiler alone).
#pragma once
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

}  // namespace mirl
