// The counter-based draw of the read bootstraps, in ONE place for boot_resample (gk_boot.hip) and
// callboot_draw (gk_callboot.hip): draw i of replicate b of stream g picks one of n reads from those numbers and the seed
// alone (a splitmix64 finish, its high 32 bits scaled to [0, n)).  tests/boot_reference.py restates it independently.
#pragma once
#include <stdint.h>

#ifndef GK_HD
#define GK_HD __host__ __device__
#endif

constexpr uint64_t kGkDrawGolden = 0x9E3779B97F4A7C15ull;      // the step of the draw counter (2^64 / the golden ratio)
constexpr uint64_t kGkDrawMix1 = 0xBF58476D1CE4E5B9ull;        // splitmix64's two multipliers: the steps of the replicate
constexpr uint64_t kGkDrawMix2 = 0x94D049BB133111EBull;        // and of the stream as well

GK_HD static inline uint32_t gk_boot_draw(uint64_t seed, uint64_t i, uint64_t b, uint64_t g, uint32_t n) {
  uint64_t z = seed + (i + 1) * kGkDrawGolden + (b + 1) * kGkDrawMix1 + (g + 1) * kGkDrawMix2;
  z ^= z >> 30; z *= kGkDrawMix1;
  z ^= z >> 27; z *= kGkDrawMix2;
  z ^= z >> 31;
  return (uint32_t)(((z >> 32) * (uint64_t)n) >> 32);      // < n
}
