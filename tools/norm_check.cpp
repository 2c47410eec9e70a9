// DefaultNormalizeScore exactness check for the sweep's truncation formula
// (ksched_kernels.hip normalize_inv):
//   floor(100 * raw / max) == (uint32_t) fma((double)(100u * raw), RN(1/max), 2^-40)
//   for 0 <= raw <= max < 2^25, RN(1/max) taken as 0 for max == 0 (giving 0,
//   as norm_check_kernel and the host's guesses store it).
// Covers every pair 0 <= raw <= max <= 16384 (taint counts and sums of
// preferred weights in practice) and the top corner of the stated range,
// max in [2^25 - 4096, 2^25), raw in [max - 4096, max], where 100 * raw is
// largest and the quotient sits next to 100.
// Build: g++ -O2 -mfma -ffp-contract=off norm_check.cpp -o norm_check
#include <cmath>
#include <cstdint>
#include <cstdio>
int main() {
  uint64_t bad = 0, n = 0;
  auto test = [&](uint32_t raw, uint32_t max) {
    const uint32_t want = max ? (uint32_t)((uint64_t)100u * raw / max) : 0u;
    const double inv = max ? 1.0 / (double)max : 0.0;
    const uint32_t got = (uint32_t)std::fma((double)(100u * raw), inv, 0x1p-40);
    ++n;
    if (got != want) {
      if (bad < 10) printf("MISMATCH raw=%u max=%u want=%u got=%u\n", raw, max, want, got);
      ++bad;
    }
  };
  for (uint32_t max = 0; max <= 16384; ++max)
    for (uint32_t raw = 0; raw <= max; ++raw) test(raw, max);
  const uint32_t top = 1u << 25;
  for (uint32_t max = top - 4096; max < top; ++max)
    for (uint32_t raw = max - 4096; raw <= max; ++raw) test(raw, max);
  printf("checked %llu, mismatches %llu\n", (unsigned long long)n, (unsigned long long)bad);
  return bad != 0;
}
