// capacity_check — host-only check of ks_capacity's exact capped quotient
// (k8s-1m_amd/csrc/ksched_capacity.hpp cap_quot / cap_quot_d)
// against 128-bit integer division over the edge grid: free = q req + {-1, 0,
// 1} for requests from 1 to 2^63 - 1, quotients around every cap, caps from 0
// to 2^31, free values around 2^44, 2^53, 2^62 and 2^63 - 1, and a random
// sweep.  Also counts how often a binary64 divide-and-truncate would have been
// wrong on the same grid (it must be: the grid is there to catch it).
//
// Stand-alone, no HIP, no Python:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -I k8s-1m_amd/csrc -I include tools/capacity_check.cpp -o /tmp/capacity_check && /tmp/capacity_check
#include <stdint.h>
#include <stdio.h>

#include <random>
#include <vector>

#include "ksched_capacity.hpp"

namespace {

uint64_t checked = 0, bad = 0, float_wrong = 0;

void check(int64_t free, int64_t req, uint32_t cap) {
  const unsigned __int128 q = (unsigned __int128)(uint64_t)free / (uint64_t)req;
  const uint32_t want = q < cap ? (uint32_t)q : cap;
  const double rcp = 1.0 / (double)req;
  const uint32_t got = ks::cap_quot(free, req, rcp, cap);
  ++checked;
  if (got != want) {
    if (bad++ < 20) printf("cap_quot(%lld, %lld, cap %u) = %u, want %u\n", (long long)free, (long long)req, cap, got, want);
  }
  if (free < (1ll << 53)) {  // the cpu / memory form: the free value as an exact binary64
    const uint32_t got_d = ks::cap_quot_d(free, (double)free, req, rcp, cap);
    ++checked;
    if (got_d != want) {
      if (bad++ < 20)
        printf("cap_quot_d(%lld, %lld, cap %u) = %u, want %u\n", (long long)free, (long long)req, cap, got_d, want);
    }
  }
  const double fq = (double)free / (double)req;
  const uint32_t shortcut = fq >= (double)cap ? cap : (uint32_t)fq;
  float_wrong += shortcut != want;
}

}  // namespace

int main() {
  const int64_t I63 = INT64_MAX;
  std::vector<int64_t> reqs = {1, 2, 3, 7, 100, 1000, (1ll << 20) + 1, (1ll << 31) - 1, (1ll << 31), (1ll << 32) + 1,
                               (1ll << 43) - 1, (1ll << 44) - 1, (1ll << 46) - 1, (1ll << 53) - 1, (1ll << 53) + 1,
                               (1ll << 62) - 1, (1ll << 62) + 1, I63 - 1, I63};
  std::vector<uint32_t> caps = {0u, 1u, 2u, 3u, 109u, 110u, 111u, 65535u, 65536u, (1u << 24) + 1u, 0x7FFFFFFEu, 0x7FFFFFFFu,
                                0x80000000u};
  std::vector<int64_t> frees = {0, 1, 2, (1ll << 44) - 1, (1ll << 44), (1ll << 53) - 1, (1ll << 53), (1ll << 53) + 1,
                                (1ll << 62) - 1, (1ll << 62), (1ll << 62) + 1, I63 - 1, I63};
  for (int64_t req : reqs) {
    for (uint32_t cap : caps) {
      // quotients around the cap and small ones, free = q req + {-1, 0, 1} where it fits
      std::vector<uint64_t> qs = {0, 1, 2, 3, 5, 109, 110, 111, 65535, 65536, (1ull << 31) - 1, 1ull << 31, (1ull << 31) + 1,
                                  (1ull << 32) - 1, 1ull << 32, (1ull << 32) + 1, (1ull << 40) + 12345};
      for (int d = -3; d <= 3; ++d)
        if ((int64_t)cap + d >= 0) qs.push_back((uint64_t)((int64_t)cap + d));
      for (uint64_t q : qs) {
        const unsigned __int128 base = (unsigned __int128)q * (uint64_t)req;
        for (int d = -1; d <= 1; ++d) {
          const __int128 f = (__int128)base + d;
          if (f < 0 || f > (__int128)I63) continue;
          check((int64_t)f, req, cap);
        }
      }
      for (int64_t f : frees) check(f, req, cap);
    }
  }
  // a random sweep: requests and free values of every magnitude, caps of every magnitude
  std::mt19937_64 rng(20240519);
  for (int i = 0; i < 2000000; ++i) {
    const int rb = 1 + (int)(rng() % 63), fb = 1 + (int)(rng() % 63), cb = (int)(rng() % 32);
    int64_t req = (int64_t)(rng() >> (64 - rb));
    if (req < 1) req = 1;
    int64_t free = (int64_t)(rng() >> (64 - fb));
    if (i & 1) {  // next to an exact multiple
      const uint64_t q = (uint64_t)free / (uint64_t)req;
      const __int128 f = (__int128)q * req + (int)(rng() % 3) - 1;
      if (f >= 0 && f <= (__int128)I63) free = (int64_t)f;
    }
    const uint32_t cap = (uint32_t)(rng() >> 32) >> (31 - cb) >> 1;
    check(free, req, cap > 0x80000000u ? 0x80000000u : cap);
  }
  printf("capacity_check: %llu quotients checked, %llu wrong; a binary64 divide-and-truncate would be wrong on %llu\n",
         (unsigned long long)checked, (unsigned long long)bad, (unsigned long long)float_wrong);
  if (bad) return 1;
  if (!float_wrong) {
    printf("capacity_check: the grid never separates the exact quotient from the float shortcut\n");
    return 1;
  }
  return 0;
}
