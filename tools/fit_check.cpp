// Exactness check for the general NodeResourcesFit scorer (ksched_eval.hpp
// fit_resource / score_fit_general):
//
// (1) MostAllocated per resource.  With cap = Allocatable (1 <= cap < 2^44),
//     z = the node's NonZeroRequested and p = the pod's non-zero request, the
//     kernel computes, all in binary64,
//       lf100 = (cap - z) * 100, x = lf100 - p * 100, cap100 = cap * 100,
//       q = fma(min(cap100 - x, cap100), RN(1 / cap), 2^-45), score = cvt_u32(q)
//     which must equal min(z + p, cap) * 100 / cap in integers: for every
//     requested value on small capacities, next to every integer quotient on
//     random capacities up to 2^44, next to powers of two, and beyond capacity
//     (the clamp: non-zero defaults can exceed Allocatable).
// (2) LeastAllocated through the same function: requested > capacity gives a
//     negative q, which the unsigned conversion turns into 0.
// (3) The weighted division: floor(n / d) == (2 n * ceil(2^31 / d)) >> 32 for
//     every n <= 20000 (100 x 100 + 100 x 100) and every d in 1..200, and 0
//     for d == 0 (n is 0 there).
// Build: g++ -O2 -mfma -ffp-contract=off fit_check.cpp -o fit_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>

static uint32_t cvt_u32(double q) {  // v_cvt_u32_f64: truncation, negative -> 0
  if (!(q > 0.0)) return 0u;
  if (q >= 4294967295.0) return 0xFFFFFFFFu;
  return (uint32_t)q;
}

static uint32_t fit_resource(bool most, double lf100, double nz100, double cap, double inv) {
  double x = lf100 - nz100;
  const double cap100 = cap * 100.0;
  if (most) x = std::fmin(cap100 - x, cap100);
  return cvt_u32(std::fma(x, inv, 0x1p-45));
}

static uint32_t weight_rcp(uint32_t d) { return d ? (uint32_t)(((1ull << 31) + d - 1) / d) : 0u; }
static uint32_t umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

int main() {
  std::mt19937_64 g(11);
  uint64_t bad = 0, n = 0;
  // z: node NonZeroRequested, p: pod non-zero request (z + p may exceed cap)
  auto test = [&](int64_t z, int64_t p, int64_t cap) {
    if (z < 0 || p < 0 || cap < 1) return;
    const int64_t req = z + p;
    const double capd = (double)cap, inv = 1.0 / capd;
    const double lf100 = (double)(cap - z) * 100.0, nz100 = (double)p * 100.0;
    const int64_t want_most = (int64_t)(((unsigned __int128)(req < cap ? req : cap) * 100u) / (uint64_t)cap);
    const int64_t want_least = req > cap ? 0 : (int64_t)(((unsigned __int128)(cap - req) * 100u) / (uint64_t)cap);
    const int64_t got_most = fit_resource(true, lf100, nz100, capd, inv);
    const int64_t got_least = fit_resource(false, lf100, nz100, capd, inv);
    n += 2;
    if (got_most != want_most || got_least != want_least) {
      if (bad < 10)
        printf("MISMATCH z=%lld p=%lld cap=%lld most %lld/%lld least %lld/%lld\n", (long long)z, (long long)p,
               (long long)cap, (long long)got_most, (long long)want_most, (long long)got_least, (long long)want_least);
      ++bad;
    }
  };
  // every requested value up to 2 cap (the clamp) on small capacities, split two ways
  for (int64_t cap = 1; cap <= 1200; ++cap)
    for (int64_t req = 0; req <= 2 * cap + 2; ++req) {
      test(req, 0, cap);
      test(req / 3, req - req / 3, cap);
    }
  for (int64_t cap : {4000ll, 8000ll, 16000ll, 32000ll, 64000ll, 96000ll, 128000ll})
    for (int64_t req = 0; req <= cap + 200; ++req) test(req - req / 2, req / 2, cap);
  auto near_integers = [&](int64_t cap) {
    for (int64_t k = 0; k <= 100; ++k) {
      const int64_t r0 = (int64_t)(((__int128)k * cap) / 100);  // req * 100 next to k * cap
      for (int64_t d = -3; d <= 3; ++d) {
        const int64_t req = r0 + d;
        if (req < 0) continue;
        const int64_t z = (int64_t)(g() % (uint64_t)(req + 1));
        test(z, req - z, cap);
      }
    }
    test(cap, 0, cap);
    test(0, 0, cap);
    test(0, cap, cap);
    test(cap, 1, cap);          // just beyond capacity
    test(cap, cap, cap);        // twice the capacity
    test(2 * cap, 100000, cap); // a node already beyond its capacity
  };
  for (int i = 0; i < 300000; ++i) {
    const int sh = (int)(g() % 44);
    int64_t cap = (int64_t)(g() >> (64 - 44)) >> sh;
    if (cap < 1) cap = 1;
    near_integers(cap);
    for (int j = 0; j < 4; ++j) {
      const int64_t z = (int64_t)(g() % (uint64_t)(cap + 1)), p = (int64_t)(g() % (uint64_t)(cap / 2 + 2));
      test(z, p, cap);
    }
  }
  for (int e = 1; e <= 44; ++e)
    for (int64_t d = -50; d <= 50; ++d) {
      const int64_t cap = (1ll << e) + d;
      if (cap >= 1 && cap < (1ll << 44)) near_integers(cap);
    }
  near_integers((1ll << 44) - 1);
  const int64_t Gi = 1ll << 30;
  for (int64_t cap : {32 * Gi, 64 * Gi, 256 * Gi, 1024 * Gi, 16383 * Gi})
    for (int64_t req = 0; req <= cap + (64ll << 20); req += 1 << 20) test(req / 2, req - req / 2, cap);

  // (3) the weighted division over its whole domain
  uint64_t nd = 0;
  if (weight_rcp(0) != 0 || umulhi(0u, weight_rcp(0)) != 0) ++bad;
  for (uint32_t d = 1; d <= 200; ++d) {
    const uint32_t rcp = weight_rcp(d);
    for (uint32_t v = 0; v <= 20000; ++v) {
      ++nd;
      if (umulhi(v << 1, rcp) != v / d) {
        if (bad < 10) printf("MISMATCH n=%u d=%u got %u want %u\n", v, d, umulhi(v << 1, rcp), v / d);
        ++bad;
      }
    }
  }
  // and the scorer's own combination for every weight pair on the score corners
  for (uint32_t wc = 0; wc <= 100; ++wc)
    for (uint32_t wm = 0; wm <= 100; ++wm) {
      if (!wc && !wm) continue;
      for (uint32_t sc : {0u, 1u, 37u, 50u, 99u, 100u})
        for (uint32_t sm : {0u, 1u, 37u, 50u, 99u, 100u}) {
          const uint32_t v = wc * sc + wm * sm;
          ++nd;
          if (umulhi(v << 1, weight_rcp(wc + wm)) != v / (wc + wm)) ++bad;
          if (wc && umulhi((wc * sc) << 1, weight_rcp(wc)) != sc) ++bad;
          if (wm && umulhi((wm * sm) << 1, weight_rcp(wm)) != sm) ++bad;
        }
    }
  printf("checked %llu scores and %llu divisions, mismatches %llu\n", (unsigned long long)n, (unsigned long long)nd,
         (unsigned long long)bad);
  return bad != 0;
}
