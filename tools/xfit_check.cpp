// Exactness check for NodeResourcesFit over listed extended resources
// (k8s-1m_amd/csrc/ksched_fit_shape.hpp).  It includes
// the header the host runtime and the kernels compile, so what is checked is
// the product's code, against plain int64 arithmetic
// (resource_allocation.go, least_allocated.go, most_allocated.go,
// requested_to_capacity_ratio.go):
//
// (1) fit_x_score, one resource's score from its int64 columns, in both
//     directions: every capacity 1..1200 with every requested 0..2 cap; every
//     power of two below 2^44 and its neighbours, and 200,000 random capacities
//     below 2^44, each with the requested values round every percent boundary
//     (where the quotient's fraction is smallest and largest), 0, cap, beyond
//     cap up to int64's end, and random ones; capacity 0.
// (2) fit_x_div, the LeastAllocated / MostAllocated divide floor(n / d) by the
//     reciprocal multiply, for every d <= 1000 and n <= 100 d.
// (3) fit_x_round_div against llround((double)n / d), which is Go's
//     int64(math.Round(float64(n) / float64(d))), over the same domain.
// (4) The node score as the kernels compose it (fit_x_add / fit_x_add_rtcr,
//     then the divide) for cpu, memory and 1..3 extended resources over a grid
//     of scores that holds 0, with cpu / memory present or not.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -I include -I k8s-1m_amd/csrc tools/xfit_check.cpp -o xfit_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>

#include "ksched_fit_shape.hpp"

using ks::fit_weight_rcp;
using ks::fit_x_add;
using ks::fit_x_add_rtcr;
using ks::fit_x_div;
using ks::fit_x_round_div;
using ks::fit_x_score;
using ks::FitXSum;

static uint64_t bad = 0, nres = 0;

// upstream in integers; 128 bits where req * 100 leaves int64 (upstream itself
// overflows there: the clamp's answer is the one a wider integer gives)
static int64_t want_most(int64_t cap, int64_t req) {
  if (cap == 0) return 0;
  return (int64_t)((__int128)(req < cap ? req : cap) * 100 / cap);
}
static int64_t want_least(int64_t cap, int64_t req) {
  if (cap == 0 || req > cap) return 0;
  return (int64_t)((__int128)(cap - req) * 100 / cap);
}
static void check_res(int64_t cap, int64_t req) {
  nres += 2;
  const int64_t gm = fit_x_score(true, cap, req), gl = fit_x_score(false, cap, req);
  if (gm != want_most(cap, req) || gl != want_least(cap, req)) {
    if (bad++ < 10)
      printf("MISMATCH resource cap=%lld req=%lld most %lld / %lld least %lld / %lld\n", (long long)cap, (long long)req,
             (long long)gm, (long long)want_most(cap, req), (long long)gl, (long long)want_least(cap, req));
  }
}
static void check_cap(int64_t cap, std::mt19937_64 &g) {
  check_res(cap, 0);
  check_res(cap, cap);
  check_res(cap, cap + 1);
  check_res(cap, 2 * cap);
  check_res(cap, INT64_MAX);
  check_res(cap, INT64_MAX - cap);
  for (int64_t k = 0; k <= 100; ++k) {  // requested * 100 / cap crosses k here (and cap - requested likewise)
    const int64_t r = (int64_t)(((__int128)cap * k + 99) / 100);
    for (int64_t e = -2; e <= 2; ++e)
      if (r + e >= 0) check_res(cap, r + e);
  }
  for (int i = 0; i < 8; ++i) check_res(cap, (int64_t)(g() % (uint64_t)(2 * cap + 1)));
}

int main() {
  std::mt19937_64 g(23);
  // (1)
  check_res(0, 0);
  check_res(0, 5);
  for (int64_t cap = 1; cap <= 1200; ++cap)
    for (int64_t req = 0; req <= 2 * cap; ++req) check_res(cap, req);
  for (int b = 0; b < 44; ++b)
    for (int64_t e = -1; e <= 1; ++e) {
      const int64_t cap = (1ll << b) + e;
      if (cap >= 1 && cap < ks::FIT_X_MAX_CAP) check_cap(cap, g);
    }
  check_cap(ks::FIT_X_MAX_CAP - 1, g);
  for (int i = 0; i < 200000; ++i) {
    const int bits = 1 + (int)(g() % 44);
    const int64_t cap = (int64_t)(g() % ((1ull << bits) - 1)) + 1;
    check_cap(cap, g);
  }

  // (2), (3)
  uint64_t ndiv = 0;
  for (uint32_t d = 1; d <= 1000; ++d) {
    const uint32_t rcp = fit_weight_rcp(d);
    for (uint32_t n = 0; n <= 100 * d; ++n) {
      ndiv += 2;
      if (fit_x_div(n, rcp) != n / d) {
        if (bad++ < 10) printf("MISMATCH divide n=%u d=%u got %u want %u\n", n, d, fit_x_div(n, rcp), n / d);
      }
      const long long want = std::llround((double)n / (double)d);
      if ((long long)fit_x_round_div(n, d) != want) {
        if (bad++ < 10) printf("MISMATCH round n=%u d=%u got %u want %lld\n", n, d, fit_x_round_div(n, d), want);
      }
    }
  }
  if (fit_x_div(7, fit_weight_rcp(0)) != 0 || fit_x_round_div(7, 0) != 0) {
    printf("MISMATCH zero divisor\n");
    ++bad;
  }

  // (4) weights: cpu, memory (0: not listed), then up to three extended ones
  uint64_t nscore = 0;
  const uint32_t grid[] = {0, 1, 2, 33, 49, 50, 51, 99, 100};
  const uint32_t wsets[][5] = {{1, 1, 3, 0, 0},  {0, 0, 1, 0, 0},    {2, 0, 1, 5, 0},    {1, 1, 3, 2, 0},
                               {100, 100, 100, 100, 100}, {0, 7, 13, 1, 100}, {1, 0, 1, 1, 1}, {3, 2, 1, 0, 0}};
  for (auto &w : wsets) {
    const int nx = w[4] ? 3 : w[3] ? 2 : 1;
    const uint32_t wx = w[2] + w[3] + w[4];
    for (int hc = 0; hc < 2; ++hc)
      for (int hm = 0; hm < 2; ++hm) {
        // the reciprocals the host computes per pod: xrcp[has_cpu + 2 has_mem]
        const uint32_t rcp = fit_weight_rcp(wx + (hc ? w[0] : 0) + (hm ? w[1] : 0));
        for (uint32_t sc : grid)
          for (uint32_t sm : grid)
            for (uint32_t s0 : grid)
              for (uint32_t s1 : grid)
                for (uint32_t s2 : grid) {
                  if ((nx < 2 && s1 != grid[0]) || (nx < 3 && s2 != grid[0])) continue;
                  const uint32_t s[5] = {hc ? sc : 0, hm ? sm : 0, s0, s1, s2};
                  const bool has[5] = {hc != 0, hm != 0, true, nx >= 2, nx >= 3};
                  // upstream: resources with non-zero allocatable (LeastAllocated /
                  // MostAllocated) or a positive score (RequestedToCapacityRatio)
                  int64_t n = 0, d = 0, dr = 0;
                  for (int k = 0; k < 5; ++k) {
                    if (!has[k]) continue;
                    n += (int64_t)s[k] * w[k];
                    d += w[k];
                    if (s[k] > 0) dr += w[k];
                  }
                  const int64_t want = d ? n / d : 0;
                  const int64_t wantr = dr ? std::llround((double)n / (double)dr) : 0;
                  FitXSum a{0, 0}, b{0, 0};
                  for (int k = 0; k < 5; ++k) {
                    fit_x_add(a, w[k], s[k], has[k]);
                    fit_x_add_rtcr(b, w[k], has[k] ? s[k] : 0u);
                  }
                  nscore += 2;
                  if ((int64_t)a.d != d || (int64_t)fit_x_div(a.n, rcp) != want ||
                      (int64_t)fit_x_round_div(b.n, b.d) != wantr) {
                    if (bad++ < 10)
                      printf("MISMATCH node score got %u / %u want %lld / %lld\n", fit_x_div(a.n, rcp),
                             fit_x_round_div(b.n, b.d), (long long)want, (long long)wantr);
                  }
                }
      }
  }
  printf("checked %llu resource scores, %llu divisions and %llu node scores, mismatches %llu\n",
         (unsigned long long)nres, (unsigned long long)ndiv, (unsigned long long)nscore, (unsigned long long)bad);
  return bad != 0;
}
