// Exactness check for NodeResourcesFit's RequestedToCapacityRatio
// (k8s-1m_amd/csrc/ksched_fit_shape.hpp).  It includes
// the header the host runtime and the kernels compile, so what is checked is
// the product's code:
//
// (1) fit_shape_table against a direct int64 transcription of
//     helper.BuildBrokenLinearFunction for every argument 0..100: every
//     two-point shape (x0 < x1 in 0..100, scores 0..10: 611,050 shapes), every
//     one-point shape, and 400,000 random shapes of 1..8 points; and its
//     refusals.
// (2) The rounding divide: floor((2 n + d) / (2 d)) by the reciprocal multiply
//     with divisor 2 d against llround((double)n / d), which is Go's
//     int64(math.Round(float64(n) / float64(d))), for every d <= 200 and
//     n <= 100 d.
// (3) fit_rtcr_node_score, the node score as the kernel writes it, against
//     integer arithmetic over every weight pair and a grid of resource scores
//     that holds 0 (a zero score, or a resource masked for zero Allocatable).
// Build: g++ -O2 -std=c++17 -I include -I k8s-1m_amd/csrc tools/rtcr_check.cpp -o rtcr_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "ksched_fit_shape.hpp"

using ks::fit_rtcr_node_score;
using ks::fit_shape_table;
using ks::fit_weight_rcp;

// shape_score.go, transcribed: scores already x 10
static int64_t raw(const std::vector<ks_fit_shape_point> &s, int64_t p) {
  for (size_t i = 0; i < s.size(); ++i) {
    if (p <= s[i].utilization) {
      if (i == 0) return (int64_t)s[0].score * 10;
      const int64_t x0 = s[i - 1].utilization, x1 = s[i].utilization;
      const int64_t y0 = (int64_t)s[i - 1].score * 10, y1 = (int64_t)s[i].score * 10;
      const int64_t num = (y1 - y0) * (p - x0), den = x1 - x0;
      // Go's / spelled out: the magnitude's quotient with the numerator's sign
      const int64_t q = (num < 0 ? -num : num) / den;
      return y0 + (num < 0 ? -q : q);
    }
  }
  return (int64_t)s.back().score * 10;
}

static uint64_t bad = 0;

static void check_shape(const std::vector<ks_fit_shape_point> &s) {
  uint8_t t[101];
  if (!fit_shape_table(s.data(), (uint32_t)s.size(), t)) {
    if (bad++ < 10) printf("REFUSED a valid shape of %zu points\n", s.size());
    return;
  }
  for (int64_t p = 0; p <= 100; ++p)
    if ((int64_t)t[p] != raw(s, p)) {
      if (bad++ < 10) printf("MISMATCH table p=%lld got %d want %lld (%zu points)\n", (long long)p, t[p], (long long)raw(s, p), s.size());
      return;
    }
}

int main() {
  uint64_t nshapes = 0;
  for (int32_t x0 = 0; x0 <= 100; ++x0)
    for (int32_t y0 = 0; y0 <= 10; ++y0) {
      check_shape({{x0, y0}});
      ++nshapes;
      for (int32_t x1 = x0 + 1; x1 <= 100; ++x1)
        for (int32_t y1 = 0; y1 <= 10; ++y1) {
          check_shape({{x0, y0}, {x1, y1}});
          ++nshapes;
        }
    }
  std::mt19937_64 g(17);
  for (int i = 0; i < 400000; ++i) {
    const uint32_t n = 1 + (uint32_t)(g() % 8);
    bool used[101] = {false};
    std::vector<ks_fit_shape_point> s;
    while (s.size() < n) {
      const int32_t x = (int32_t)(g() % 101);
      if (used[x]) continue;
      used[x] = true;
      s.push_back({x, 0});
    }
    std::vector<ks_fit_shape_point> sorted;
    for (int32_t x = 0; x <= 100; ++x)
      if (used[x]) sorted.push_back({x, (int32_t)(g() % 11)});
    check_shape(sorted);
    ++nshapes;
  }
  {  // the longest shape, and the refusals
    std::vector<ks_fit_shape_point> s;
    for (int32_t x = 0; x <= 100; ++x) s.push_back({x, (x * 7) % 11});
    check_shape(s);
    uint8_t t[101];
    s.push_back({100, 1});
    const ks_fit_shape_point dup[2] = {{10, 1}, {10, 2}}, down[2] = {{20, 1}, {10, 2}}, hi[1] = {{101, 1}}, neg[1] = {{-1, 1}},
                             sc[1] = {{5, 11}}, scn[1] = {{5, -1}}, ok[1] = {{5, 5}};
    if (fit_shape_table(s.data(), 102, t) || fit_shape_table(nullptr, 1, t) || fit_shape_table(ok, 0, t) ||
        fit_shape_table(ok, 1, nullptr) || fit_shape_table(dup, 2, t) || fit_shape_table(down, 2, t) ||
        fit_shape_table(hi, 1, t) || fit_shape_table(neg, 1, t) || fit_shape_table(sc, 1, t) ||
        fit_shape_table(scn, 1, t) || !fit_shape_table(ok, 1, t)) {
      printf("MISMATCH refusals\n");
      ++bad;
    }
  }

  // (2) the rounding divide over its whole domain
  uint64_t ndiv = 0;
  for (uint32_t d = 1; d <= 200; ++d) {
    const uint32_t rcp = fit_weight_rcp(2 * d);
    for (uint32_t n = 0; n <= 100 * d; ++n) {
      ++ndiv;
      const uint32_t got = (uint32_t)(((uint64_t)((2 * n + d) << 1) * rcp) >> 32);
      const long long want = std::llround((double)n / (double)d);
      if ((long long)got != want) {
        if (bad++ < 10) printf("MISMATCH round n=%u d=%u got %u want %lld\n", n, d, got, want);
      }
    }
  }

  // (3) the node score as the kernel computes it.  tc / tm arrive masked: 0
  // for a resource with zero Allocatable, whatever T[0] holds.
  uint64_t nscore = 0;
  const uint32_t grid[] = {0, 1, 2, 3, 4, 20, 21, 30, 45, 50, 55, 67, 70, 90, 97, 99, 100};
  for (uint32_t wc = 0; wc <= 100; ++wc)
    for (uint32_t wm = 0; wm <= 100; ++wm) {
      if (!wc && !wm) continue;
      const uint32_t rc = fit_weight_rcp(2 * wc), rm = fit_weight_rcp(2 * wm), rb = fit_weight_rcp(2 * (wc + wm));
      for (uint32_t tc : grid)
        for (uint32_t tm : grid) {
          // resource_allocation.go / requested_to_capacity_ratio.go in integers
          int64_t n = 0, d = 0;
          if (wc && tc > 0) n += (int64_t)tc * wc, d += wc;
          if (wm && tm > 0) n += (int64_t)tm * wm, d += wm;
          const int64_t want = d == 0 ? 0 : (2 * n + d) / (2 * d);
          const int64_t wantf = d == 0 ? 0 : std::llround((double)n / (double)d);
          const uint32_t got = fit_rtcr_node_score(tc, tm, wc, wm, rc, rm, rb);
          ++nscore;
          if ((int64_t)got != want || want != wantf) {
            if (bad++ < 10)
              printf("MISMATCH score tc=%u tm=%u wc=%u wm=%u got %u want %lld / %lld\n", tc, tm, wc, wm, got,
                     (long long)want, (long long)wantf);
          }
        }
    }
  // the issue's examples
  const uint32_t r2 = fit_weight_rcp(2), r4 = fit_weight_rcp(4);
  if (fit_rtcr_node_score(30, 45, 1, 1, r2, r2, r4) != 38 || fit_rtcr_node_score(100, 0, 1, 1, r2, r2, r4) != 100 ||
      fit_rtcr_node_score(0, 0, 1, 1, r2, r2, r4) != 0) {
    printf("MISMATCH examples\n");
    ++bad;
  }
  printf("checked %llu shapes, %llu divisions and %llu node scores, mismatches %llu\n", (unsigned long long)nshapes,
         (unsigned long long)ndiv, (unsigned long long)nscore, (unsigned long long)bad);
  return bad != 0;
}
