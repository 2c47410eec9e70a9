// Exactness check for NodeResourcesBalancedAllocation over a list of resources
// (k8s-1m_amd/csrc/ksched_ba.hpp).  It includes the
// header the host runtime and the kernels compile, so what is checked is the
// product's sequence -- the reciprocal, div_rn, the divides by n -- against
// upstream's plain float64 operations (balanced_allocation.go): `/` and sqrt.
//
// (1) ba_x_fraction, one scalar resource's fraction from its int64 columns,
//     against min(float64(req) / float64(alloc), 1): every Allocatable 1..1200
//     with every requested 0..2 alloc; every power of two below 2^44 and its
//     neighbours and 200,000 random ones, with requested 0, alloc, beyond it up
//     to int64's end, and random values.
// (2) ba_div_n against x / float64(n), n = 3..10: sums of up to ten fractions,
//     their squared deviations, and random doubles over 120 binades.
// (3) the node score, ba_score_list against the plain restatement: every grid
//     of 3 and of 4 fractions k/c for c <= 12 in every order (the grid holds
//     every permutation), all-equal fractions k/c for c <= 64 and n = 3..10,
//     1,000,000 random lists of 3..10 fractions, lists with one or two
//     fractions (the shortcut), and the known answers of DESIGN.md §5.12.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -I k8s-1m_amd/csrc tools/ba_check.cpp -o ba_check
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "ksched_ba.hpp"

using ks::ba_div_n;
using ks::ba_list_push;
using ks::ba_score_list;
using ks::ba_x_fraction;

static uint64_t bad = 0, nfrac = 0, ndiv = 0, nscore = 0;

// ---- upstream, in plain float64
static double want_fraction(int64_t alloc, int64_t req) {
  const double f = (double)req / (double)alloc;
  return f > 1.0 ? 1.0 : f;
}
static int64_t want_score(const std::vector<double> &f) {
  double tot = 0.0;
  for (double v : f) tot += v;
  double sd = 0.0;
  const size_t n = f.size();
  if (n == 2) {
    sd = std::fabs((f[0] - f[1]) / 2.0);
  } else if (n > 2) {
    const double mean = tot / (double)n;
    double sum = 0.0;
    for (double v : f) sum = sum + (v - mean) * (v - mean);
    sd = std::sqrt(sum / (double)n);
  }
  return (int64_t)((1.0 - sd) * 100.0);
}

static void check_fraction(int64_t alloc, int64_t req) {
  ++nfrac;
  const double got = ba_x_fraction(alloc, req), want = want_fraction(alloc, req);
  if (got != want && bad++ < 10)
    printf("MISMATCH fraction alloc=%lld req=%lld got %.17g want %.17g\n", (long long)alloc, (long long)req, got, want);
}
static void check_alloc(int64_t alloc, std::mt19937_64 &g) {
  const int64_t reqs[] = {0, 1, alloc - 1, alloc, alloc + 1, 2 * alloc, INT64_MAX, INT64_MAX - alloc, alloc / 3, alloc / 7};
  for (int64_t r : reqs)
    if (r >= 0) check_fraction(alloc, r);
  for (int i = 0; i < 8; ++i) check_fraction(alloc, (int64_t)(g() % (uint64_t)(2 * alloc + 1)));
}

static void check_div(double x) {
  for (uint32_t n = 3; n <= 10; ++n) {
    ++ndiv;
    const double got = ba_div_n(x, n), want = x / (double)n;
    if (got != want && bad++ < 10) printf("MISMATCH divide x=%.17g n=%u got %.17g want %.17g\n", x, n, got, want);
  }
}

// One node: fractions num[i] / den[i] in list order (den 0: the resource is
// left out).  The product's side sees int64 columns, as the kernels do.
static int64_t check_score(const std::vector<int64_t> &num, const std::vector<int64_t> &den) {
  uint64_t bal = 0;
  for (size_t i = 0; i < num.size(); ++i) bal = ba_list_push(bal, (uint32_t)i);
  const int32_t got = ba_score_list(bal, [&](uint32_t e, double &f) {
    if (den[e] == 0) return false;
    f = ba_x_fraction(den[e], num[e]);
    return true;
  });
  std::vector<double> f;
  for (size_t i = 0; i < num.size(); ++i)
    if (den[i]) f.push_back(want_fraction(den[i], num[i]));
  const int64_t want = want_score(f);
  ++nscore;
  // the mean and the variance's divide see operands the grids reach
  if (f.size() > 2) {
    double tot = 0.0;
    for (double v : f) tot += v;
    check_div(tot);
    const double mean = tot / (double)f.size();
    double sum = 0.0;
    for (double v : f) sum = sum + (v - mean) * (v - mean);
    check_div(sum);
  }
  if ((int64_t)got != want && bad++ < 10) {
    printf("MISMATCH score got %d want %lld:", got, (long long)want);
    for (size_t i = 0; i < num.size(); ++i) printf(" %lld/%lld", (long long)num[i], (long long)den[i]);
    printf("\n");
  }
  return got;
}
static void known(const std::vector<int64_t> &num, int64_t den, int64_t want) {
  if (check_score(num, std::vector<int64_t>(num.size(), den)) != want) {
    ++bad;
    printf("MISMATCH known answer: want %lld\n", (long long)want);
  }
}

int main() {
  std::mt19937_64 g(29);
  // (1)
  for (int64_t alloc = 1; alloc <= 1200; ++alloc)
    for (int64_t req = 0; req <= 2 * alloc; ++req) check_fraction(alloc, req);
  for (int b = 0; b < 44; ++b)
    for (int64_t e = -1; e <= 1; ++e) {
      const int64_t alloc = (1ll << b) + e;
      if (alloc >= 1 && alloc < ks::BA_MAX_ALLOC) check_alloc(alloc, g);
    }
  check_alloc(ks::BA_MAX_ALLOC - 1, g);
  for (int i = 0; i < 200000; ++i) {
    const int bits = 1 + (int)(g() % 44);
    check_alloc((int64_t)(g() % ((1ull << bits) - 1)) + 1, g);
  }

  // (2) beyond the operands check_score feeds in
  check_div(0.0);
  for (int i = 0; i < 2000000; ++i) {
    const double m = 1.0 + (double)(g() >> 11) * 0x1p-53;  // [1, 2)
    check_div(std::ldexp(m, -(int)(g() % 120) + 4));        // 2^-115 .. 2^5
  }

  // (3) known answers
  known({25, 75, 50}, 100, 79);
  known({0, 0, 1}, 1, 52);
  known({25, 25, 75, 75}, 100, 75);
  for (int64_t k = 0; k <= 10; ++k) known({k, k, k}, 10, k == 7 || k == 8 ? 99 : 100);
  known({0, 1, 4, 9}, 10, 65);
  known({4, 9, 0, 1}, 10, 64);
  known({1, 8}, 10, (int64_t)((1.0 - std::fabs((0.1 - 0.8) / 2.0)) * 100.0));  // the shortcut's value
  known({3}, 10, 100);
  known({}, 10, 100);
  if (check_score({1, 1, 8}, {10, 0, 10}) != check_score({1, 8}, {10, 10})) {  // a zero Allocatable leaves two: the shortcut
    ++bad;
    printf("MISMATCH two fractions beside a zero Allocatable\n");
  }
  // grids of 3 and 4 fractions k / c
  for (int64_t c = 1; c <= 12; ++c) {
    const std::vector<int64_t> d3(3, c), d4(4, c);
    for (int64_t k0 = 0; k0 <= c; ++k0)
      for (int64_t k1 = 0; k1 <= c; ++k1)
        for (int64_t k2 = 0; k2 <= c; ++k2) {
          check_score({k0, k1, k2}, d3);
          for (int64_t k3 = 0; k3 <= c; ++k3) check_score({k0, k1, k2, k3}, d4);
        }
  }
  // all-equal fractions: the rounded mean may differ from them
  for (int64_t c = 1; c <= 64; ++c)
    for (int64_t k = 0; k <= c; ++k)
      for (size_t n = 3; n <= 10; ++n) check_score(std::vector<int64_t>(n, k), std::vector<int64_t>(n, c));
  // random lists: mixed denominators, requested beyond Allocatable, zero Allocatable
  for (int i = 0; i < 1000000; ++i) {
    const size_t n = 1 + (size_t)(g() % 10);
    std::vector<int64_t> num(n), den(n);
    for (size_t j = 0; j < n; ++j) {
      const int bits = 1 + (int)(g() % 44);
      den[j] = g() % 16 == 0 ? 0 : (int64_t)(g() % ((1ull << bits) - 1)) + 1;
      num[j] = den[j] ? (int64_t)(g() % (uint64_t)(den[j] + den[j] / 8 + 1)) : 3;
    }
    check_score(num, den);
  }
  printf("checked %llu fractions, %llu divisions by n and %llu node scores, mismatches %llu\n", (unsigned long long)nfrac,
         (unsigned long long)ndiv, (unsigned long long)nscore, (unsigned long long)bad);
  return bad != 0;
}
