// NodeResourcesBalancedAllocation over a list of resources (DESIGN.md §4,
// §5.12): upstream v1.31.3 balanced_allocation.go#balancedResourceScorer in
// IEEE binary64, one rounding per operation.  Plain C++ shared by the host
// runtime, the one-pod chain's kernels and tools/ba_check.cpp, which checks
// exactly this code on the CPU.  Every unit that includes it is built with
// -ffp-contract=off: the products and sums below are separate operations.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define KS_HD __host__ __device__
#else
#define KS_HD
#endif

namespace ks {

// The list in force as one launch sees it (SpreadArgs::bal_lo / bal_hi): the entries that
// take part for the pod, in list order, 4 bits each -- 0..7 the pod's record
// (XResDev) of a listed scalar resource it requests, BA_CPU, BA_MEM -- and
// their count in the top 4 bits.  A listed name the pod does not request, or
// one without a column, has no entry.  0: the default scorer.
constexpr uint32_t BA_MAX_LIST = 10;  // cpu, memory, MAX_XRES scalar names
constexpr uint32_t BA_CPU = 8, BA_MEM = 9;
constexpr int64_t BA_MAX_ALLOC = 1ll << 44;  // a listed resource's Allocatable stays below it (as cpu / memory)
KS_HD inline uint32_t ba_list_count(uint64_t bal) { return (uint32_t)(bal >> 60); }
KS_HD inline uint32_t ba_list_entry(uint64_t bal, uint32_t j) { return (uint32_t)(bal >> (4u * j)) & 15u; }
inline uint64_t ba_list_push(uint64_t bal, uint32_t code) {
  const uint32_t n = ba_list_count(bal);
  return (bal & ~(15ull << 60)) | ((uint64_t)code << (4u * n)) | ((uint64_t)(n + 1) << 60);
}

// RN(a / b) from y = RN(1 / b) (Markstein; ksched_eval.hpp div_rn).
KS_HD inline double ba_div_rn(double a, double b, double y) {
  const double q0 = a * y;
  const double r = __builtin_fma(-b, q0, a);
  return __builtin_fma(r, y, q0);
}

// A scalar resource's fraction min(req / alloc, 1), alloc != 0: the clamp is
// taken in int64 first (Requested may exceed Allocatable by any amount after
// ks_pods_add), so the value converted lies in [0, alloc], alloc < 2^44, both
// conversions are exact and the quotient is at most 1.  y = RN(1 / alloc).
KS_HD inline double ba_x_fraction(int64_t alloc, int64_t req, double y) {
  int64_t m = req < alloc ? req : alloc;
  m = m > 0 ? m : 0;
  return ba_div_rn((double)m, (double)alloc, y);
}
KS_HD inline double ba_x_fraction(int64_t alloc, int64_t req) { return ba_x_fraction(alloc, req, 1.0 / (double)alloc); }

// x / float64(n), n = 3..10 fractions: the IEEE quotient from RN(1 / n) (the
// literals are rounded by the compiler).
KS_HD inline double ba_rcp_n(uint32_t n) {
  const double rcp[BA_MAX_LIST + 1] = {0.0,       1.0,       1.0 / 2.0, 1.0 / 3.0, 1.0 / 4.0, 1.0 / 5.0,
                                       1.0 / 6.0, 1.0 / 7.0, 1.0 / 8.0, 1.0 / 9.0, 1.0 / 10.0};
  return rcp[n <= BA_MAX_LIST ? n : 0];
}
KS_HD inline double ba_div_n(double x, uint32_t n, double rcp_n) { return ba_div_rn(x, (double)n, rcp_n); }
KS_HD inline double ba_div_n(double x, uint32_t n) { return ba_div_n(x, n, ba_rcp_n(n)); }

// int64((1 - std) * 100)
KS_HD inline int32_t ba_score_of_std(double sd) { return (int32_t)((1.0 - sd) * 100.0); }

// The node's score.  frac(entry, &f) gives the fraction of one entry of the
// list, or false when the node's Allocatable of it is 0 (left out).  Fractions
// and totalFraction are accumulated in list order.  Zero or one fraction: std
// 0; two: |f0 - f1| / 2, upstream's shortcut (the general formula rounds
// differently); more: mean = total / n, sum += (f - mean)(f - mean) in list
// order, std = sqrt(sum / n).  The variance pass asks for the fractions again
// instead of keeping up to ten doubles alive: the filter kernels have no
// registers for them.
template <class F>
KS_HD inline int32_t ba_score_list(uint64_t bal, F &&frac) {
  const uint32_t cnt = ba_list_count(bal);
  double tot = 0.0, first = 0.0, last = 0.0;
  uint32_t n = 0;
  for (uint32_t j = 0; j < cnt; ++j) {
    double f;
    if (!frac(ba_list_entry(bal, j), f)) continue;
    if (!n) first = f;
    last = f;
    tot = tot + f;
    ++n;
  }
  double sd = 0.0;
  if (n == 2) {
    sd = std::fabs((first - last) * 0.5);  // (f0 - f1) / 2 is exact either way
  } else if (n > 2) {
    // the reciprocal of the list's own length is the same for every node (on
    // the device: a scalar); a node that leaves a resource out looks its own up
    const double yc = ba_rcp_n(cnt);
    const double yn = n == cnt ? yc : ba_rcp_n(n);
    const double mean = ba_div_n(tot, n, yn);
    double sum = 0.0;
    for (uint32_t j = 0; j < cnt; ++j) {
      double f;
      if (!frac(ba_list_entry(bal, j), f)) continue;
      const double d = f - mean;
      const double dd = d * d;
      sum = sum + dd;
    }
    // correctly rounded: libm's on the host; on the device the compiler's
    // lowering ends in the FMA-residual step (tests/test_gpu_ba.py's grid)
    sd = std::sqrt(ba_div_n(sum, n, yn));
  }
  return ba_score_of_std(sd);
}

}  // namespace ks
