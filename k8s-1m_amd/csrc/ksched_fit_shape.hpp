// NodeResourcesFit RequestedToCapacityRatio: the shape table and the node
// score's rounding divide.  Plain C++ shared by the host
// runtime, the kernels and tools/rtcr_check.cpp, which checks exactly this code
// on the CPU.
#pragma once
#include <cstdint>

#include "ksched.h"

#if defined(__HIPCC__)
#define KS_HD __host__ __device__
#else
#define KS_HD
#endif

namespace ks {

// a product of two factors below 2^24: on the device v_mul_u32_u24 (full rate;
// as asm for the reason given at ksched_eval.hpp's wmul)
KS_HD inline uint32_t fit_mul24(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint32_t r;
  asm("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
#else
  return a * b;
#endif
}

constexpr uint32_t FIT_SHAPE_MAX_POINTS = 101;  // strictly increasing utilisations in 0..100
constexpr uint32_t FIT_TABLE_N = 101;           // T[u], u = 0..100
constexpr uint32_t FIT_TABLE_WORDS = 32;        // its device / LDS copy: 128 bytes, the tail repeats T[100]

// ceil(2^31 / d): floor(n / d) == (2 n x rcp) >> 32 while n x d < 2^31
KS_HD inline uint32_t fit_weight_rcp(uint32_t d) {
  return d ? (uint32_t)(((1ull << 31) + d - 1) / d) : 0u;
}

// helper.BuildBrokenLinearFunction over every utilisation it can be asked:
// T[p] = raw(p) with the scores x 10 (MaxNodeScore / MaxCustomPriorityScore)
// and Go's int64 division, which truncates toward zero (a falling segment has a
// negative numerator; C++'s / truncates the same way).  false: not a valid
// shape (null, empty, more than 101 points, a utilisation outside 0..100 or
// not strictly increasing, a score outside 0..10).
inline bool fit_shape_table(const ks_fit_shape_point *pts, uint32_t n, uint8_t out[FIT_TABLE_N]) {
  if (!pts || !out || n == 0 || n > FIT_SHAPE_MAX_POINTS) return false;
  for (uint32_t i = 0; i < n; ++i) {
    if (pts[i].utilization < 0 || pts[i].utilization > 100 || pts[i].score < 0 || pts[i].score > 10) return false;
    if (i && pts[i].utilization <= pts[i - 1].utilization) return false;
  }
  uint32_t i = 0;
  for (int64_t p = 0; p <= 100; ++p) {
    while (i < n && p > pts[i].utilization) ++i;  // the first point with p <= x_i
    int64_t v;
    if (i == n) {
      v = (int64_t)pts[n - 1].score * 10;
    } else if (i == 0) {
      v = (int64_t)pts[0].score * 10;
    } else {
      const int64_t x0 = pts[i - 1].utilization, x1 = pts[i].utilization;
      const int64_t y0 = (int64_t)pts[i - 1].score * 10, y1 = (int64_t)pts[i].score * 10;
      v = y0 + (y1 - y0) * (p - x0) / (x1 - x0);
    }
    out[p] = (uint8_t)v;  // between y0 and y1: 0..100
  }
  return true;
}

// The node score from the two resources' shape scores tc, tm (0 for a
// resource whose Allocatable is zero): n = wc tc + wm tm and d = the summed
// weight of the resources whose score is positive; math.Round(n / d) =
// floor((2 n + d) / (2 d)) by the reciprocal multiply with divisor 2 d:
// rcp_cpu / rcp_mem / rcp_both = fit_weight_rcp(2 wc), (2 wm), (2 (wc + wm)).
// A weight of 0 (not listed) needs no test: its term of n and of d is 0, and
// where both scores are 0 the numerator is.  2 n + d <= 40,200, 2 d <= 400.
KS_HD inline uint32_t fit_rtcr_node_score(uint32_t tc, uint32_t tm, uint32_t wc, uint32_t wm, uint32_t rcp_cpu,
                                          uint32_t rcp_mem, uint32_t rcp_both) {
  const uint32_t n = fit_mul24(wc, tc) + fit_mul24(wm, tm);
  const uint32_t d = (tc ? wc : 0u) + (tm ? wm : 0u);
  const uint32_t rcp = tc ? (tm ? rcp_both : rcp_cpu) : rcp_mem;
  return (uint32_t)(((uint64_t)((2u * n + d) << 1) * rcp) >> 32);
}

// ---- listed extended (scalar) resources -------------------
// The one-FMA floor's epsilon (ksched_eval.hpp LA_EPS).
constexpr double FIT_X_EPS = 0x1p-45;
constexpr int64_t FIT_X_MAX_CAP = 1ll << 44;  // a listed resource's Allocatable stays below it (as cpu / memory)

// One listed scalar resource's score from its int64 columns: cap =
// Allocatable, req = Requested + the pod's request (Requested, not
// NonZeroRequested).  most: min(req, cap) * 100 / cap, else
// max(cap - req, 0) * 100 / cap, int64 truncation.  The clamp is taken in
// int64 first -- Requested may exceed Allocatable by any amount after
// ks_pods_add -- so the value converted lies in [0, cap], cap < 2^44, its
// hundredfold is exact and the floor is fit_resource's: y = RN(1 / cap), one
// FMA, truncation.  cap == 0 -> 0 (the caller leaves the resource out).
// Checked by tools/xfit_check.cpp.
KS_HD inline uint32_t fit_x_score(bool most, int64_t cap, int64_t req) {
  int64_t m = req < cap ? req : cap;  // min(req, cap)
  m = m > 0 ? m : 0;
  const int64_t v = most ? m : cap - m;  // in [0, cap]
  const double y = cap ? 1.0 / (double)cap : 0.0;
  const double q = __builtin_fma((double)v * 100.0, y, FIT_X_EPS);
  return (uint32_t)q;  // 0 <= q < 101
}

// Sum of weight x score (n) and of the weights that count (d) over the
// resources of one node: at most 10 resources of weight <= 100 and score <=
// 100, so n <= 100,000 and d <= 1,000.
struct FitXSum {
  uint32_t n, d;
};
// LeastAllocated / MostAllocated: the resource counts when its Allocatable is non-zero.
KS_HD inline void fit_x_add(FitXSum &s, uint32_t w, uint32_t score, bool has_cap) {
  s.n += fit_mul24(w, score);
  s.d += has_cap ? w : 0u;
}
// RequestedToCapacityRatio: t = T[utilisation], 0 for a zero Allocatable; the
// resource counts when t is positive.
KS_HD inline void fit_x_add_rtcr(FitXSum &s, uint32_t w, uint32_t t) {
  s.n += fit_mul24(w, t);
  s.d += t ? w : 0u;
}
// floor(n / d) by the reciprocal multiply, rcp = fit_weight_rcp(d): exact while
// n x d < 2^31 (here <= 10^8).  d == 0 has rcp == 0 -> 0.
KS_HD inline uint32_t fit_x_div(uint32_t n, uint32_t rcp) { return (uint32_t)(((uint64_t)(n << 1) * rcp) >> 32); }
// math.Round(n / d) = floor((2 n + d) / (2 d)): d varies per node over the
// subsets of the listed resources, so this one is a 32-bit division (the
// one-pod chain runs it once per feasible node); 2 n + d <= 201,000.
KS_HD inline uint32_t fit_x_round_div(uint32_t n, uint32_t d) { return d ? (2u * n + d) / (2u * d) : 0u; }

}  // namespace ks
