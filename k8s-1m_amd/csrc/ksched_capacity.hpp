// ksched_capacity.hpp — ks_capacity: how many more replicas
// of a pod the cluster holds.  The exact capped quotient the capacity passes
// (ksched_capacity.hip) compute per (pod, node, resource), the pod-side
// constants the call uploads beside the PodDev, and the record a pass fills.
// The quotient is plain C++ for host and device: tools/capacity_check.cpp
// compiles it without HIP and runs it over the edge grid.
#pragma once

#include <stdint.h>

#include "ksched_fit_shape.hpp"  // KS_HD

namespace ks {

// min(floor(free / req), cap) for free >= 0, req >= 1, 0 <= cap <= 2^31, exact.
// rcp is RN(1 / RN(req)), computed once per pod on the host.
//
// With Q = free / req the product g = RN(RN(free) rcp) carries three roundings
// and the reciprocal's own: |g - Q| <= Q e with e < 2^-50 (four relative
// errors of at most 2^-53 each and their cross terms).
//   g >= cap + 2:  Q >= g / (1 + e) > (cap + 2)(1 - e) > cap + 1 as cap + 2 <=
//                  2^31 + 2, so floor(Q) > cap and the answer is cap: the
//                  quotient need not be known.
//   g <  cap + 2:  Q < (cap + 2) / (1 - e) < 2^32, so |g - Q| < 2^-18 and
//                  t = trunc(g) is floor(Q) - 1, floor(Q) or floor(Q) + 1.
//                  t <= cap + 1 < 2^32 fits 32 bits and t req <= (floor(Q) +
//                  1) req <= free + req < 2^64, so the product below does not
//                  wrap in 64 unsigned bits; one compare on each side
//                  (t req <= free < (t + 1) req) settles which of the three.
KS_HD inline uint32_t cap_quot(int64_t free, int64_t req, double rcp, uint32_t cap) {
  const uint64_t f = (uint64_t)free, r = (uint64_t)req;
  const double g = (double)free * rcp;
  if (g >= (double)cap + 2.0) return cap;
  uint64_t t = (uint64_t)(uint32_t)g;  // g in [0, 2^31 + 2]: the conversion is exact truncation
  const uint64_t pr = t * r;
  if (pr > f) t -= 1;               // t >= 1 here; (t - 1) req <= free by the bound above
  else if (f - pr >= r) t += 1;
  return t < (uint64_t)cap ? (uint32_t)t : cap;
}

// The same for cpu and memory, whose free value (< 2^44) the node row already
// holds as an exact binary64.
KS_HD inline uint32_t cap_quot_d(int64_t free, double free_d, int64_t req, double rcp, uint32_t cap) {
  const uint64_t f = (uint64_t)free, r = (uint64_t)req;
  const double g = free_d * rcp;
  if (g >= (double)cap + 2.0) return cap;
  uint64_t t = (uint64_t)(uint32_t)g;
  const uint64_t pr = t * r;
  if (pr > f) t -= 1;
  else if (f - pr >= r) t += 1;
  return t < (uint64_t)cap ? (uint32_t)t : cap;
}

// A node's free pod slots are an int32 difference: at most 2^31 - 1, so a cap
// one above a count (a tie told from a larger quotient) stays within 2^31.
constexpr uint32_t CAP_MAX_SLOTS = 0x7FFFFFFFu;

// Binding terms, in tie order (ksched.h KS_CAP_*): the first term that attains
// the minimum binds a node.
enum CapTerm : uint32_t { CAP_PODS = 0, CAP_CPU = 1, CAP_MEM = 2, CAP_PORTS = 3, CAP_X = 4, CAP_TERMS = 12 };

// Pod-side constants of a capacity call, one per distinct pod beside its
// PodDev: the reciprocals of its requests (0 where the request is 0; rcp_x by
// record of the one-pod program).
struct alignas(16) CapPod {
  double rcp_cpu, rcp_mem;
  double rcp_x[8];
};
static_assert(sizeof(CapPod) == 80, "CapPod layout");

// What a pass adds up for one pod over the present nodes.
struct alignas(16) CapRec {
  unsigned long long replicas;  // sum of c_i
  uint32_t eligible, room;      // nodes passing the static filters; of those, c_i >= 1
  uint32_t max_per_node;
  uint32_t bound[CAP_TERMS];    // eligible nodes per binding term
  uint32_t _pad[3];
};
static_assert(sizeof(CapRec) == 80, "CapRec layout");

}  // namespace ks
