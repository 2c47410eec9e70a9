// ksched_forget.hpp — ks_batch_forget's host-only pieces: the
// check of the caller's index list and the per-batch record of the pods
// already taken back.  No HIP and nothing of the context: ksched_host.cpp
// includes it, and tools/forget_check.cpp runs it under ASan + UBSan.
#pragma once

#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace ks {

// One bit per pod of a batch: set by ks_batch_forget, cleared by the batch's
// next run (a run places every pod anew).
struct ForgetBits {
  std::vector<uint64_t> w;
  uint32_t n = 0;
  void reset(uint32_t pods) {
    n = pods;
    w.assign(((size_t)pods + 63) / 64, 0);
  }
  bool test(uint32_t i) const { return i < n && ((w[i >> 6] >> (i & 63)) & 1u) != 0; }
  void set(uint32_t i) {
    if (i < n) w[i >> 6] |= 1ull << (i & 63);
  }
  uint32_t count() const {
    uint32_t c = 0;
    for (uint64_t x : w) c += (uint32_t)__builtin_popcountll(x);
    return c;
  }
};

enum ForgetListError : uint32_t {
  FL_OK = 0,
  FL_RANGE,        // an index >= the batch's pod count
  FL_ORDER,        // not strictly increasing (a repeat or a descent)
  FL_UNSCHEDULED,  // the pod's result is not KS_POD_SCHEDULED
  FL_FORGOTTEN,    // forgotten already since the batch's last run
};
struct ForgetListCheck {
  ForgetListError err = FL_OK;
  uint32_t at = 0;  // position in the list of the first offender
};

// The whole list is checked before anything is applied; the first offending
// position wins (at one position: range, then order, then the pod's state).
// scheduled(i): pod i's result is KS_POD_SCHEDULED.
template <class Scheduled>
ForgetListCheck forget_check_list(const uint32_t *idx, uint32_t n, uint32_t npods, const ForgetBits &done,
                                  Scheduled scheduled) {
  for (uint32_t k = 0; k < n; ++k) {
    const uint32_t i = idx[k];
    if (i >= npods) return {FL_RANGE, k};
    if (k && i <= idx[k - 1]) return {FL_ORDER, k};
    if (!scheduled(i)) return {FL_UNSCHEDULED, k};
    if (done.test(i)) return {FL_FORGOTTEN, k};
  }
  return {};
}

// ks_last_error's text for a refused list.
inline std::string forget_list_message(const ForgetListCheck &r, const uint32_t *idx, uint32_t npods) {
  char buf[160];
  const uint32_t i = idx[r.at];
  switch (r.err) {
    case FL_RANGE:
      std::snprintf(buf, sizeof buf, "ks_batch_forget: idx[%u] = %u, the batch has %u pods", r.at, i, npods);
      break;
    case FL_ORDER:
      std::snprintf(buf, sizeof buf, "ks_batch_forget: idx[%u] = %u after %u: the list is not strictly increasing", r.at,
                    i, idx[r.at - 1]);
      break;
    case FL_UNSCHEDULED:
      std::snprintf(buf, sizeof buf, "ks_batch_forget: idx[%u] = %u: the pod was not scheduled", r.at, i);
      break;
    case FL_FORGOTTEN:
      std::snprintf(buf, sizeof buf, "ks_batch_forget: idx[%u] = %u: forgotten already since the batch ran", r.at, i);
      break;
    default: return "";
  }
  return buf;
}

}  // namespace ks
