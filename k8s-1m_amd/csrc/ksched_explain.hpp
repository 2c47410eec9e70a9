// ksched_explain.hpp — ks_explain: the k best packed keys of
// a stream of keys, kept by one workgroup in LDS, and the record the explain
// kernels (ksched_explain.hip) fill.  The selection is plain C++ over an array
// and a barrier the caller supplies, shared by the kernels (the array in LDS,
// the barrier __syncthreads) and tools/topk_check.cpp, which runs exactly this
// code on the CPU (one thread, no barrier) against std::partial_sort.
//
// A workgroup holds TOPK_N keys: its list, the TOPK_LIST best so far in
// descending order, then a staging buffer.  Each step every thread offers one
// key (0: none); a wave ballots the lanes whose key beats the list's k-th and
// compacts them into the staging buffer by a prefix count.  When another step
// might overflow the buffer, and once at the end, the workgroup pads the used
// part of the array to a power of two with zeros and sorts it descending by a
// bitonic network: the list is again its first TOPK_LIST entries.  Keys are
// unique (they carry the slot), 0 is no key, and a key that left the list
// never returns, so nothing is ever counted twice.
#pragma once

#include <stdint.h>

#include "ksched.h"

#if defined(__HIPCC__)
#define KS_HD __host__ __device__
#else
#define KS_HD
#endif

namespace ks {

constexpr uint32_t TOPK_LIST = KS_EXPLAIN_MAX_CANDIDATES;  // the list: always this long, the caller's k reads its head
constexpr uint32_t TOPK_N = 2048;                          // list + staging buffer (16 KiB of LDS)
constexpr uint32_t TOPK_STAGE = TOPK_N - TOPK_LIST;
constexpr uint32_t TOPK_STEP = 1024;                       // keys one step can stage: a workgroup's threads
constexpr uint32_t TOPK_FLUSH = TOPK_STAGE - TOPK_STEP;    // staged keys above which the next step could overflow
static_assert((TOPK_N & (TOPK_N - 1)) == 0 && (TOPK_LIST & (TOPK_LIST - 1)) == 0 && TOPK_STAGE >= TOPK_STEP,
              "a power-of-two array that holds the list and one full step");

// The packed key (ksched_eval.hpp pack_key): TotalScore descending, then slot ascending.
KS_HD inline uint64_t topk_key(int64_t total, uint32_t slot) {
  return ((uint64_t)(total + 1) << 32) | (uint64_t)(0xFFFFFFFFu - slot);
}
KS_HD inline uint32_t topk_key_slot(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }
KS_HD inline uint32_t topk_key_top(uint64_t key) { return (uint32_t)(key >> 32); }  // TotalScore + 1 (0: no key)

// A lane's place among its wave's staged lanes (mask: the ballot).
KS_HD inline uint32_t topk_lane_rank(uint64_t mask, uint32_t lane) {
  return (uint32_t)__builtin_popcountll(mask & ((1ull << lane) - 1ull));
}

// Entries the sort runs over with `staged` keys in the buffer.
KS_HD inline uint32_t topk_sort_size(uint32_t staged) {
  uint32_t n = 2 * TOPK_LIST;
  while (n < TOPK_LIST + staged) n <<= 1;
  return n;
}

// Compare-exchange i (< n / 2) of the bitonic network's stage (size, stride);
// the exchanges of one stage touch disjoint pairs.  After the stage size == n
// the array is descending.
KS_HD inline void topk_cx(uint64_t *keys, uint32_t size, uint32_t stride, uint32_t i) {
  const uint32_t lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
  const uint64_t x = keys[lo], y = keys[hi];
  const bool desc = (lo & size) == 0;
  if (desc ? x < y : x > y) {
    keys[lo] = y;
    keys[hi] = x;
  }
}

// The list and `staged` (<= TOPK_STAGE) staged keys merged: keys[0 ..
// TOPK_LIST) is the new list.  Thread `tid` of `nth`; sync() is their barrier,
// reached by every thread the same number of times (staged is uniform).  The
// caller's barrier before the call has made the staged keys visible.
template <class Sync>
KS_HD inline void topk_merge(uint64_t *keys, uint32_t staged, uint32_t tid, uint32_t nth, Sync sync) {
  const uint32_t n = topk_sort_size(staged);
  for (uint32_t i = TOPK_LIST + staged + tid; i < n; i += nth) keys[i] = 0;
  sync();
  for (uint32_t size = 2; size <= n; size <<= 1)
    for (uint32_t stride = size >> 1; stride; stride >>= 1) {
      for (uint32_t i = tid; i < n / 2; i += nth) topk_cx(keys, size, stride, i);
      sync();
    }
}

// The best TotalScore and the number of keys at it (selectHost's tie set).
struct TopkBest {
  uint32_t top;    // TotalScore + 1 (0: no key)
  uint32_t count;
};
KS_HD inline TopkBest topk_best_merge(TopkBest a, TopkBest b) {
  if (a.top == b.top) return TopkBest{a.top, a.top ? a.count + b.count : 0u};
  return a.top > b.top ? a : b;
}

// ------------------------------------------------------------ device record
// What ks_explain copies back: 24 + 64 k bytes.
struct ExplainRec {
  uint32_t feasible, n_candidates, top_count, _pad;
  int64_t top_score;
};
struct ExplainOut {
  ExplainRec rec;
  ks_candidate cand[KS_EXPLAIN_MAX_CANDIDATES];
};
static_assert(sizeof(ExplainRec) == 24 && sizeof(ks_candidate) == 64 &&
                  sizeof(ExplainOut) == 24 + 64 * KS_EXPLAIN_MAX_CANDIDATES,
              "ks_explain's record");

}  // namespace ks
