// Top-k check for ks_explain's selection (ksched_explain.hpp):
// the kernels' two levels run on the CPU with exactly the shared code -- the
// staging rank, the flush rule, the pad-and-sort merge, the (best, count)
// pairs -- one thread standing for the workgroup (no barrier), waves of 64
// lanes staged in the kernel's order, positions dealt to the blocks by the
// kernel's grid stride, then the blocks' lists through the same routine.
// Against std::partial_sort of the keys, descending, on: random key sets with
// and without infeasible positions; all-equal totals; totals strictly
// ascending and strictly descending with the slot; fewer keys than k; one
// position; sizes around the wave, the block and the second grid stride;
// k = 1, 2, 16, 64, 127 and 128.  The arrays are heap blocks of their exact
// size, so AddressSanitizer sees an index one past the staging buffer.
// Build: g++ -O1 -g -std=c++17 -fsanitize=address,undefined -I include -I k8s-1m_amd/csrc tools/topk_check.cpp -o topk_check
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <random>
#include <vector>

#include "ksched_explain.hpp"

using namespace ks;

constexpr uint32_t WAVE_LANES = 64, BLOCK_THREADS = TOPK_STEP, MAX_BLOCKS = 256;

// One workgroup's selection over the keys it is offered, `step` per step.
struct Block {
  std::vector<uint64_t> keys = std::vector<uint64_t>(TOPK_N, 0xDEADBEEFDEADBEEFull);  // (LDS is not zeroed either)
  uint32_t nstage = 0, staged = 0, k;
  uint64_t thr = 0;
  uint32_t merges = 0;
  bool overflow = false;
  explicit Block(uint32_t k_) : k(k_) {
    for (uint32_t i = 0; i < TOPK_LIST; ++i) keys[i] = 0;
  }
  void flush() {
    nstage = 0;
    topk_merge(keys.data(), staged, 0u, 1u, [] {});
    staged = 0;
    ++merges;
  }
  // the threads' keys of one step (at most BLOCK_THREADS; missing threads offer 0)
  void step(const uint64_t *in, uint32_t n) {
    for (uint32_t w = 0; w < BLOCK_THREADS / WAVE_LANES; ++w) {
      uint64_t lane_key[WAVE_LANES], mask = 0;
      for (uint32_t l = 0; l < WAVE_LANES; ++l) {
        const uint32_t t = w * WAVE_LANES + l;
        lane_key[l] = t < n ? in[t] : 0ull;
        if (lane_key[l] > thr) mask |= 1ull << l;
      }
      if (!mask) continue;
      const uint32_t base = nstage;
      nstage += (uint32_t)__builtin_popcountll(mask);
      for (uint32_t l = 0; l < WAVE_LANES; ++l)
        if (mask >> l & 1ull) {
          const uint32_t i = base + topk_lane_rank(mask, l);
          if (i >= TOPK_STAGE) overflow = true;  // the flush rule failed
          else keys[TOPK_LIST + i] = lane_key[l];
          ++staged;
        }
    }
    if (staged > TOPK_FLUSH) {
      flush();
      thr = keys[k - 1];
    }
  }
  void finish() {
    if (staged) flush();
  }
};

struct Answer {
  std::vector<uint64_t> keys;  // the k final keys (0: none)
  TopkBest best{0, 0};
  bool overflow = false;
  uint32_t merges = 0;
};

// The two kernels over `pos` (a position's key, 0: not feasible).
static Answer device_way(const std::vector<uint64_t> &pos, uint32_t k) {
  const uint32_t npos = (uint32_t)pos.size();
  const uint32_t blocks = std::max(1u, std::min((npos + BLOCK_THREADS - 1) / BLOCK_THREADS, MAX_BLOCKS));
  std::vector<uint64_t> lists((size_t)blocks * TOPK_LIST);
  Answer a;
  for (uint32_t b = 0; b < blocks; ++b) {
    Block blk(k);
    TopkBest best{0, 0};
    for (uint32_t base = b * BLOCK_THREADS; base < npos; base += blocks * BLOCK_THREADS) {
      const uint32_t n = std::min(BLOCK_THREADS, npos - base);
      for (uint32_t t = 0; t < n; ++t)
        if (pos[base + t]) best = topk_best_merge(best, TopkBest{topk_key_top(pos[base + t]), 1u});
      blk.step(&pos[base], n);
    }
    blk.finish();
    for (uint32_t i = 0; i < TOPK_LIST; ++i) lists[(size_t)b * TOPK_LIST + i] = blk.keys[i];
    a.best = topk_best_merge(a.best, best);
    a.overflow |= blk.overflow;
    a.merges += blk.merges;
  }
  // the merge level: the k-entry head of each block's list
  std::vector<uint64_t> heads((size_t)blocks * k);
  for (uint32_t i = 0; i < heads.size(); ++i) heads[i] = lists[(size_t)(i / k) * TOPK_LIST + i % k];
  Block m(k);
  for (uint32_t base = 0; base < heads.size(); base += BLOCK_THREADS)
    m.step(&heads[base], std::min<uint32_t>(BLOCK_THREADS, (uint32_t)heads.size() - base));
  m.finish();
  a.overflow |= m.overflow;
  a.keys.assign(m.keys.begin(), m.keys.begin() + k);
  return a;
}

static uint64_t mismatches = 0, cases = 0;

static void check(const char *what, const std::vector<uint64_t> &pos, uint32_t k) {
  ++cases;
  std::vector<uint64_t> want;
  for (uint64_t key : pos)
    if (key) want.push_back(key);
  const uint32_t m = (uint32_t)std::min<size_t>(k, want.size());
  std::partial_sort(want.begin(), want.begin() + m, want.end(), std::greater<uint64_t>());
  TopkBest wb{0, 0};
  if (m) {
    wb.top = topk_key_top(want[0]);
    for (uint64_t key : pos)
      if (key && topk_key_top(key) == wb.top) ++wb.count;
  }
  const Answer got = device_way(pos, k);
  bool ok = !got.overflow && got.best.top == wb.top && got.best.count == wb.count;
  for (uint32_t i = 0; i < k && ok; ++i) ok = got.keys[i] == (i < m ? want[i] : 0ull);
  if (!ok) {
    ++mismatches;
    std::printf("MISMATCH %s: n %zu k %u overflow %d best %u x %u (want %u x %u)\n", what, pos.size(), k,
                (int)got.overflow, got.best.top, got.best.count, wb.top, wb.count);
  }
}

int main() {
  // the key's fields
  if (topk_key_slot(topk_key(41, 7)) != 7 || topk_key_top(topk_key(41, 7)) != 42 ||
      !(topk_key(5, 3) > topk_key(5, 4)) || !(topk_key(6, 9) > topk_key(5, 0))) {
    std::printf("MISMATCH key fields\n");
    ++mismatches;
  }
  std::mt19937_64 rng(20261020);
  const uint32_t ks_[] = {1, 2, 16, 64, 127, 128};
  const uint32_t ns[] = {1, 2, 63, 64, 65, 127, 129, 1023, 1024, 1025, 2500, 5000, 270000};
  for (uint32_t n : ns)
    for (uint32_t k : ks_) {
      std::vector<uint64_t> pos(n);
      // every slot at one total: the k lowest slots, the tie set is every node
      for (uint32_t i = 0; i < n; ++i) pos[i] = topk_key(700, i);
      check("all equal", pos, k);
      // totals strictly ascending with the slot: every position displaces the list
      for (uint32_t i = 0; i < n; ++i) pos[i] = topk_key(i, i);
      check("ascending", pos, k);
      for (uint32_t i = 0; i < n; ++i) pos[i] = topk_key(n - i, i);
      check("descending", pos, k);
      // few distinct totals, a third of the positions infeasible
      for (uint32_t i = 0; i < n; ++i) pos[i] = rng() % 3 ? topk_key((int64_t)(rng() % 50), i) : 0ull;
      check("random, few totals", pos, k);
      for (uint32_t i = 0; i < n; ++i) pos[i] = topk_key((int64_t)(rng() % 7000000), i);
      check("random, wide totals", pos, k);
      // fewer keys than k: a handful of feasible positions, then none
      for (uint32_t i = 0; i < n; ++i) pos[i] = rng() % 97 == 0 && i % 5 == 0 ? topk_key((int64_t)(rng() % 9), i) : 0ull;
      check("sparse", pos, k);
      for (uint32_t i = 0; i < n; ++i) pos[i] = 0;
      check("none feasible", pos, k);
      // the best keys inside one wave of one block / in the last, partial wave / one per block
      for (uint32_t i = 0; i < n; ++i) pos[i] = topk_key(10, i);
      for (uint32_t w0 = n / 2 / 64 * 64, i = w0; i < w0 + 64 && i < n; ++i) pos[i] = topk_key(90, i);
      check("one wave", pos, k);
      for (uint32_t i = 0; i < n; ++i) pos[i] = topk_key(10, i);
      for (uint32_t i = (n - 1) / 64 * 64; i < n; ++i) pos[i] = topk_key(90, i);
      check("last wave", pos, k);
      for (uint32_t i = 0; i < n; ++i) pos[i] = topk_key(10 + (i % 1024 == 17 ? 80 : 0), i);
      check("one per block", pos, k);
    }
  // random sizes
  for (int it = 0; it < 300; ++it) {
    const uint32_t n = 1 + (uint32_t)(rng() % 6000), k = 1 + (uint32_t)(rng() % 128);
    const uint64_t spread = 1 + rng() % 5000;
    std::vector<uint64_t> pos(n);
    for (uint32_t i = 0; i < n; ++i) pos[i] = rng() % 4 ? topk_key((int64_t)(rng() % spread), i) : 0ull;
    check("random sizes", pos, k);
  }
  // a (best, count) merge with nothing on one side
  const TopkBest none{0, 0}, some{9, 3};
  if (topk_best_merge(none, none).count != 0 || topk_best_merge(none, some).count != 3 ||
      topk_best_merge(some, none).top != 9 || topk_best_merge(some, some).count != 6) {
    std::printf("MISMATCH best merge\n");
    ++mismatches;
  }
  std::printf("cases %llu mismatches %llu\n", (unsigned long long)cases, (unsigned long long)mismatches);
  return mismatches ? 1 : 0;
}
