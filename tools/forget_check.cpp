// ks_batch_forget's host bookkeeping (csrc/ksched_forget.hpp) on the CPU: the
// check of the caller's index list and the per-batch record of forgotten pods,
// against a plain re-statement of the rules, under AddressSanitizer + UBSan.
//   * constructed lists: empty; one pod; every refusal (range, repeat, descent,
//     unscheduled, forgotten already) alone and behind valid indices, at the
//     first, a middle and the last position; the first offender wins;
//   * batch sizes around the bitmap's word edges (0, 1, 63, 64, 65, 127, 128,
//     129, 4097): first / last pod, reset after a run, indices beyond the end;
//   * seeded random lists against the re-statement, with the bitmap following
//     the accepted ones (a batch's life: runs, forgets, runs).
// Build and run (host only, no HIP):
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
//     -I k8s-1m_amd/csrc tools/forget_check.cpp -o forget_check && ./forget_check
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "ksched_forget.hpp"

using namespace ks;

static int failures = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    if (!(cond)) {                                                    \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

// the rules, restated without the bitmap
static ForgetListCheck reference(const std::vector<uint32_t> &idx, uint32_t npods, const std::set<uint32_t> &done,
                                 const std::vector<uint8_t> &sched) {
  for (uint32_t k = 0; k < idx.size(); ++k) {
    const uint32_t i = idx[k];
    if (i >= npods) return {FL_RANGE, k};
    if (k && i <= idx[k - 1]) return {FL_ORDER, k};
    if (!sched[i]) return {FL_UNSCHEDULED, k};
    if (done.count(i)) return {FL_FORGOTTEN, k};
  }
  return {};
}

static ForgetListCheck run(const std::vector<uint32_t> &idx, uint32_t npods, const ForgetBits &done,
                           const std::vector<uint8_t> &sched) {
  // a list of its own size on the heap: a read past its end is ASan's to find
  uint32_t *copy = idx.empty() ? nullptr : new uint32_t[idx.size()];
  std::copy(idx.begin(), idx.end(), copy);
  const ForgetListCheck r =
      forget_check_list(copy, (uint32_t)idx.size(), npods, done, [&](uint32_t i) { return sched.at(i) != 0; });
  if (r.err) {
    const std::string msg = forget_list_message(r, copy, npods);
    CHECK(!msg.empty() && msg.size() < 160);
  }
  delete[] copy;
  return r;
}

static bool same(const ForgetListCheck &a, const ForgetListCheck &b) { return a.err == b.err && (!a.err || a.at == b.at); }

static void constructed() {
  const uint32_t n = 10;
  std::vector<uint8_t> sched(n, 1);
  sched[4] = 0;
  ForgetBits done;
  done.reset(n);
  done.set(7);
  CHECK(run({}, n, done, sched).err == FL_OK);
  CHECK(run({}, 0, ForgetBits(), {}).err == FL_OK);
  CHECK(run({0}, n, done, sched).err == FL_OK);
  CHECK(run({0, 1, 2, 3, 5, 6, 8, 9}, n, done, sched).err == FL_OK);
  struct Case {
    std::vector<uint32_t> idx;
    ForgetListError err;
    uint32_t at;
  };
  const Case cases[] = {
      {{10}, FL_RANGE, 0},          {{0, 10}, FL_RANGE, 1},      {{0, 1, 0xFFFFFFFFu}, FL_RANGE, 2},
      {{1, 1}, FL_ORDER, 1},        {{3, 2}, FL_ORDER, 1},       {{0, 2, 2, 3}, FL_ORDER, 2},
      {{0, 1, 2, 1}, FL_ORDER, 3},  {{4}, FL_UNSCHEDULED, 0},    {{0, 4, 5}, FL_UNSCHEDULED, 1},
      {{7}, FL_FORGOTTEN, 0},       {{5, 6, 7}, FL_FORGOTTEN, 2},
      // the first offender wins, whatever follows
      {{4, 7, 3, 10}, FL_UNSCHEDULED, 0}, {{0, 7, 4, 12}, FL_FORGOTTEN, 1}, {{9, 10, 4}, FL_RANGE, 1},
      // at one position: range before order before the pod's state
      {{5, 12}, FL_RANGE, 1},       {{8, 7}, FL_ORDER, 1},       {{5, 4}, FL_ORDER, 1},
  };
  for (const Case &c : cases) {
    const ForgetListCheck r = run(c.idx, n, done, sched);
    CHECK(r.err == c.err && r.at == c.at);
  }
  // a batch of no pods refuses every index
  CHECK(run({0}, 0, ForgetBits(), {}).err == FL_RANGE);
}

static void bitmap_edges() {
  for (uint32_t n : {0u, 1u, 63u, 64u, 65u, 127u, 128u, 129u, 4097u}) {
    ForgetBits b;
    b.reset(n);
    CHECK(b.count() == 0 && b.w.size() == ((size_t)n + 63) / 64);
    CHECK(!b.test(0) && !b.test(n) && !b.test(n + 1) && !b.test(0xFFFFFFFFu));
    b.set(n);            // beyond the end: ignored
    b.set(0xFFFFFFFFu);
    CHECK(b.count() == 0);
    if (!n) continue;
    b.set(0);
    b.set(n - 1);
    b.set(n - 1);  // twice: still one bit
    CHECK(b.test(0) && b.test(n - 1) && b.count() == (n == 1 ? 1u : 2u));
    if (n > 2) CHECK(!b.test(1) && !b.test(n - 2));
    for (uint32_t i = 0; i < n; ++i) b.set(i);
    CHECK(b.count() == n);
    b.reset(n);  // the batch ran again
    CHECK(b.count() == 0 && !b.test(0) && !b.test(n - 1));
    b.reset(n / 2);  // the pooled batch reused for a smaller one
    CHECK(b.n == n / 2 && !b.test(n / 2));
  }
}

static void random_lives(uint32_t seed) {
  std::mt19937 rng(seed);
  for (int life = 0; life < 200; ++life) {
    const uint32_t n = 1 + rng() % 300;
    std::vector<uint8_t> sched(n);
    for (auto &s : sched) s = rng() % 8 != 0;
    ForgetBits bits;
    std::set<uint32_t> done;
    bits.reset(n);
    for (int call = 0; call < 12; ++call) {
      if (rng() % 6 == 0) {  // the batch runs again
        bits.reset(n);
        done.clear();
        for (auto &s : sched) s = rng() % 8 != 0;
      }
      std::vector<uint32_t> idx;
      const uint32_t want = rng() % (n + 2);
      for (uint32_t i = 0; i < n && idx.size() < want; ++i)
        if (rng() % 3 == 0 && (rng() % 16 == 0 || (sched[i] && !done.count(i)))) idx.push_back(i);
      // now and then a fault of each kind
      const uint32_t fault = rng() % 10;
      if (fault == 0) idx.push_back(n + rng() % 3);
      if (fault == 1 && idx.size() > 1) std::swap(idx[rng() % idx.size()], idx[rng() % idx.size()]);
      if (fault == 2 && !idx.empty()) idx.insert(idx.begin() + rng() % idx.size(), idx[rng() % idx.size()]);
      const ForgetListCheck got = run(idx, n, bits, sched), want_r = reference(idx, n, done, sched);
      CHECK(same(got, want_r));
      if (!got.err)
        for (uint32_t i : idx) {
          bits.set(i);
          done.insert(i);
        }
      CHECK(bits.count() == done.size());
      for (uint32_t i = 0; i < n; ++i) CHECK(bits.test(i) == (done.count(i) != 0));
    }
  }
}

int main() {
  constructed();
  bitmap_edges();
  for (uint32_t seed = 1; seed <= 5; ++seed) random_lives(seed);
  if (failures) {
    std::printf("forget_check: %d failures\n", failures);
    return 1;
  }
  std::printf("forget_check: ok\n");
  return 0;
}
