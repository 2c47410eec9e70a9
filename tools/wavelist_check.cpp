// Wave-list check for the resource-only sweep's batch step (ksched_dev.hpp
// wl_fold / wl_merge / wl_entry): the list of one wave and pod,
// folded per lane segment and merged across segments as the kernel does it,
// against the sequential definition the per-pod reduction implemented:
//   B      = max over the lanes of b2
//   c_l    = b1_l > B ? b1_l : 0          (the candidates)
//   c1, c2 = the largest, then the next candidate, picked one at a time
//   bound  = max(B, the third candidate)
// for 64 lanes' pairs b1 >= b2, keys unique within the wave unless 0.
// Every segment width 1..64 dividing the wave runs on the constructed cases,
// widths 1, WL_SEG (the kernel's) and 64 on the random ones,
// with the segments' tuples combined in the kernel's exchange order (partner
// segment g ^ 1, g ^ 2, ...).  Cases: all pairs zero; one, two and three
// candidates; the wave's two best keys in one lane; ties at 0; keys at the
// 31-bit top; seeded random waves (dense, sparse, few distinct lanes).
// Build: g++ -O2 -std=c++17 -I include -I k8s-1m_amd/csrc tools/wavelist_check.cpp -o wavelist_check
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>

#include "ksched_dev.hpp"

using namespace ks;

struct Pair {
  uint32_t b1, b2;
};

// the definition, sequentially
static void reference(const Pair *p, uint32_t out[3]) {
  uint32_t B = 0;
  for (int l = 0; l < WAVE; ++l) B = std::max(B, p[l].b2);
  uint32_t c[WAVE];
  for (int l = 0; l < WAVE; ++l) c[l] = p[l].b1 > B ? p[l].b1 : 0u;
  uint32_t pick[3];
  for (int i = 0; i < 3; ++i) {
    uint32_t m = 0;
    for (int l = 0; l < WAVE; ++l) m = std::max(m, c[l]);
    pick[i] = m;
    if (m)
      for (int l = 0; l < WAVE; ++l)
        if (c[l] == m) c[l] = 0;
  }
  out[0] = pick[0];
  out[1] = pick[1];
  out[2] = std::max(B, pick[2]);
}

// the kernel's way with segments of `seg` lanes
static void batched(const Pair *p, int seg, uint32_t out[3]) {
  const int ns = WAVE / seg;
  WaveTuple t[WAVE], n[WAVE];
  for (int g = 0; g < ns; ++g) {
    WaveTuple w = {0u, 0u, 0u, 0u};
    for (int i = 0; i < seg; ++i) wl_fold(w, p[g * seg + i].b1, p[g * seg + i].b2);
    t[g] = w;
  }
  for (int m = 1; m < ns; m <<= 1) {  // every segment merges with its partner, as the lanes do
    for (int g = 0; g < ns; ++g) n[g] = wl_merge(t[g], t[g ^ m]);
    std::copy(n, n + ns, t);
  }
  for (uint32_t e = 0; e < 3; ++e) out[e] = wl_entry(t[0], e);
  for (int g = 1; g < ns; ++g)  // every lane ends with the pod's tuple
    for (uint32_t e = 0; e < 3; ++e)
      if (wl_entry(t[g], e) != out[e]) out[e] = 0xFFFFFFFFu;
}

static uint64_t n_checked = 0, n_bad = 0;

static void check(const Pair *p, bool every_width = true) {
  uint32_t want[3];
  reference(p, want);
  for (int seg = 1; seg <= WAVE; seg <<= 1) {
    if (!every_width && seg != 1 && seg != WL_SEG && seg != WAVE) continue;
    uint32_t got[3];
    batched(p, seg, got);
    ++n_checked;
    if (got[0] != want[0] || got[1] != want[1] || got[2] != want[2]) {
      if (n_bad < 10)
        printf("MISMATCH seg=%d want=(%u, %u, %u) got=(%u, %u, %u)\n", seg, want[0], want[1], want[2], got[0], got[1],
               got[2]);
      ++n_bad;
    }
  }
}

int main() {
  static_assert(WL_T * WL_SEG == WAVE, "a batch step's lanes");
  const uint32_t TOP = 0x7FFFFFFFu;
  Pair p[WAVE];
  auto clear = [&] {
    for (auto &x : p) x = {0u, 0u};
  };
  // all pairs zero
  clear();
  check(p);
  // one, two and three candidates, at every lane distance, low keys and the 31-bit top
  for (uint32_t hi : {100u, TOP})
    for (int a = 0; a < WAVE; ++a)
      for (int b = 0; b < WAVE; ++b)
        for (int c = 0; c < WAVE; c += 7) {
          clear();
          p[a].b1 = hi;
          check(p);
          if (b == a) continue;
          p[b].b1 = hi - 1;
          check(p);
          if (c == a || c == b) continue;
          p[c].b1 = hi - 2;
          check(p);
          // ... with seconds below, between and above them
          for (uint32_t s : {1u, hi - 3, hi - 2, hi - 1}) {
            p[a].b2 = std::min(s, hi - 1);
            check(p);
            p[a].b2 = 0;
            p[c].b2 = std::min(s, hi - 3);
            check(p);
            p[c].b2 = 0;
          }
        }
  // the wave's two best keys in one lane: b2 of a lane above every other lane's b1
  for (uint32_t hi : {1000u, TOP})
    for (int a = 0; a < WAVE; ++a)
      for (int b = 0; b < WAVE; ++b) {
        if (a == b) continue;
        clear();
        p[a] = {hi, hi - 1};
        p[b] = {hi - 2, 0u};
        check(p);
        p[b].b2 = hi - 5;
        check(p);
        p[(b + 1) % WAVE == a ? (b + 2) % WAVE : (b + 1) % WAVE].b1 = hi - 3;
        check(p);
      }
  // seeded random waves: unique non-zero keys, b1 >= b2, zeros mixed in
  std::mt19937_64 g(11);
  for (int it = 0; it < 2000000; ++it) {
    const int mode = it % 6;
    const uint32_t span = mode < 2 ? 200u : mode < 4 ? 1u << 20 : TOP;  // a narrow span crowds the ranks
    const uint32_t base = mode == 5 ? TOP - span + 1 : 1u;
    uint32_t used[2 * WAVE];
    int nu = 0;
    auto fresh = [&]() -> uint32_t {
      for (;;) {
        const uint32_t k = base + (uint32_t)(g() % span);
        if (std::find(used, used + nu, k) == used + nu) {
          used[nu++] = k;
          return k;
        }
      }
    };
    const uint32_t fill = (uint32_t)(g() % 101);  // share of lanes with a feasible node
    for (int l = 0; l < WAVE; ++l) {
      p[l] = {0u, 0u};
      if (g() % 100 >= fill) continue;
      uint32_t x = fresh(), y = (g() & 1) ? fresh() : 0u;
      if (y > x) std::swap(x, y);
      p[l] = {x, y};
    }
    check(p, false);
  }
  printf("checked %llu, mismatches %llu\n", (unsigned long long)n_checked, (unsigned long long)n_bad);
  return n_bad != 0;
}
