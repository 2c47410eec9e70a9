// diag_msg_check.cpp — the host half of ks_diagnose on its own (DESIGN.md
// §5.15): ksched_diag.hpp's DiagRec -> reason rows assembly and FitError's
// text, as plain C++ with no HIP and no context, so that it can be built with
// -fsanitize=address,undefined and run stand-alone:
//
//   g++ -std=c++17 -fsanitize=address,undefined -Iinclude -Ik8s-1m_amd/csrc tools/diag_msg_check.cpp -o diag_msg_check
//
// Prints "mismatches N" and exits non-zero when N > 0.
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "ksched_diag.hpp"

using namespace ks;

static int bad = 0;
#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      ++bad;                                                  \
      std::printf("line %d: %s\n", __LINE__, #x);             \
    }                                                         \
  } while (0)

static std::string message(uint32_t n_all, const char *pm, const std::vector<ks_reason> &r, ks_status *st = nullptr) {
  size_t len = 0;
  ks_status s = fit_error_message(n_all, pm, r.data(), (uint32_t)r.size(), nullptr, 0, &len);
  CHECK(s == KS_ERR_INVALID);  // the sizing call
  std::vector<char> buf(len + 1, '#');  // exactly what the call asks for: a write past it is the sanitizer's to find
  size_t len2 = 0;
  s = fit_error_message(n_all, pm, r.data(), (uint32_t)r.size(), buf.data(), buf.size(), &len2);
  if (st) *st = s;
  CHECK(s == KS_OK && len2 == len && buf[len] == '\0');
  return std::string(buf.data());
}

// the definition, restated: merge, format, sort as strings, join
static std::string expect(uint32_t n_all, const std::vector<ks_reason> &r) {
  std::vector<std::pair<std::string, unsigned long long>> h;
  for (auto &x : r) {
    bool seen = false;
    for (auto &e : h)
      if (e.first == x.reason) {
        e.second += x.count;
        seen = true;
      }
    if (!seen) h.push_back({x.reason, x.count});
  }
  std::vector<std::string> parts;
  for (auto &e : h) parts.push_back(std::to_string(e.second) + " " + e.first);
  for (size_t i = 0; i < parts.size(); ++i)  // insertion sort by unsigned bytes
    for (size_t j = i; j > 0 && std::memcmp(parts[j].c_str(), parts[j - 1].c_str(),
                                            std::min(parts[j].size(), parts[j - 1].size()) + 1) < 0; --j)
      std::swap(parts[j], parts[j - 1]);
  std::string s = "0/" + std::to_string(n_all) + " nodes are available:";
  for (size_t i = 0; i < parts.size(); ++i) s += (i ? ", " : " ") + parts[i];
  if (!parts.empty()) s += ".";
  return s;
}

int main() {
  // ---- the formatter
  {
    std::vector<ks_reason> r = {{4, 12, REASON_INSUFFICIENT_MEMORY},
                                {2, 3, "node(s) had untolerated taint {dedicated: infra}"},
                                {4, 999985, REASON_INSUFFICIENT_CPU}};
    CHECK(message(1000000, nullptr, r) ==
          "0/1000000 nodes are available: 12 Insufficient memory, 3 node(s) had untolerated taint {dedicated: infra}, "
          "999985 Insufficient cpu.");
    r = {{4, 2, REASON_INSUFFICIENT_MEMORY}, {4, 10, REASON_INSUFFICIENT_CPU}};
    CHECK(message(12, nullptr, r) == "0/12 nodes are available: 10 Insufficient cpu, 2 Insufficient memory.");
    r = {{4, 6, "x"}, {4, 2, "y"}, {4, 5, "x"}};
    CHECK(message(13, nullptr, r) == "0/13 nodes are available: 11 x, 2 y.");
    CHECK(message(7, nullptr, {}) == "0/7 nodes are available:");
    CHECK(message(5, REASON_AFFINITY_CONFLICT, r) == "0/5 nodes are available: pod affinity terms conflict.");
    size_t len = 0;
    char small[8] = "keepme";
    CHECK(fit_error_message(5, nullptr, r.data(), 3, small, sizeof small, &len) == KS_ERR_INVALID && len > 8);
    CHECK(std::strcmp(small, "keepme") == 0);
    CHECK(fit_error_message(5, nullptr, r.data(), 3, small, sizeof small, nullptr) == KS_ERR_INVALID);
    CHECK(fit_error_message(5, nullptr, nullptr, 3, small, sizeof small, &len) == KS_ERR_INVALID);
    CHECK(fit_error_message(5, nullptr, r.data(), 3, nullptr, 8, &len) == KS_ERR_INVALID);
    ks_reason null_reason{0, 1, nullptr};
    CHECK(fit_error_message(5, nullptr, &null_reason, 1, small, sizeof small, &len) == KS_ERR_INVALID);
  }
  // random histograms against the restated definition (counts up to 2^32 - 1: the merged sums need 64 bits)
  {
    std::mt19937 rng(20261020);
    const char *names[] = {"Insufficient cpu", "Insufficient memory", "Too many pods", "a", "a b", "A", "10", "~"};
    for (int it = 0; it < 2000; ++it) {
      std::vector<ks_reason> r;
      const int n = (int)(rng() % 9);
      for (int i = 0; i < n; ++i) {
        const uint32_t c = (rng() & 3) ? rng() % 120 : rng();
        r.push_back({(uint32_t)(rng() % 9), c, names[rng() % 8]});
      }
      const uint32_t n_all = rng();
      CHECK(message(n_all, nullptr, r) == expect(n_all, r));
    }
  }
  // ---- DiagRec -> rows
  {
    DiagNames nm;
    nm.taint[0] = diag_taint_reason("dedicated", "infra");
    nm.taint[5] = diag_taint_reason("dedicated", "infra");  // the same key and value under the other effect
    nm.taint[62] = diag_taint_reason("k", "");
    nm.xres[0] = "ephemeral-storage";
    nm.xres[7] = "amd.com/gpu";
    CHECK(nm.taint[0] == "node(s) had untolerated taint {dedicated: infra}");
    CHECK(nm.taint[62] == "node(s) had untolerated taint {k: }");
    CHECK(diag_insufficient("amd.com/gpu") == "Insufficient amd.com/gpu");
    DiagRec rec{};
    std::vector<DiagRow> rows;
    diag_rows(rec, nm, false, &rows);
    CHECK(rows.empty());
    rec.cnt[DG_UNSCHED] = 1;
    rec.cnt[DG_NODE_NAME] = 2;
    rec.cnt[DG_TAINT] = 3 + 4 + 9;
    rec.taint[0] = 3;
    rec.taint[5] = 4;
    rec.taint[62] = 9;
    rec.cnt[DG_AFFINITY] = 5;
    rec.cnt[DG_PREFILTERED] = 6;
    rec.cnt[DG_PORTS] = 7;
    rec.cnt[DG_FIT] = 10;
    rec.cnt[DG_FIT_PODS] = 10;
    rec.cnt[DG_FIT_CPU] = 8;
    rec.cnt[DG_FIT_MEM] = 0;
    rec.cnt[DG_FIT_X + 0] = 1;
    rec.cnt[DG_FIT_X + 7] = 2;
    rec.cnt[DG_SPREAD_LABEL] = 11;
    rec.cnt[DG_SPREAD_SKEW] = 12;
    rec.cnt[DG_IPA_AFF] = 13;
    rec.cnt[DG_IPA_ANTI] = 14;
    rec.cnt[DG_IPA_EXIST] = 15;
    rec.cnt[DG_FEASIBLE] = 16;
    diag_rows(rec, nm, false, &rows);
    auto count_of = [&](uint32_t plugin, const std::string &reason) {
      uint32_t c = 0, hits = 0;
      for (auto &r : rows)
        if (r.plugin == plugin && r.reason == reason) {
          c = r.count;
          ++hits;
        }
      CHECK(hits <= 1);
      return c;
    };
    CHECK(rows.size() == 16);
    CHECK(count_of(KS_PLUGIN_NODE_UNSCHEDULABLE, REASON_UNSCHEDULABLE) == 1);
    CHECK(count_of(KS_PLUGIN_NODE_NAME, REASON_NODE_NAME) == 2);
    CHECK(count_of(KS_PLUGIN_TAINT_TOLERATION, nm.taint[0]) == 7);  // two bits, one string, one row
    CHECK(count_of(KS_PLUGIN_TAINT_TOLERATION, nm.taint[62]) == 9);
    CHECK(count_of(KS_PLUGIN_NODE_AFFINITY, REASON_AFFINITY) == 5);
    CHECK(count_of(KS_FAIL_PREFILTER_RESULT, REASON_PREFILTER_RESULT) == 6);
    CHECK(count_of(KS_STATUS_NODE_PORTS, REASON_NODE_PORTS) == 7);
    CHECK(count_of(KS_PLUGIN_NODE_RESOURCES_FIT, REASON_TOO_MANY_PODS) == 10);
    CHECK(count_of(KS_PLUGIN_NODE_RESOURCES_FIT, REASON_INSUFFICIENT_CPU) == 8);
    CHECK(count_of(KS_PLUGIN_NODE_RESOURCES_FIT, REASON_INSUFFICIENT_MEMORY) == 0);
    CHECK(count_of(KS_PLUGIN_NODE_RESOURCES_FIT, "Insufficient ephemeral-storage") == 1);
    CHECK(count_of(KS_PLUGIN_NODE_RESOURCES_FIT, "Insufficient amd.com/gpu") == 2);
    CHECK(count_of(KS_PLUGIN_POD_TOPOLOGY_SPREAD, REASON_SPREAD_LABEL) == 11);
    CHECK(count_of(KS_PLUGIN_POD_TOPOLOGY_SPREAD, REASON_SPREAD_SKEW) == 12);
    CHECK(count_of(KS_PLUGIN_INTER_POD_AFFINITY, REASON_IPA_AFFINITY) == 13);
    CHECK(count_of(KS_PLUGIN_INTER_POD_AFFINITY, REASON_IPA_ANTI) == 14);
    CHECK(count_of(KS_PLUGIN_INTER_POD_AFFINITY, REASON_IPA_EXISTING) == 15);
    ks_diagnosis d{};
    diag_counts(rec, &d);
    const uint32_t want[KS_NUM_FAIL_COUNTS] = {1, 2, 16, 5, 10, 23, 42, 6};
    for (int k = 0; k < KS_NUM_FAIL_COUNTS; ++k) CHECK(d.plugin_nodes[k] == want[k]);
    CHECK(d.node_ports_nodes == 7 && d.feasible_nodes == 16);
    // every plugin but NodeResourcesFit: its reasons' counts sum to its first-failure count
    uint32_t sum[16] = {};
    for (auto &r : rows) sum[r.plugin] += r.count;
    for (int k = 0; k < KS_NUM_FAIL_COUNTS; ++k)
      if (k != KS_PLUGIN_NODE_RESOURCES_FIT) CHECK(sum[k] == d.plugin_nodes[k]);
    CHECK(sum[KS_PLUGIN_NODE_RESOURCES_FIT] >= d.plugin_nodes[KS_PLUGIN_NODE_RESOURCES_FIT]);
    CHECK(sum[KS_STATUS_NODE_PORTS] == d.node_ports_nodes);
    // the PreFilter conflict: NodeAffinity's row carries the conflict reason
    DiagRec cf{};
    cf.cnt[DG_AFFINITY] = 9;
    diag_rows(cf, nm, true, &rows);
    CHECK(rows.size() == 1 && rows[0].reason == REASON_AFFINITY_CONFLICT && rows[0].count == 9);
    // rows -> message
    diag_rows(rec, nm, false, &rows);
    std::vector<ks_reason> kr;
    for (auto &r : rows) kr.push_back({r.plugin, r.count, r.reason.c_str()});
    CHECK(message(161, nullptr, kr) == expect(161, kr));
  }
  std::printf("mismatches %d\n", bad);
  return bad ? 1 : 0;
}
