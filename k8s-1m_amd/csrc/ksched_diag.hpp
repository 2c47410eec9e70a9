// ksched_diag.hpp — ks_diagnose: the record the diagnose pass
// (ksched_diag.hip) fills, upstream's reason strings, and the host code that
// turns the record into ks_reason rows and FitError.Error()'s text.  The host
// part is plain C++ over the C ABI's structs: tools/diag_msg_check.cpp
// compiles it without HIP.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ksched.h"

namespace ks {

// ------------------------------------------------------------ reason table
// Upstream v1.31.3's status reasons, transcribed (parity is unpinned, DESIGN
// §7): one line each, so a correction is a one-line change.
constexpr const char *REASON_UNSCHEDULABLE = "node(s) were unschedulable";
constexpr const char *REASON_NODE_NAME = "node(s) didn't match the requested node name";
constexpr const char *REASON_TAINT_FMT = "node(s) had untolerated taint {%s: %s}";
constexpr const char *REASON_AFFINITY = "node(s) didn't match Pod's node affinity/selector";
constexpr const char *REASON_AFFINITY_CONFLICT = "pod affinity terms conflict";
constexpr const char *REASON_PREFILTER_RESULT = "node is filtered out by the prefilter result";
constexpr const char *REASON_NODE_PORTS = "node(s) didn't have free ports for the requested pod ports";
constexpr const char *REASON_TOO_MANY_PODS = "Too many pods";
constexpr const char *REASON_INSUFFICIENT_CPU = "Insufficient cpu";
constexpr const char *REASON_INSUFFICIENT_MEMORY = "Insufficient memory";
constexpr const char *REASON_INSUFFICIENT_FMT = "Insufficient %s";  // ephemeral-storage, scalar resources
constexpr const char *REASON_SPREAD_LABEL = "node(s) didn't match pod topology spread constraints (missing required label)";
constexpr const char *REASON_SPREAD_SKEW = "node(s) didn't match pod topology spread constraints";
constexpr const char *REASON_IPA_AFFINITY = "node(s) didn't match pod affinity rules";
constexpr const char *REASON_IPA_ANTI = "node(s) didn't match pod anti-affinity rules";
constexpr const char *REASON_IPA_EXISTING = "node(s) didn't satisfy existing pods anti-affinity rules";

// ------------------------------------------------------------ device record
// A present node's status as one mask: exactly one of the bits DG_UNSCHED ..
// DG_FEASIBLE (its first failing plugin, or none), and under DG_FIT every
// reason NodeResourcesFit gives (fitsRequest collects them all).
enum DiagBit : uint32_t {
  DG_UNSCHED = 0,      // NodeUnschedulable
  DG_NODE_NAME = 1,    // NodeName
  DG_TAINT = 2,        // TaintToleration (the taint: DiagRec::taint or the multi-taint list)
  DG_AFFINITY = 3,     // NodeAffinity (Filter, or PreFilter's conflict)
  DG_FIT = 4,          // NodeResourcesFit
  DG_SPREAD_LABEL = 5, // PodTopologySpread: the node lacks a DoNotSchedule key
  DG_SPREAD_SKEW = 6,  // ... skew above maxSkew
  DG_IPA_AFF = 7,      // InterPodAffinity: satisfyPodAffinity
  DG_IPA_ANTI = 8,     // ... satisfyPodAntiAffinity
  DG_IPA_EXIST = 9,    // ... satisfyExistingPodsAntiAffinity
  DG_PREFILTERED = 10, // outside the PreFilterResult
  DG_PORTS = 11,       // NodePorts
  DG_FEASIBLE = 12,
  DG_FIT_PODS = 13,    // Too many pods
  DG_FIT_CPU = 14,
  DG_FIT_MEM = 15,
  DG_FIT_X = 16,       // + extended-resource column (0 .. 7)
  DG_BITS = 24,
};
constexpr int DIAG_TAINT_BINS = 64;  // hard-taint dictionary bits (63 in use)
struct DiagRec {
  uint32_t cnt[32];                  // nodes per DiagBit
  uint32_t taint[DIAG_TAINT_BINS];   // nodes whose only untolerated taint is this dictionary bit
  uint32_t n_multi;                  // nodes with several untolerated taints: their slots are listed
  uint32_t _pad[3];
};
static_assert(sizeof(DiagRec) == 400, "DiagRec layout");

// ------------------------------------------------------------------- host
struct DiagRow {
  uint32_t plugin, count;
  std::string reason;
};
// Names the context resolves for a record: the "{key: value}" reason of every
// hard-taint dictionary bit and the name of every extended-resource column.
struct DiagNames {
  std::string taint[DIAG_TAINT_BINS];
  std::string xres[8];
};

inline std::string diag_taint_reason(const std::string &key, const std::string &value) {
  std::string s(64 + key.size() + value.size(), '\0');
  const int n = snprintf(&s[0], s.size(), REASON_TAINT_FMT, key.c_str(), value.c_str());
  s.resize((size_t)n);
  return s;
}
inline std::string diag_insufficient(const std::string &name) {
  std::string s(32 + name.size(), '\0');
  const int n = snprintf(&s[0], s.size(), REASON_INSUFFICIENT_FMT, name.c_str());
  s.resize((size_t)n);
  return s;
}

// The record (rec.taint holding the listed nodes too, resolved by the caller)
// as reason rows: one per reason string with a non-zero count, in plugin
// order; two dictionary bits with one string (a taint under NoSchedule and
// NoExecute) give one row.  `conflict`: NodeAffinity's PreFilter rejected the
// pod, so DG_AFFINITY carries the conflict reason.
inline void diag_rows(const DiagRec &rec, const DiagNames &nm, bool conflict, std::vector<DiagRow> *out) {
  out->clear();
  auto add = [&](uint32_t plugin, uint32_t count, const std::string &reason) {
    if (!count) return;
    for (DiagRow &r : *out)
      if (r.plugin == plugin && r.reason == reason) {
        r.count += count;
        return;
      }
    out->push_back(DiagRow{plugin, count, reason});
  };
  add(KS_PLUGIN_NODE_UNSCHEDULABLE, rec.cnt[DG_UNSCHED], REASON_UNSCHEDULABLE);
  add(KS_PLUGIN_NODE_NAME, rec.cnt[DG_NODE_NAME], REASON_NODE_NAME);
  for (int b = 0; b < DIAG_TAINT_BINS; ++b) add(KS_PLUGIN_TAINT_TOLERATION, rec.taint[b], nm.taint[b]);
  add(KS_PLUGIN_NODE_AFFINITY, rec.cnt[DG_AFFINITY], conflict ? REASON_AFFINITY_CONFLICT : REASON_AFFINITY);
  add(KS_FAIL_PREFILTER_RESULT, rec.cnt[DG_PREFILTERED], REASON_PREFILTER_RESULT);
  add(KS_STATUS_NODE_PORTS, rec.cnt[DG_PORTS], REASON_NODE_PORTS);
  add(KS_PLUGIN_NODE_RESOURCES_FIT, rec.cnt[DG_FIT_PODS], REASON_TOO_MANY_PODS);
  add(KS_PLUGIN_NODE_RESOURCES_FIT, rec.cnt[DG_FIT_CPU], REASON_INSUFFICIENT_CPU);
  add(KS_PLUGIN_NODE_RESOURCES_FIT, rec.cnt[DG_FIT_MEM], REASON_INSUFFICIENT_MEMORY);
  for (int x = 0; x < 8; ++x) add(KS_PLUGIN_NODE_RESOURCES_FIT, rec.cnt[DG_FIT_X + x], diag_insufficient(nm.xres[x]));
  add(KS_PLUGIN_POD_TOPOLOGY_SPREAD, rec.cnt[DG_SPREAD_LABEL], REASON_SPREAD_LABEL);
  add(KS_PLUGIN_POD_TOPOLOGY_SPREAD, rec.cnt[DG_SPREAD_SKEW], REASON_SPREAD_SKEW);
  add(KS_PLUGIN_INTER_POD_AFFINITY, rec.cnt[DG_IPA_AFF], REASON_IPA_AFFINITY);
  add(KS_PLUGIN_INTER_POD_AFFINITY, rec.cnt[DG_IPA_ANTI], REASON_IPA_ANTI);
  add(KS_PLUGIN_INTER_POD_AFFINITY, rec.cnt[DG_IPA_EXIST], REASON_IPA_EXISTING);
}

// The record's first-failure counts as ks_diagnosis carries them.
inline void diag_counts(const DiagRec &rec, ks_diagnosis *d) {
  const uint32_t *c = rec.cnt;
  d->feasible_nodes = c[DG_FEASIBLE];
  d->plugin_nodes[KS_PLUGIN_NODE_UNSCHEDULABLE] = c[DG_UNSCHED];
  d->plugin_nodes[KS_PLUGIN_NODE_NAME] = c[DG_NODE_NAME];
  d->plugin_nodes[KS_PLUGIN_TAINT_TOLERATION] = c[DG_TAINT];
  d->plugin_nodes[KS_PLUGIN_NODE_AFFINITY] = c[DG_AFFINITY];
  d->plugin_nodes[KS_PLUGIN_NODE_RESOURCES_FIT] = c[DG_FIT];
  d->plugin_nodes[KS_PLUGIN_POD_TOPOLOGY_SPREAD] = c[DG_SPREAD_LABEL] + c[DG_SPREAD_SKEW];
  d->plugin_nodes[KS_PLUGIN_INTER_POD_AFFINITY] = c[DG_IPA_AFF] + c[DG_IPA_ANTI] + c[DG_IPA_EXIST];
  d->plugin_nodes[KS_FAIL_PREFILTER_RESULT] = c[DG_PREFILTERED];
  d->node_ports_nodes = c[DG_PORTS];
}

// FitError.Error() without the PostFilter part: "0/N nodes are available:",
// then " <prefilter_msg>." or the reasons' histogram -- equal strings merged,
// "<count> <reason>" sorted bytewise (sort.Strings), joined by ", ".
inline ks_status fit_error_message(uint32_t num_all_nodes, const char *prefilter_msg, const ks_reason *reasons,
                                   uint32_t n, char *buf, size_t cap, size_t *len) {
  if (!len || (n && !reasons) || (cap && !buf)) return KS_ERR_INVALID;
  for (uint32_t i = 0; i < n; ++i)
    if (!reasons[i].reason) return KS_ERR_INVALID;
  std::string msg = "0/" + std::to_string(num_all_nodes) + " nodes are available:";
  if (prefilter_msg && prefilter_msg[0]) {
    msg += " " + std::string(prefilter_msg) + ".";
  } else {
    std::vector<std::pair<std::string, uint64_t>> hist;
    for (uint32_t i = 0; i < n; ++i) {
      auto it = std::find_if(hist.begin(), hist.end(),
                             [&](const std::pair<std::string, uint64_t> &h) { return h.first == reasons[i].reason; });
      if (it == hist.end()) hist.emplace_back(reasons[i].reason, reasons[i].count);
      else it->second += reasons[i].count;
    }
    std::vector<std::string> parts;
    for (auto &h : hist) parts.push_back(std::to_string(h.second) + " " + h.first);
    std::sort(parts.begin(), parts.end());  // std::string compares as unsigned bytes, as Go's strings
    for (size_t i = 0; i < parts.size(); ++i) msg += (i ? ", " : " ") + parts[i];
    if (!parts.empty()) msg += ".";
  }
  *len = msg.size();
  if (cap < msg.size() + 1) return KS_ERR_INVALID;  // *len set: the caller sizes its buffer (+ the terminator)
  std::copy(msg.begin(), msg.end(), buf);
  buf[msg.size()] = '\0';
  return KS_OK;
}

}  // namespace ks
