// ksched_spread_dev.hpp — device helpers of the one-pod chain's node passes
// (ksched_spread.hip) that the diagnose pass (ksched_diag.hip) shares: the
// pod's staged program, a position's loads, the InterPodAffinity views, the
// wave reductions and the accumulator totals.  Internal linkage: each unit
// compiles its own copies.
#pragma once

#include <hip/hip_runtime.h>

#include "ksched_ba.hpp"
#include "ksched_dev.hpp"
#include "ksched_eval.hpp"
#include "ksched_kernels.hpp"
#include "ksched_util.hpp"

namespace ks {

namespace {

constexpr int SP_THREADS = 1024;  // few fat blocks (at most SPREAD_MAX_BLOCKS): one partial record each
constexpr uint32_t SP_LDS = 4096;     // LDS domain-histogram entries per block
constexpr uint32_t SP_LDS_DOM = 1024; // keys with at most this many domains aggregate in LDS
constexpr uint32_t SP_OFF_NONE = 0xFFFFFFFFu;
constexpr int8_t SST_FEASIBLE = -1, SST_EMPTY = -2, SST_IGNORED = -3;  // per-position status
constexpr int SP_BATCH = 4;           // positions per thread per step of the score / select passes

// The pod's one-pod-path program (ksched_dev.hpp SoloHdr): SpreadDev, XResDev, ImageDev records.
__device__ __forceinline__ const SoloHdr &solo_hdr(const SpreadArgs &a, const PodDev &p) {
  return *reinterpret_cast<const SoloHdr *>(a.clauses + p.solo_off);
}
__device__ __forceinline__ const SpreadDev *spread_recs(const SpreadArgs &a, const PodDev &p) {
  return reinterpret_cast<const SpreadDev *>(&solo_hdr(a, p) + 1);
}
__device__ __forceinline__ uint32_t spread_count(const SpreadArgs &a, const PodDev &p) { return solo_hdr(a, p).n_spread; }
__device__ __forceinline__ const XResDev *xres_recs(const SpreadArgs &a, const PodDev &p) {
  return reinterpret_cast<const XResDev *>(spread_recs(a, p) + solo_hdr(a, p).n_spread);
}
__device__ __forceinline__ const ImageDev *image_recs(const SpreadArgs &a, const PodDev &p) {
  return reinterpret_cast<const ImageDev *>(xres_recs(a, p) + solo_hdr(a, p).n_xres);
}
__device__ __forceinline__ const AffDev *aff_recs(const SpreadArgs &a, const PodDev &p) {
  return reinterpret_cast<const AffDev *>(image_recs(a, p) + solo_hdr(a, p).n_img);
}
// SPL_XFIT: the strategy's weight of an extended-resource column (0: not listed)
__device__ __forceinline__ uint32_t xfit_weight(const SpreadArgs &a, uint32_t col) {
  return (uint32_t)(a.xw >> (8u * (col & (MAX_XRES - 1)))) & 0xFFu;
}
// RequestedToCapacityRatio's staged shape table (null under the other strategies, which read none)
template <int GF>
__device__ __forceinline__ const uint8_t *fit_table_bytes() {
  if constexpr (GF == 2) return (const uint8_t *)fit_table_lds();
  else return nullptr;
}
// SPL_BAL: NodeResourcesBalancedAllocation over the list in force (a.bal_lo / bal_hi:
// the entries that take part for this pod, in list order; ksched_ba.hpp).  cpu
// and memory are score_ba's fractions; a listed scalar resource's come from
// its two columns at the pod's record, the values the fit check compared.  The
// list's order is not the records', and ba_score_list asks for every fraction
// twice; the filter instances have no registers for ten doubles, so the filter
// pass keeps the fractions of the pod's first BA_KEEP records from its fit
// check (xf0, xf1; negative: the node's Allocatable is 0) -- one listed
// resource, the common case, then costs no second load and one reciprocal --
// and the fractions of further records are computed from a second read of the
// two columns, once per pass.  The dump (KEPT false) reads them all again.
constexpr uint32_t BA_KEEP = 2;
__device__ __forceinline__ uint32_t ba_listed_records(const SpreadArgs &a) {
  const uint64_t bal = (uint64_t)a.bal_hi << 32 | a.bal_lo;
  uint32_t m = 0;
  for (uint32_t j = 0; j < ba_list_count(bal); ++j) m |= 1u << ba_list_entry(bal, j);
  return m & ((1u << MAX_XRES) - 1u);
}
template <bool KEPT>
__device__ __forceinline__ int32_t score_ba_list(const SpreadArgs &a, const PodDev &p, const NodeRegs &r,
                                                 const XResDev *xr, uint32_t pos, double xf0 = 0.0, double xf1 = 0.0) {
  return ba_score_list((uint64_t)a.bal_hi << 32 | a.bal_lo, [&](uint32_t e, double &f) {
    if (e == BA_CPU) {
      if (r.inv_cpu == 0.0) return false;
      f = fmin(div_rn(r.rcpu + p.req_cpu_d, r.acpu_d, r.inv_cpu), 1.0);
      return true;
    }
    if (e == BA_MEM) {
      if (r.inv_mem == 0.0) return false;
      f = fmin(div_rn(r.rmem + p.req_mem_d, r.amem_d, r.inv_mem), 1.0);
      return true;
    }
    if constexpr (KEPT) {
      if (e < BA_KEEP) {
        f = e ? xf1 : xf0;
        return f >= 0.0;
      }
    }
    const XResDev &x = xr[e & (MAX_XRES - 1)];
    const size_t ix = (size_t)(x.col & (MAX_XRES - 1)) * a.npos + pos;
    const int64_t xa = a.xalloc[ix];
    if (xa == 0) return false;
    f = ba_x_fraction(xa, (int64_t)((uint64_t)a.xreq[ix] + (uint64_t)x.req));
    return true;
  });
}
// Count column of an InterPodAffinity record at a position.
__device__ __forceinline__ uint32_t aff_count(const SpreadArgs &a, const AffDev &r, uint32_t pos) {
  return ((r.kind & AF_TERM) ? a.tcnt : a.cnt)[(size_t)r.col * a.npos + pos];
}
constexpr uint64_t IPA_BIAS = 1ull << 63;  // signed raw scores as unsigned min / max keys

// interpodaffinity Filter over the prefilter domain counts: every required
// affinity key present and its domain holding a pod that matches all the
// required affinity terms (unless no such pod exists anywhere and the pod
// matches its own terms), no required anti-affinity match in the node's
// domains, no bound pod's required anti-affinity term matching the pod there.
// Domain sum of record r at a position whose domain is d (!= DOM_NONE).
// The filter pass's view of the records at one position: domain sums of the
// low-cardinality records staged in LDS (aoff: segment per record or
// SP_OFF_NONE), the first AF_PF records' domain ids and per-node counts
// loaded with the position's other inputs.
constexpr int AF_PF = 4;
struct AffView {
  const uint32_t *aoff, *lds;
  uint32_t dm[AF_PF], nc[AF_PF];
};
__device__ __forceinline__ uint32_t aff_dom(const SpreadArgs &a, const AffDev *ad, const AffView &v, uint32_t r,
                                            uint32_t pos) {
  if (r >= (uint32_t)AF_PF) return a.dom[(size_t)ad[r].key * a.npos + pos];
  uint32_t d = v.dm[0];
#pragma unroll
  for (int k = 1; k < AF_PF; ++k) d = r == (uint32_t)k ? v.dm[k] : d;
  return d;
}
__device__ __forceinline__ uint32_t aff_sum(const SpreadArgs &a, const AffDev *ad, const AffView &v, uint32_t r,
                                            uint32_t pos, uint32_t d) {
  const AffDev &q = ad[r];
  if (q.kind & AF_NODE) {
    if (r >= (uint32_t)AF_PF) return aff_count(a, q, pos);
    uint32_t c = v.nc[0];
#pragma unroll
    for (int k = 1; k < AF_PF; ++k) c = r == (uint32_t)k ? v.nc[k] : c;
    return c;
  }
  const uint32_t o = v.aoff[r];
  return o != SP_OFF_NONE ? v.lds[o + d] : a.adcnt[(size_t)r * a.dom_cap + d];
}
__device__ __forceinline__ void aff_prefetch(const SpreadArgs &a, const AffDev *ad, uint32_t na, uint32_t pos,
                                             AffView &v) {
#pragma unroll
  for (int r = 0; r < AF_PF; ++r) {
    v.dm[r] = (uint32_t)r < na ? a.dom[(size_t)ad[r].key * a.npos + pos] : DOM_NONE;
    v.nc[r] = (uint32_t)r < na && (ad[r].kind & AF_NODE) ? aff_count(a, ad[r], pos) : 0u;
  }
}

__device__ __forceinline__ bool ipa_fits(const SpreadArgs &a, const AffDev *ad, uint32_t na, const AffView &v,
                                         uint32_t pos, bool first_ok) {
  bool has_req = false, exist = true;
  for (uint32_t r = 0; r < na; ++r) {
    const uint32_t kind = ad[r].kind & AF_KIND;
    if (kind > AF_EXIST_ANTI) continue;
    const uint32_t d = aff_dom(a, ad, v, r, pos);
    if (kind == AF_REQ_AFF) {
      has_req = true;
      if (d == DOM_NONE) return false;  // all topology labels must exist on the node
      if (!aff_sum(a, ad, v, r, pos, d)) exist = false;
    } else if (d != DOM_NONE && aff_sum(a, ad, v, r, pos, d)) {
      return false;
    }
  }
  return !has_req || exist || first_ok;
}

// interpodaffinity Score: Σ topologyScore[key][node's value].
__device__ __forceinline__ int64_t ipa_raw_score(const SpreadArgs &a, const AffDev *ad, uint32_t na, const AffView &v,
                                                 uint32_t pos) {
  int64_t raw = 0;
  for (uint32_t r = 0; r < na; ++r) {
    if ((ad[r].kind & AF_KIND) != AF_SCORE) continue;
    const uint32_t d = aff_dom(a, ad, v, r, pos);
    if (d != DOM_NONE) raw += (int64_t)ad[r].weight * (int64_t)aff_sum(a, ad, v, r, pos, d);
  }
  return raw;
}

// The pod's program staged in LDS by the node-parallel passes: read in every
// node iteration, records in global memory would be re-fetched after each of
// the iteration's stores (the compiler cannot rule out aliasing).
struct SoloLds {
  SoloHdr h;
  SpreadDev sd[MAX_SPREAD];
  XResDev xr[MAX_XRES];
  ImageDev img[MAX_IMG];
  AffDev ad[MAX_AFF];
};
__device__ __forceinline__ void stage_solo(const SpreadArgs &a, const PodDev &p, SoloLds &s) {
  const SoloHdr &h = solo_hdr(a, p);
  const uint32_t t = threadIdx.x;
  if (t == 0) s.h = h;
  if (t < h.n_spread) s.sd[t] = spread_recs(a, p)[t];
  if (t < h.n_xres) s.xr[t] = xres_recs(a, p)[t];
  if (t < h.n_img) s.img[t] = image_recs(a, p)[t];
  if (t < h.n_aff) s.ad[t] = aff_recs(a, p)[t];
}

// imagelocality#calculatePriority over sumImageScores of the node (label bits
// of the "image present" keys); 0 without present images.
__device__ __forceinline__ int64_t image_score(const SoloLds &sl, const NodeExt &e) {
  const SoloHdr &h = sl.h;
  if (!h.n_img) return 0;
  const ImageDev *g = sl.img;
  int64_t sum = 0;
  for (uint32_t k = 0; k < h.n_img; ++k) {
    // the label word by a select chain: a dynamic index would put e.lab in scratch
    const uint32_t wi = g[k].bit >> 6;
    uint64_t w = 0;
#pragma unroll
    for (int q = 0; q < LW; ++q) w = (uint32_t)q == wi ? e.lab[q] : w;
    if ((w >> (g[k].bit & 63)) & 1ull) sum += g[k].scaled;
  }
  const int64_t mb = 1024 * 1024, min_t = 23 * mb, max_t = 1000 * mb * (int64_t)h.n_containers;
  sum = sum < min_t ? min_t : (sum > max_t ? max_t : sum);
  return 100 * (sum - min_t) / (max_t - min_t);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}
__device__ __forceinline__ uint64_t wave_max64(uint64_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t w = __shfl_xor(v, o);
    v = w > v ? w : v;
  }
  return v;
}
__device__ __forceinline__ uint64_t wave_min64(uint64_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const uint64_t w = __shfl_xor(v, o);
    v = w < v ? w : v;
  }
  return v;
}

// LDS segments of the low-cardinality constraints (thread 0; caller syncs);
// with `aoff`, then of the InterPodAffinity records the prep pass sums.
__device__ void lds_segments(const SpreadArgs &a, const SpreadDev *sd, uint32_t n, uint32_t *off,
                             const AffDev *ad = nullptr, uint32_t na = 0, uint32_t *aoff = nullptr) {
  uint32_t o = 0;
  for (uint32_t c = 0; c < n; ++c) {
    const uint32_t nd = a.ndom[sd[c].key];
    const bool small = nd <= SP_LDS_DOM && o + nd <= SP_LDS;
    off[c] = small ? o : SP_OFF_NONE;
    if (small) o += nd;
  }
  for (uint32_t r = 0; r < na; ++r) {
    const uint32_t nd = a.ndom[ad[r].key];
    const bool small = (ad[r].kind & AF_KIND) != AF_OWN && !(ad[r].kind & AF_NODE) && nd <= SP_LDS_DOM &&
                       o + nd <= SP_LDS;
    aoff[r] = small ? o : SP_OFF_NONE;
    if (small) o += nd;
  }
}

__device__ __forceinline__ uint32_t grid_threads() { return gridDim.x * blockDim.x; }

// A position's inputs of the node passes, every load issued before any branch:
// the passes visit each position once, so the slot -> pod-count -> resource-row
// chain of load_core (three dependent round trips through the memory system)
// becomes one.  dm / kc: domain ids and selector-class counts of the pod's
// first SP_PF constraints (kc only where `want_cnt`).
constexpr int SP_PF = 4;
struct PosIn {
  uint32_t slot;
  int32_t ap, np;
  int64_t acpu, amem, rc, rm, zc, zm;
  uint32_t dm[SP_PF], kc[SP_PF];
};
__device__ __forceinline__ void load_pos(const SpreadArgs &a, const SpreadDev *sd, uint32_t n, uint32_t want_cnt,
                                         uint32_t pos, bool core, PosIn &v) {
  v.slot = a.pos_slot[pos];
  v.ap = a.t.apods[pos];
  if (core) {
    v.np = a.t.npods[pos];
    v.acpu = a.t.acpu[pos];
    v.amem = a.t.amem[pos];
    v.rc = a.t.rcpu[pos];
    v.rm = a.t.rmem[pos];
    v.zc = a.t.zcpu[pos];
    v.zm = a.t.zmem[pos];
  }
#pragma unroll
  for (int c = 0; c < SP_PF; ++c) {
    v.dm[c] = (uint32_t)c < n ? a.dom[(size_t)sd[c].key * a.npos + pos] : DOM_NONE;
    v.kc[c] = (uint32_t)c < n && ((want_cnt >> c) & 1u) ? a.cnt[(size_t)sd[c].cls * a.npos + pos] : 0u;
  }
  // the values are needed before the first branch: no load sinks below it
  asm volatile("" ::"v"(v.slot), "v"(v.ap), "v"(v.dm[0]), "v"(v.dm[1]), "v"(v.dm[2]), "v"(v.dm[3]), "v"(v.kc[0]),
               "v"(v.kc[1]), "v"(v.kc[2]), "v"(v.kc[3]));
  if (core) asm volatile("" ::"v"(v.np), "v"(v.acpu), "v"(v.amem), "v"(v.rc), "v"(v.rm), "v"(v.zc), "v"(v.zm));
}
// Domain id of constraint c at the position (prefetched for c < SP_PF).
__device__ __forceinline__ uint32_t pos_dom(const SpreadArgs &a, const SpreadDev *sd, const PosIn &v, uint32_t c,
                                            uint32_t pos) {
  if (c >= (uint32_t)SP_PF) return a.dom[(size_t)sd[c].key * a.npos + pos];
  uint32_t d = v.dm[0];
#pragma unroll
  for (int k = 1; k < SP_PF; ++k) d = c == (uint32_t)k ? v.dm[k] : d;
  return d;
}
// Selector-class count of constraint c at the position (prefetched where want_cnt).
__device__ __forceinline__ uint32_t pos_cnt(const SpreadArgs &a, const SpreadDev *sd, const PosIn &v, uint32_t c,
                                            uint32_t pos) {
  if (c >= (uint32_t)SP_PF) return a.cnt[(size_t)sd[c].cls * a.npos + pos];
  uint32_t k = v.kc[0];
#pragma unroll
  for (int q = 1; q < SP_PF; ++q) k = c == (uint32_t)q ? v.kc[q] : k;
  return k;
}
__device__ __forceinline__ void pos_regs(const SpreadArgs &a, uint32_t pos, const PosIn &v, NodeRegs &r) {
  if (v.ap < 0) load_core(a.t, pos, v.slot, false, r);  // empty slot: load_core's benign values, no loads
  else r = make_regs(v.acpu, v.amem, v.rc, v.rm, v.zc, v.zm, v.ap, v.np, v.slot);
}

// Totals of the accumulator copies (ACC_SHARDS) written by the previous passes.
struct Totals {
  uint32_t fail[NFILT + 2];
  uint32_t feasible, ignored, tt_max, na_max;
  uint64_t pts_min, pts_max, ipa_min, ipa_max, best;
};
__device__ __forceinline__ Totals acc_totals(const SpreadAcc *acc) {
  Totals t{};
  t.pts_min = t.ipa_min = ~0ull;
  for (int k = 0; k < ACC_SHARDS; ++k) {
    const SpreadAccShard &q = acc->sh[k];
    for (int f = 0; f < NFILT + 2; ++f) t.fail[f] += q.fail[f];
    t.ipa_min = min(t.ipa_min, q.ipa_min);
    t.ipa_max = max(t.ipa_max, q.ipa_max);
    t.feasible += q.feasible;
    t.ignored += q.ignored;
    t.tt_max = max(t.tt_max, q.tt_max);
    t.na_max = max(t.na_max, q.na_max);
    t.pts_min = min(t.pts_min, q.pts_min);
    t.pts_max = max(t.pts_max, q.pts_max);
    t.best = max(t.best, q.best);
  }
  return t;
}
__device__ __forceinline__ SpreadAccShard &acc_shard(const SpreadArgs &a) { return a.acc->sh[blockIdx.x % ACC_SHARDS]; }

}  // namespace

}  // namespace ks
