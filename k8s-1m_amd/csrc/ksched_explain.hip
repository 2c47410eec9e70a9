// ksched_explain.hip — ks_explain's passes.
//
// The one-pod chain's front (prep / min / filter / score, ksched_spread.hip)
// leaves per position the status, the packed normalisation-free score parts,
// the PodTopologySpread raw and the InterPodAffinity raw, and in the
// accumulators the normalisers.  The chain's select pass turns them into
// TotalScores and keeps the best packed key; these passes run in its place:
//   explain_topk_kernel    on the chain's grid, one traversal of the positions
//                          whatever k is: the total of every feasible or
//                          ignored position, formed as the select pass forms
//                          it, and each workgroup's best keys (ksched_explain.hpp:
//                          a sorted list and a staging buffer in LDS), with
//                          the best total and the positions at it; clears the
//                          domain scratch as the select pass does
//   explain_merge_kernel   one workgroup: the blocks' lists through the same
//                          routine, the final keys, the record's counts
//   explain_gather_kernel  one lane per winner: its ks_node_score, recomputed
//                          with the device helpers the score dump uses
// then the accumulators are reset (launch_spread_reset).  No per-node output.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ksched_explain.hpp"
// (the shared helpers have internal linkage, and these passes stage no domain histogram)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "ksched_spread_dev.hpp"
#pragma clang diagnostic pop

namespace ks {

namespace {

constexpr int GATHER_THREADS = KS_EXPLAIN_MAX_CANDIDATES;
static_assert(SP_THREADS == (int)TOPK_STEP, "a step stages at most one key per thread");
static_assert(MAX_SPREAD <= GATHER_THREADS && MAX_XRES <= GATHER_THREADS && MAX_IMG <= GATHER_THREADS &&
                  MAX_AFF <= GATHER_THREADS,
              "stage_solo: one record per thread");

// What the select pass reads from the accumulators before its node loop.
struct ScoreCtx {
  bool has_score, ipa_on;
  int64_t tt_max, na_max, pmin, pmax, imin, idiff;
  uint32_t feasible;
};
__device__ __forceinline__ ScoreCtx score_ctx(const SpreadArgs &a, const SpreadDev *sd, uint32_t n) {
  ScoreCtx c;
  c.has_score = false;
  for (uint32_t q = 0; q < n; ++q) c.has_score |= (sd[q].flags & SP_SCORE) != 0;
  const Totals tot = acc_totals(a.acc);
  c.tt_max = tot.tt_max;
  c.na_max = tot.na_max;
  c.pmin = (int64_t)tot.pts_min;
  c.pmax = (int64_t)tot.pts_max;
  c.ipa_on = a.acc->score_any != 0;
  c.imin = (int64_t)(tot.ipa_min - IPA_BIAS);
  c.idiff = (int64_t)(tot.ipa_max - tot.ipa_min);
  c.feasible = tot.feasible;
  return c;
}

// One feasible (or ignored) position's TotalScore with its normalised parts:
// spread_select_kernel's select_one, the same terms in the same order.
struct NodeTotal {
  int64_t total, raw, norm, ipa_raw, ipa;
};
__device__ __forceinline__ NodeTotal node_total(const SpreadArgs &a, const PodDev &p, const ScoreCtx &c, int8_t s,
                                                uint64_t pk, int64_t raw_in, int64_t ipa_in) {
  NodeTotal t{0, 0, 0, 0, 0};
  if (c.has_score && s != SST_IGNORED) {
    t.raw = raw_in;
    t.norm = c.pmax == 0 ? 100 : 100 * (c.pmax + c.pmin - t.raw) / c.pmax;
  }
  int64_t total = (int64_t)(uint32_t)pk;
  int64_t tt = 100;
  if (p.flags & PF_TT) tt = normalize((int64_t)((pk >> 32) & 0xFF), c.tt_max, true);
  total += (int64_t)a.w.tt * tt;
  if (p.flags & PF_HAS_PREF) {
    int64_t na = 0;
    if (p.flags & PF_NA) na = normalize((int64_t)(pk >> 40), c.na_max, false);
    total += (int64_t)a.w.na * na;
  }
  if (c.has_score) total += (int64_t)a.w_pts * t.norm;
  if (c.ipa_on) {
    t.ipa_raw = ipa_in;
    if (c.idiff > 0) t.ipa = (int64_t)(100.0 * ((double)(t.ipa_raw - c.imin) / (double)c.idiff));
  }
  total += (int64_t)a.w_ipa * t.ipa;
  t.total = total;
  return t;
}

// One step of the workgroup's selection (ksched_explain.hpp): every thread
// offers a key (0: none); the lanes above `thr`, the list's k-th key, go to
// the staging buffer.  Returns the keys the workgroup staged in this step, the
// same value in every thread.  Called by all threads of the block.
__device__ __forceinline__ uint32_t topk_stage(uint64_t *keys, uint32_t *nstage, uint64_t key, uint64_t thr) {
  const bool pass = key > thr;
  const uint64_t m = __ballot(pass);
  if (m) {  // (wave-uniform)
    const uint32_t lane = threadIdx.x % WAVE;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(nstage, (uint32_t)__builtin_popcountll(m));
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    const uint32_t i = base + topk_lane_rank(m, lane);
    // (i < TOPK_STAGE by the flush rule: at most TOPK_FLUSH staged before a step of at most TOPK_STEP)
    if (pass && i < TOPK_STAGE) keys[TOPK_LIST + i] = key;
  }
  return (uint32_t)__syncthreads_count(pass ? 1 : 0);
}
// The staged keys merged into the list; every thread of the block, `staged` uniform.
__device__ __forceinline__ void topk_flush(uint64_t *keys, uint32_t *nstage, uint32_t staged) {
  if (threadIdx.x == 0) *nstage = 0;
  topk_merge(keys, staged, threadIdx.x, blockDim.x, [] { __syncthreads(); });
}
// The list emptied (every thread of the block; ends with a barrier).
__device__ __forceinline__ void topk_init(uint64_t *keys, uint32_t *nstage) {
  for (uint32_t i = threadIdx.x; i < TOPK_LIST; i += blockDim.x) keys[i] = 0;
  if (threadIdx.x == 0) *nstage = 0;
  __syncthreads();
}

__device__ __forceinline__ TopkBest wave_best(TopkBest b) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    TopkBest w;
    w.top = __shfl_xor(b.top, o);
    w.count = __shfl_xor(b.count, o);
    b = topk_best_merge(b, w);
  }
  return b;
}

}  // namespace

__global__ __launch_bounds__(SP_THREADS) void explain_topk_kernel(SpreadArgs a, ExplainArgs x) {
  __shared__ uint64_t s_keys[TOPK_N];
  __shared__ uint32_t s_nstage;
  __shared__ TopkBest s_best[SP_THREADS / WAVE];
  __shared__ SoloLds s_solo;
  const PodDev p = a.pods[a.pod];
  stage_solo(a, p, s_solo);
  topk_init(s_keys, &s_nstage);
  const SpreadDev *sd = s_solo.sd;
  const uint32_t n = s_solo.h.n_spread;
  const ScoreCtx cx = score_ctx(a, sd, n);
  const uint32_t k = x.k;
  uint32_t staged = 0;
  uint64_t thr = 0;
  TopkBest best{0, 0};
  // one position per thread per step; every thread of the block takes the
  // same number of steps, so the barriers of the selection are convergent
  for (uint32_t base = blockIdx.x * SP_THREADS; base < a.npos; base += grid_threads()) {
    const uint32_t pos = base + threadIdx.x;
    uint64_t key = 0;
    if (pos < a.npos) {
      const int8_t s = a.st[pos];
      const uint32_t slot = a.pos_slot[pos];
      if ((s == SST_FEASIBLE || s == SST_IGNORED) && slot != SLOT_NONE) {
        const uint64_t pk = a.part[pos];
        const int64_t raw = cx.has_score && s == SST_FEASIBLE ? a.raw[pos] : 0;
        const int64_t ipr = cx.ipa_on ? a.ipa_raw[pos] : 0;
        key = topk_key(node_total(a, p, cx, s, pk, raw, ipr).total, slot);
        best = topk_best_merge(best, TopkBest{topk_key_top(key), 1u});
      }
    }
    staged += topk_stage(s_keys, &s_nstage, key, thr);
    if (staged > TOPK_FLUSH) {  // (uniform)
      topk_flush(s_keys, &s_nstage, staged);
      staged = 0;
      thr = s_keys[k - 1];
    }
  }
  if (staged) topk_flush(s_keys, &s_nstage, staged);  // (uniform)
  if (threadIdx.x < TOPK_LIST) x.blk_keys[(size_t)blockIdx.x * TOPK_LIST + threadIdx.x] = s_keys[threadIdx.x];
  best = wave_best(best);
  if (threadIdx.x % WAVE == 0) s_best[threadIdx.x / WAVE] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < SP_THREADS / WAVE; ++w) best = topk_best_merge(best, s_best[w]);
    x.blk_best[blockIdx.x] = best;
  }
  // the domain scratch of this pod's constraints and records cleared, as the select pass clears it
  for (uint32_t c = 0; c < n; ++c)
    if ((sd[c].flags & (SP_SCORE | SP_HOST)) != (SP_SCORE | SP_HOST))
      for (uint32_t d = blockIdx.x * SP_THREADS + threadIdx.x; d < a.ndom[sd[c].key]; d += grid_threads()) {
        a.dcnt[(size_t)c * a.dom_cap + d] = 0;
        a.dflag[(size_t)c * a.dom_cap + d] = 0;
      }
  const AffDev *ad = s_solo.ad;
  for (uint32_t r = 0; r < s_solo.h.n_aff; ++r)
    if ((ad[r].kind & AF_KIND) != AF_OWN && !(ad[r].kind & AF_NODE))
      for (uint32_t d = blockIdx.x * SP_THREADS + threadIdx.x; d < a.ndom[ad[r].key]; d += grid_threads())
        a.adcnt[(size_t)r * a.dom_cap + d] = 0;
}

// One workgroup: the heads of the nblk block lists merged into the k final keys, the
// blocks' (best, count) pairs into the tie set, and the record's counts.
__global__ __launch_bounds__(SP_THREADS) void explain_merge_kernel(SpreadArgs a, ExplainArgs x, uint32_t nblk) {
  __shared__ uint64_t s_keys[TOPK_N];
  __shared__ uint32_t s_nstage;
  __shared__ TopkBest s_best[SP_THREADS / WAVE];
  static_assert(SPREAD_MAX_BLOCKS <= SP_THREADS, "one block pair per thread");
  topk_init(s_keys, &s_nstage);
  // the k-entry head of each block's list: what lies below it is not among the k best
  const uint32_t k = x.k, total = nblk * k;
  uint32_t staged = 0;
  uint64_t thr = 0;
  for (uint32_t base = 0; base < total; base += SP_THREADS) {
    const uint32_t i = base + threadIdx.x;
    const uint64_t key = i < total ? x.blk_keys[(size_t)(i / k) * TOPK_LIST + i % k] : 0ull;
    staged += topk_stage(s_keys, &s_nstage, key, thr);
    if (staged > TOPK_FLUSH) {
      topk_flush(s_keys, &s_nstage, staged);
      staged = 0;
      thr = s_keys[k - 1];
    }
  }
  if (staged) topk_flush(s_keys, &s_nstage, staged);
  const bool mine = threadIdx.x < k && s_keys[threadIdx.x] != 0;
  if (threadIdx.x < TOPK_LIST) x.keys[threadIdx.x] = mine ? s_keys[threadIdx.x] : 0ull;
  // the blocks' pairs, one per thread (nblk <= SPREAD_MAX_BLOCKS < SP_THREADS)
  TopkBest best{0, 0};
  if (threadIdx.x < nblk) best = x.blk_best[threadIdx.x];
  best = wave_best(best);
  if (threadIdx.x % WAVE == 0) s_best[threadIdx.x / WAVE] = best;
  const uint32_t ncand = (uint32_t)__syncthreads_count(mine ? 1 : 0);
  if (threadIdx.x == 0) {
    for (int w = 1; w < SP_THREADS / WAVE; ++w) best = topk_best_merge(best, s_best[w]);
    ExplainRec r;
    r.feasible = acc_totals(a.acc).feasible;
    r.n_candidates = ncand;
    r.top_count = best.count;
    r._pad = 0;
    r.top_score = best.top ? (int64_t)best.top - 1 : 0;
    x.out->rec = r;
  }
}

// One lane per winner: the record the score dump (spread_select_kernel with
// SpreadArgs::dump) writes for its slot.  xg: the strategy (1, 2) lists an
// extended resource the pod requests, else 0; bal: the balanced list names a
// scalar resource the pod requests -- the dump's template switches, here
// run-time branches of at most KS_EXPLAIN_MAX_CANDIDATES lanes.
__global__ __launch_bounds__(GATHER_THREADS) void explain_gather_kernel(SpreadArgs a, ExplainArgs x, uint32_t xg,
                                                                        uint32_t bal) {
  __shared__ SoloLds s_solo;
  const PodDev p = a.pods[a.pod];
  stage_solo(a, p, s_solo);
  __syncthreads();
  const uint32_t t = threadIdx.x;
  if (t >= x.k) return;
  const uint64_t key = x.keys[t];
  if (!key) return;
  const ScoreCtx cx = score_ctx(a, s_solo.sd, s_solo.h.n_spread);
  const uint32_t slot = topk_key_slot(key);
  ks_candidate cd{};
  cd.slot = slot;
  cd.score.status = ST_EMPTY;
  const uint32_t pos = slot < a.nslots ? a.slot_pos[slot] : SLOT_NONE;
  if (pos < a.npos) {  // (always: the key came from this position)
    const int8_t s = a.st[pos];
    const NodeTotal nt = node_total(a, p, cx, s, a.part[pos], cx.has_score && s == SST_FEASIBLE ? a.raw[pos] : 0,
                                    cx.ipa_on ? a.ipa_raw[pos] : 0);
    NodeRegs r;
    load_core(a.t, pos, slot, true, r);
    NodeExt e;
    load_ext(a.t, pos, true, e);
    const uint8_t *T = (const uint8_t *)a.fit_table;
    ks_node_score &o = cd.score;
    o.status = ST_FEASIBLE;
    if (xg) {
      FitXSum fx{0, 0};
      const XResDev *xr = s_solo.xr;
      for (uint32_t q = 0; q < s_solo.h.n_xres; ++q) {
        const size_t ix = (size_t)(xr[q].col & (MAX_XRES - 1)) * a.npos + pos;
        const uint32_t w = xfit_weight(a, xr[q].col);
        if (!w) continue;
        const int64_t cap = a.xalloc[ix], req = (int64_t)((uint64_t)a.xreq[ix] + (uint64_t)xr[q].req);
        if (xg == 2) fit_x_resource<2>(fx, w, cap, req, a.fs, T);
        else fit_x_resource<1>(fx, w, cap, req, a.fs, T);
      }
      o.least_allocated = xg == 2 ? score_fit_x<2>(p, r, a.fs, fx, a.xrcp, T) : score_fit_x<1>(p, r, a.fs, fx, a.xrcp, T);
    } else if (a.fit_general == 2) {
      o.least_allocated = score_fit_rtcr(p.nz100_cpu, p.nz100_mem, r, a.fs, T);
    } else {
      o.least_allocated = a.fit_general ? score_fit<1>(p, r, a.fs) : score_fit<0>(p, r, a.fs);
    }
    o.balanced_allocation = bal ? score_ba_list<false>(a, p, r, s_solo.xr, pos) : score_ba(p, r);
    const int64_t tr = (p.flags & PF_TT) ? taint_raw(p, e) : 0;
    o.taint_raw = (int32_t)tr;
    o.taint_score = (int32_t)normalize(tr, (p.flags & PF_TT) ? cx.tt_max : 0, true);
    const int64_t nr = (p.flags & PF_NA) ? preferred_raw(p, a.clauses, e, slot) : 0;
    o.affinity_raw = (int32_t)nr;
    o.affinity_score = (p.flags & PF_HAS_PREF) ? (int32_t)normalize(nr, (p.flags & PF_NA) ? cx.na_max : 0, false) : 0;
    o.image_locality = (int32_t)image_score(s_solo, e);
    o.spread_raw = (int32_t)nt.raw;
    o.spread_score = (int32_t)nt.norm;
    o.affinity_pod_raw = (int32_t)nt.ipa_raw;
    o.affinity_pod_score = (int32_t)nt.ipa;
    o.total_score = nt.total;
  }
  x.out->cand[t] = cd;
}

hipError_t launch_explain(const SpreadArgs &args, const ExplainArgs &x, uint32_t passes, hipStream_t st) {
  if (!x.k || x.k > (uint32_t)KS_EXPLAIN_MAX_CANDIDATES) return hipErrorInvalidValue;
  SpreadArgs a = args;
  a.no_commit = 1;
  a.win_mode = 0;  // over every present node, as the score dump
  a.dump = nullptr;
  hipError_t e = launch_spread_front(a, passes, st);
  if (e != hipSuccess) return e;
  const uint32_t blocks =
      std::max<uint32_t>(1, std::min<uint32_t>((a.npos + SP_THREADS - 1) / SP_THREADS, (uint32_t)SPREAD_MAX_BLOCKS));
  const uint32_t gf = a.fit_general == 2 ? 2u : a.fit_general ? 1u : 0u;
  const uint32_t xg = (passes & SPL_XFIT) && gf ? gf : 0u;
  const uint32_t bal = (passes & SPL_BAL) && (a.bal_lo | a.bal_hi) ? 1u : 0u;
  explain_topk_kernel<<<blocks, SP_THREADS, 0, st>>>(a, x);
  explain_merge_kernel<<<1, SP_THREADS, 0, st>>>(a, x, blocks);
  explain_gather_kernel<<<1, GATHER_THREADS, 0, st>>>(a, x, xg, bal);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  return launch_spread_reset(a, st);
}

}  // namespace ks
