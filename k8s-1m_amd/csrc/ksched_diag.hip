// ksched_diag.hip — ks_diagnose's node-parallel pass.
//
// Upstream answers an unschedulable pod with a FitError whose text is a
// histogram over the reasons of every node's status.  The one-pod chain's
// filter pass (ksched_spread.hip spread_filter_kernel) knows each node's first
// failing plugin only; this pass runs the same first-failure chain on the same
// grid, with the same loads, and keeps what the status says instead of what
// the scores need:
//   NodeResourcesFit  every insufficient resource and "Too many pods" at once
//                     (fitsRequest collects them all before it returns)
//   TaintToleration   the node's untolerated taint: its dictionary bit where
//                     the node has one, else the node's slot goes to a list
//                     and the host takes the first in the node's taint order
//                     (a bit set holds no order)
//   PodTopologySpread the first failing DoNotSchedule constraint: label
//                     missing, else skew
//   InterPodAffinity  the first failing of satisfyPodAffinity,
//                     satisfyPodAntiAffinity, satisfyExistingPodsAntiAffinity
// A node's status is one 32-bit mask (ksched_diag.hpp DiagBit); a wave ORs its
// lanes' masks and counts, by ballot, only the bits some lane set; the block
// keeps its counters and the 64-bin taint histogram in LDS and issues one
// global atomic per non-zero counter.  No score work, no per-node output:
// what returns to the host is the DiagRec and the used prefix of the list.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ksched_diag.hpp"
#include "ksched_spread_dev.hpp"

namespace ks {

namespace {

// satisfyPodAffinity / satisfyPodAntiAffinity / satisfyExistingPodsAntiAffinity
// over the prefilter domain counts (ipa_fits, by check): the DiagBit of the
// first failing one in upstream's order, or DG_FEASIBLE.
__device__ __forceinline__ uint32_t ipa_reason(const SpreadArgs &a, const AffDev *ad, uint32_t na, const AffView &v,
                                               uint32_t pos, bool first_ok) {
  bool has_req = false, exist = true, missing = false, anti = false, existing = false;
  for (uint32_t r = 0; r < na; ++r) {
    const uint32_t kind = ad[r].kind & AF_KIND;
    if (kind > AF_EXIST_ANTI) continue;
    const uint32_t d = aff_dom(a, ad, v, r, pos);
    if (kind == AF_REQ_AFF) {
      has_req = true;
      if (d == DOM_NONE) missing = true;  // all topology labels must exist on the node
      else if (!aff_sum(a, ad, v, r, pos, d)) exist = false;
    } else if (d != DOM_NONE && aff_sum(a, ad, v, r, pos, d)) {
      (kind == AF_REQ_ANTI ? anti : existing) = true;
    }
  }
  if (missing || (has_req && !exist && !first_ok)) return DG_IPA_AFF;
  return anti ? DG_IPA_ANTI : existing ? DG_IPA_EXIST : DG_FEASIBLE;
}

}  // namespace

// AFF / PORTS: as spread_filter_kernel's -- the pod has InterPodAffinity
// records; the pod wants host ports.
template <bool AFF, bool PORTS>
__global__ __launch_bounds__(SP_THREADS) void diagnose_kernel(SpreadArgs a, DiagArgs g) {
  __shared__ uint32_t s_h[SP_LDS];
  __shared__ uint32_t s_off[MAX_SPREAD];
  __shared__ uint32_t s_aoff[MAX_AFF];
  __shared__ uint32_t s_minm[MAX_SPREAD];
  __shared__ uint32_t s_cnt[32];
  __shared__ uint32_t s_taint[DIAG_TAINT_BINS];
  __shared__ SoloLds s_solo;
  const PodDev p = a.pods[a.pod];
  stage_solo(a, p, s_solo);
  for (uint32_t i = threadIdx.x; i < SP_LDS; i += SP_THREADS) s_h[i] = 0;
  if (threadIdx.x < 32) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x < DIAG_TAINT_BINS) s_taint[threadIdx.x] = 0;
  __syncthreads();
  const SpreadDev *sd = s_solo.sd;
  const uint32_t n = s_solo.h.n_spread;
  if (threadIdx.x == 0) lds_segments(a, sd, n, s_off, s_solo.ad, AFF ? s_solo.h.n_aff : 0u, s_aoff);
  __syncthreads();
  // the prep pass's domain sums and the min pass's minima, staged as the filter pass stages them
  for (uint32_t r = 0; r < (AFF ? s_solo.h.n_aff : 0u); ++r) {
    if (s_aoff[r] == SP_OFF_NONE) continue;
    for (uint32_t d = threadIdx.x; d < a.ndom[s_solo.ad[r].key]; d += SP_THREADS)
      s_h[s_aoff[r] + d] = a.adcnt[(size_t)r * a.dom_cap + d];
  }
  for (uint32_t c = 0; c < n; ++c) {
    if ((sd[c].flags & SP_SCORE) || s_off[c] == SP_OFF_NONE) continue;
    for (uint32_t d = threadIdx.x; d < a.ndom[sd[c].key]; d += SP_THREADS)
      s_h[s_off[c] + d] = a.dcnt[(size_t)c * a.dom_cap + d];
  }
  if (threadIdx.x < n && !(sd[threadIdx.x].flags & SP_SCORE)) {
    const uint32_t c = threadIdx.x;
    s_minm[c] = a.acc->ndomains[c] < (uint32_t)sd[c].min_domains ? 0u : a.acc->min_match[c];
  }
  __syncthreads();
  const uint32_t n_xres = s_solo.h.n_xres;
  const AffDev *ad = s_solo.ad;
  const uint32_t na = AFF ? s_solo.h.n_aff : 0u;
  bool ipa_filter = false;
  for (uint32_t r = 0; r < na; ++r) ipa_filter |= (ad[r].kind & AF_KIND) <= AF_EXIST_ANTI;
  const bool ipa_first_ok = !a.acc->aff_any && (s_solo.h.aff_flags & AFF_SELF);
  const bool need_ext = p.flags & PF_EXT;  // taint / label columns: the EXT filter chain alone reads them here
  const uint32_t lane = threadIdx.x % WAVE;
  // every lane of a wave takes the same number of steps: the reductions below sit at a convergent point
  for (uint32_t base = blockIdx.x * SP_THREADS + (threadIdx.x - lane); base < a.npos; base += grid_threads()) {
    const uint32_t pos = base + lane;
    uint32_t mask = 0;              // the node's status (DiagBit bits); 0: no present node here
    uint32_t tbit = DIAG_TAINT_BINS;  // its one untolerated taint's dictionary bit
    if (pos < a.npos) {
      PosIn in;
      AffView av{s_aoff, s_h, {}, {}};
      if (AFF) aff_prefetch(a, ad, na, pos, av);
      uint64_t used_ports = 0;
      if constexpr (PORTS) used_ports = a.used_ports[pos];
      load_pos(a, sd, n, 0u, pos, true, in);
      if constexpr (PORTS) asm volatile("" ::"v"(used_ports));
      const uint32_t slot = in.slot;
      NodeRegs r;
      r.bits = 0;
      if (slot != SLOT_NONE) pos_regs(a, pos, in, r);
      if (r.bits & 1u) {
        NodeExt e{};
        if (need_ext) load_ext(a.t, pos, true, e);
        int s = filter<true>(p, a.clauses, r, e);
        if constexpr (PORTS) {
          // NodePorts, before NodeResourcesFit: a node failing both is NodePorts'
          if ((s == ST_FEASIBLE || s == 4) && (used_ports & a.ports_conflict)) s = ST_NODE_PORTS;
        }
        if (s == ST_FEASIBLE || s == 4) {
          // fitsRequest: every insufficient resource, not the first
          uint32_t fm = (r.bits & 2u) ? 0u : 1u << DG_FIT_PODS;
          if (p.flags & PF_HAS_REQ) {
            if ((p.req_cpu > 0) & (p.req_cpu_d > r.free_cpu)) fm |= 1u << DG_FIT_CPU;
            if ((p.req_mem > 0) & (p.req_mem_d > r.free_mem)) fm |= 1u << DG_FIT_MEM;
          }
          const XResDev *xr = s_solo.xr;
          for (uint32_t k = 0; k < n_xres; ++k) {
            const uint32_t col = xr[k].col & (MAX_XRES - 1);
            const size_t ix = (size_t)col * a.npos + pos;
            if (xr[k].req > a.xalloc[ix] - a.xreq[ix]) fm |= 1u << (DG_FIT_X + col);
          }
          mask = fm;
          s = fm ? 4 : ST_FEASIBLE;
        }
        if (s == ST_FEASIBLE) {
          for (uint32_t c = 0; c < n; ++c) {
            const SpreadDev &q = sd[c];
            if (q.flags & SP_SCORE) continue;
            const uint32_t d = pos_dom(a, sd, in, c, pos);
            if (d == DOM_NONE) {
              s = PLUGIN_SPREAD;
              mask = 1u << DG_SPREAD_LABEL;
              break;
            }
            const uint32_t dc = s_off[c] != SP_OFF_NONE ? s_h[s_off[c] + d] : a.dcnt[(size_t)c * a.dom_cap + d];
            const int64_t skew = (int64_t)dc + ((q.flags & SP_SELF) ? 1 : 0) - (int64_t)s_minm[c];
            if (skew > (int64_t)q.max_skew) {
              s = PLUGIN_SPREAD;
              mask = 1u << DG_SPREAD_SKEW;
              break;
            }
          }
        }
        if (s == ST_FEASIBLE && ipa_filter) {
          const uint32_t why = ipa_reason(a, ad, na, av, pos, ipa_first_ok);
          if (why != DG_FEASIBLE) {
            s = PLUGIN_IPA;
            mask = 1u << why;
          }
        }
        if (s == ST_FEASIBLE) mask = 1u << DG_FEASIBLE;
        else if (s == ST_PREFILTERED) mask = 1u << DG_PREFILTERED;
        else if (s == ST_NODE_PORTS) mask = 1u << DG_PORTS;
        else if (s <= 4) mask |= 1u << s;  // DG_UNSCHED .. DG_FIT are the plugins' numbers
        if (s == 2) {
          const uint64_t untol = e.hard & ~p.tol_hard & ~UNSCHED_BIT;
          if (__builtin_popcountll(untol) == 1) {
            tbit = (uint32_t)__builtin_ctzll(untol);
          } else {  // several: the node's own taint order decides, which the host holds
            const uint32_t i = atomicAdd(&g.rec->n_multi, 1u);
            if (i < g.list_cap) g.list[i] = slot;
          }
        }
      }
    }
    // the wave's counts: a ballot per bit that some lane set
    uint32_t any = mask;
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) any |= __shfl_xor(any, o);
    any = __builtin_amdgcn_readfirstlane(any);
    while (any) {
      const uint32_t b = (uint32_t)__builtin_ctz(any);
      any &= any - 1;
      const uint32_t c = (uint32_t)__builtin_popcountll(__ballot((mask >> b) & 1u));
      if (lane == 0) atomicAdd(&s_cnt[b], c);
    }
    // the one-taint nodes' bins: one LDS add per distinct bit of the wave
    uint64_t left = __ballot(tbit < (uint32_t)DIAG_TAINT_BINS);
    while (left) {
      const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)tbit, (int)__builtin_ctzll(left));
      const uint64_t same = __ballot(tbit == b);
      if (lane == 0) atomicAdd(&s_taint[b & (DIAG_TAINT_BINS - 1)], (uint32_t)__builtin_popcountll(same));
      left &= ~same;
    }
  }
  __syncthreads();
  if (threadIdx.x < 32) {
    const uint32_t v = s_cnt[threadIdx.x];
    if (v) atomicAdd(&g.rec->cnt[threadIdx.x], v);
  } else if (threadIdx.x >= WAVE && threadIdx.x < WAVE + DIAG_TAINT_BINS) {
    const uint32_t v = s_taint[threadIdx.x - WAVE];
    if (v) atomicAdd(&g.rec->taint[threadIdx.x - WAVE], v);
  }
}

// The domain scratch of the pod's constraints and records cleared, as the
// chain's select pass leaves it (the prep pass filled it).
__global__ __launch_bounds__(SP_THREADS) void diagnose_clear_kernel(SpreadArgs a) {
  const PodDev p = a.pods[a.pod];
  const SpreadDev *sd = spread_recs(a, p);
  const uint32_t n = spread_count(a, p);
  for (uint32_t c = 0; c < n; ++c)
    if ((sd[c].flags & (SP_SCORE | SP_HOST)) != (SP_SCORE | SP_HOST))
      for (uint32_t d = blockIdx.x * SP_THREADS + threadIdx.x; d < a.ndom[sd[c].key]; d += grid_threads()) {
        a.dcnt[(size_t)c * a.dom_cap + d] = 0;
        a.dflag[(size_t)c * a.dom_cap + d] = 0;
      }
  const AffDev *ad = aff_recs(a, p);
  for (uint32_t r = 0; r < solo_hdr(a, p).n_aff; ++r)
    if ((ad[r].kind & AF_KIND) != AF_OWN && !(ad[r].kind & AF_NODE))
      for (uint32_t d = blockIdx.x * SP_THREADS + threadIdx.x; d < a.ndom[ad[r].key]; d += grid_threads())
        a.adcnt[(size_t)r * a.dom_cap + d] = 0;
}

hipError_t launch_diagnose(const SpreadArgs &args, const DiagArgs &g, uint32_t passes, hipStream_t st) {
  SpreadArgs a = args;
  a.no_commit = 1;
  a.win_mode = 0;  // a FitError's loop has visited the whole list: no window
  a.dump = nullptr;
  const uint32_t blocks =
      std::max<uint32_t>(1, std::min<uint32_t>((a.npos + SP_THREADS - 1) / SP_THREADS, (uint32_t)SPREAD_MAX_BLOCKS));
  hipError_t e = hipMemsetAsync(g.rec, 0, sizeof(DiagRec), st);
  if (e != hipSuccess) return e;
  const bool counts = passes & (SPL_PREP | SPL_MIN);
  if (counts && (e = launch_spread_counts(a, passes, st)) != hipSuccess) return e;
  const bool ports = (passes & SPL_PORTS) && a.used_ports;
  if (passes & SPL_AFF) {
    if (ports) diagnose_kernel<true, true><<<blocks, SP_THREADS, 0, st>>>(a, g);
    else diagnose_kernel<true, false><<<blocks, SP_THREADS, 0, st>>>(a, g);
  } else {
    if (ports) diagnose_kernel<false, true><<<blocks, SP_THREADS, 0, st>>>(a, g);
    else diagnose_kernel<false, false><<<blocks, SP_THREADS, 0, st>>>(a, g);
  }
  if ((e = hipGetLastError()) != hipSuccess || !counts) return e;
  diagnose_clear_kernel<<<blocks, SP_THREADS, 0, st>>>(a);
  return launch_spread_reset(a, st);
}

}  // namespace ks
