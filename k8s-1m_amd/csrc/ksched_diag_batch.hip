// ksched_diag_batch.hip — ks_diagnose_pods' multi-pod pass.
//
// ks_diagnose's pass (ksched_diag.hip) reads every node row for one pod.  The
// status of a pod without a one-pod program (PF_SOLO clear) on a node is a
// function of the node row and the PodDev alone, so this pass loads a lane's
// node row once and evaluates it for a group of DPB_GROUP pods, as the sweep
// does: the grid's x runs over node positions (one per lane and grid-stride
// turn), its y over the pod groups; the pod loop is wave-uniform and reads the
// PodDev through scalar loads.  Per (pod, node) the status is filter<EXT> of
// ksched_eval.hpp and, where the node passes or fails at NodeResourcesFit,
// fitsRequest's complete reason set -- the DiagBit mask diagnose_kernel builds
// for such a pod.  Counting is diagnose_kernel's: the wave ORs its masks, one
// ballot per bit some lane set, LDS counters [group][DG_BITS] and, in the EXT
// variant, a taint histogram [group][64]; one global atomic per non-zero
// counter when the block ends.  A node with several untolerated taints goes,
// as a (pod, slot) pair, to one list shared by the call's pods, through a
// staging buffer in LDS that the block empties once per turn; the pod's own
// count (DiagRec::n_multi) stays exact when the list is full, so the host sees
// which pods lost entries.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ksched_diag.hpp"
#include "ksched_eval.hpp"
#include "ksched_kernels.hpp"

namespace ks {

namespace {

// a wave-uniform pod descriptor through the constant address space: scalar
// loads into SGPRs (the call's pods are never written while the pass reads them)
typedef unsigned dp_u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) dp_u32x4 *dp_const_words;
__device__ __forceinline__ PodDev load_pod_scalar(const PodDev *pods, uint32_t i) {
  const dp_const_words src = (dp_const_words)(pods + i);
  dp_u32x4 w[sizeof(PodDev) / 16];
#pragma unroll
  for (int k = 0; k < (int)(sizeof(PodDev) / 16); ++k) w[k] = src[k];
  PodDev p;
  __builtin_memcpy(&p, w, sizeof p);
  return p;
}

}  // namespace

// EXT: the group's pods may read the taint / label / name columns (PF_EXT).
template <bool EXT>
__global__ __launch_bounds__(DPB_THREADS) void diagnose_pods_kernel(DiagPodsArgs a) {
  // LDS counters per pod: the DiagBits, then (EXT) the taint bins and the pod's listed nodes
  constexpr uint32_t ROW = EXT ? DG_BITS + DIAG_TAINT_BINS + 1 : DG_BITS;
  [[maybe_unused]] constexpr uint32_t MULTI = DG_BITS + DIAG_TAINT_BINS;
  __shared__ uint32_t s_cnt[DPB_GROUP * ROW];
  // the pairs one turn lists, staged: one reservation in the shared list per block and turn (every wave
  // reserving for itself put all the call's waves on one address)
  __shared__ DiagPair s_pairs[EXT ? DPB_STAGE : 1];
  __shared__ uint32_t s_np;             // pairs of this turn; those beyond DPB_STAGE went to the list themselves
  __shared__ unsigned long long s_at;   // the block's reservation
  const uint32_t g0 = a.first + blockIdx.y * DPB_GROUP;               // the group's first pod
  const uint32_t ng = min((uint32_t)DPB_GROUP, a.first + a.count - g0);  // its pods (grid.y covers count: >= 1)
  for (uint32_t i = threadIdx.x; i < ng * ROW; i += DPB_THREADS) s_cnt[i] = 0;
  if (threadIdx.x == 0) s_np = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x % WAVE;
  // every thread of the block takes the same number of turns: the wave reductions and the block's barriers
  // below sit at convergent points
  for (uint32_t bb = blockIdx.x * DPB_THREADS; bb < a.npos; bb += gridDim.x * DPB_THREADS) {
    const uint32_t pos = bb + threadIdx.x;
    // the node row, once for the group's pods
    NodeRegs r;
    NodeExt e{};
    r.bits = 0;
    r.slot = SLOT_NONE;
    r.free_cpu = r.free_mem = 0.0;
    if (pos < a.npos) {
      const uint32_t slot = a.pos_slot[pos];
      const int32_t ap = a.t.apods[pos];
      const int32_t np = a.t.npods[pos];
      const int64_t acpu = a.t.acpu[pos], amem = a.t.amem[pos], rc = a.t.rcpu[pos], rm = a.t.rmem[pos];
      if (slot != SLOT_NONE && ap >= 0) {
        r.slot = slot;
        r.free_cpu = (double)(acpu - rc);  // make_regs' values of the fields filter reads
        r.free_mem = (double)(amem - rm);
        r.bits = 1u | ((int64_t)np + 1 <= (int64_t)ap ? 2u : 0u);
        if constexpr (EXT) load_ext(a.t, pos, true, e);
      }
    }
    const bool present = r.bits & 1u;
    for (uint32_t g = 0; g < ng; ++g) {
      const PodDev p = load_pod_scalar(a.pods, g0 + g);
      uint32_t mask = 0;                // the node's status for this pod (DiagBit bits); 0: no present node here
      uint32_t tbit = DIAG_TAINT_BINS;  // its one untolerated taint's dictionary bit
      bool multi = false;               // several untolerated taints: the node is listed
      if (present) {
        int s = filter<EXT>(p, a.clauses, r, e);
        if (s == ST_FEASIBLE || s == 4) {
          // fitsRequest: every insufficient resource, not the first
          uint32_t fm = (r.bits & 2u) ? 0u : 1u << DG_FIT_PODS;
          if (p.flags & PF_HAS_REQ) {
            if ((p.req_cpu > 0) & (p.req_cpu_d > r.free_cpu)) fm |= 1u << DG_FIT_CPU;
            if ((p.req_mem > 0) & (p.req_mem_d > r.free_mem)) fm |= 1u << DG_FIT_MEM;
          }
          mask = fm;
          s = fm ? 4 : ST_FEASIBLE;
        }
        if (s == ST_FEASIBLE) mask = 1u << DG_FEASIBLE;
        else if (s == ST_PREFILTERED) mask = 1u << DG_PREFILTERED;
        else mask |= 1u << s;  // DG_UNSCHED .. DG_FIT are the plugins' numbers (filter returns 0 .. 4 here)
        if constexpr (EXT) {
          if (s == 2) {
            const uint64_t untol = e.hard & ~p.tol_hard & ~UNSCHED_BIT;
            if (__builtin_popcountll(untol) == 1) tbit = (uint32_t)__builtin_ctzll(untol);
            else multi = true;  // the node's own taint order decides, which the host holds
          }
        }
      }
      uint32_t *cnt = s_cnt + g * ROW;
      // the wave's counts: a ballot per bit that some lane set
      uint32_t any = mask;
#pragma unroll
      for (int o = 32; o >= 1; o >>= 1) any |= __shfl_xor(any, o);
      any = __builtin_amdgcn_readfirstlane(any) & ((1u << DG_BITS) - 1u);
      while (any) {
        const uint32_t b = (uint32_t)__builtin_ctz(any);
        any &= any - 1;
        const uint32_t c = (uint32_t)__builtin_popcountll(__ballot((mask >> b) & 1u));
        if (lane == 0) atomicAdd(&cnt[b], c);
      }
      if constexpr (EXT) {
        // the one-taint nodes' bins: one LDS add per distinct bit of the wave
        uint64_t left = __ballot(tbit < (uint32_t)DIAG_TAINT_BINS);
        while (left) {
          const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)tbit, (int)__builtin_ctzll(left));
          const uint64_t same = __ballot(tbit == b);
          if (lane == 0) atomicAdd(&cnt[DG_BITS + (b & (DIAG_TAINT_BINS - 1))], (uint32_t)__builtin_popcountll(same));
          left &= ~same;
        }
        // the listed nodes: one place per wave in the block's staging; the pod's own count is exact whatever fits
        const uint64_t mm = __ballot(multi);
        if (mm) {
          const uint32_t lead = (uint32_t)__builtin_ctzll(mm), c = (uint32_t)__builtin_popcountll(mm);
          uint32_t at = 0;
          if (lane == lead) {
            at = atomicAdd(&s_np, c);
            atomicAdd(&cnt[MULTI], c);
          }
          at = __shfl(at, (int)lead);
          if (multi) {
            const uint32_t i = at + (uint32_t)__builtin_popcountll(mm & ((1ull << lane) - 1ull));
            const DiagPair pr{g0 + g, r.slot};
            if (i < (uint32_t)DPB_STAGE) {
              s_pairs[i] = pr;
            } else {  // the staging is full (most of the turn's nodes are listed): straight to the list
              const unsigned long long j = atomicAdd(a.list_n, 1ull);
              if (j < (unsigned long long)a.list_cap) a.list[j] = pr;
            }
          }
        }
      }
    }
    if constexpr (EXT) {
      __syncthreads();
      // the same in every thread: s_np rests until the reset below
      const uint32_t staged = min(s_np, (uint32_t)DPB_STAGE);
      if (staged) {
        if (threadIdx.x == 0) s_at = atomicAdd(a.list_n, (unsigned long long)staged);
        __syncthreads();
        const unsigned long long at = s_at;
        for (uint32_t i = threadIdx.x; i < staged; i += DPB_THREADS)
          if (at + i < (unsigned long long)a.list_cap) a.list[at + i] = s_pairs[i];
      }
      __syncthreads();
      if (threadIdx.x == 0) s_np = 0;
      __syncthreads();
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < ng * ROW; i += DPB_THREADS) {
    const uint32_t v = s_cnt[i];
    if (!v) continue;
    DiagRec &rec = a.recs[g0 + i / ROW];
    const uint32_t k = i % ROW;
    atomicAdd(k < (uint32_t)DG_BITS ? &rec.cnt[k] : k < MULTI ? &rec.taint[k - DG_BITS] : &rec.n_multi, v);
  }
}

uint32_t diagnose_pods_blocks(uint32_t npos) {
  return std::max<uint32_t>(1, std::min<uint32_t>((npos + DPB_THREADS - 1) / DPB_THREADS, (uint32_t)DPB_MAX_BLOCKS));
}

hipError_t launch_diagnose_pods(const DiagPodsArgs &a, bool ext, hipStream_t st) {
  if (!a.count) return hipSuccess;
  const dim3 grid(diagnose_pods_blocks(a.npos), (a.count + DPB_GROUP - 1) / DPB_GROUP);
  if (ext) diagnose_pods_kernel<true><<<grid, DPB_THREADS, 0, st>>>(a);
  else diagnose_pods_kernel<false><<<grid, DPB_THREADS, 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace ks
