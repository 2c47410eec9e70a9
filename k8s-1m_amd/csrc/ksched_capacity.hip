// ksched_capacity.hip — ks_capacity's node-parallel passes.
//
// How many more replicas of a pod the cluster holds is, for the pods the call
// accepts, a closed form over the resident columns: on a node that passes
// every filter before NodeResourcesFit the replicas stop at
//   c = min(free pod slots, floor(free_r / req_r) for every r with req_r > 0)
// (1 at most where the pod has host ports), whatever the scores and the
// tie-break, because only NodeResourcesFit's (and NodePorts') verdict on a
// node changes as replicas land.  Two passes compute it, neither commits:
//   capacity_pods_kernel  pods without a one-pod program, in the geometry of
//       diagnose_pods_kernel (ksched_diag_batch.hip): the lane loads its node
//       row once per grid-stride turn and walks a wave-uniform group of pods
//       whose descriptors come through scalar loads; filter<EXT> unchanged,
//       then the exact capped quotients (ksched_capacity.hpp cap_quot_d)
//   capacity_pod_kernel   a pod with a one-pod program (extended resources,
//       host ports, present images), in diagnose_kernel's place: the program
//       staged in LDS, the extended columns' quotients, the used ports
// Per pod a wave sums its lanes' counts (64 bits: 2^20 nodes of 2^31 slots
// pass 32), takes their maximum, and counts eligible nodes, nodes with room
// and the nodes per binding term by ballot; lane 0 adds them to the block's
// LDS row, and the block issues one global atomic per non-zero counter when
// it ends.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ksched_capacity.hpp"
// (the chain's helpers have internal linkage; this unit stages no domain segments)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunused-function"
#include "ksched_spread_dev.hpp"
#pragma clang diagnostic pop

namespace ks {

namespace {

// a wave-uniform record through the constant address space: scalar loads into
// SGPRs (the call's pods are never written while a pass reads them)
typedef unsigned cp_u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) cp_u32x4 *cp_const_words;
template <class T, int BYTES = (int)sizeof(T)>
__device__ __forceinline__ void load_scalar(const T *src, T &dst) {
  static_assert(BYTES % 16 == 0 && BYTES <= (int)sizeof(T), "16-byte words");
  const cp_const_words s = (cp_const_words)src;
  cp_u32x4 w[BYTES / 16];
#pragma unroll
  for (int k = 0; k < BYTES / 16; ++k) w[k] = s[k];
  __builtin_memcpy(&dst, w, BYTES);
}

// A value folded over the 16 lanes of each DPP row, every lane ending with its
// row's result: four full-rate VALU operations with a DPP operand (lane ^ 1,
// lane ^ 2, the mirrored half row, the mirrored row), no LDS traffic -- the
// shuffle butterflies of sum, maximum and mask cost 22 ds_bpermute per pod and
// wave and were most of what this pass took beyond diagnose_pods_kernel.  All
// 64 lanes are active at the call sites; a lane that is not reads the
// operation's neutral 0.  rows_*: the four rows' results met through v_readlane.
template <class Op>
__device__ __forceinline__ uint32_t row_fold(uint32_t v, Op op) {
  v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false));   // quad_perm [1, 0, 3, 2]
  v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false));   // quad_perm [2, 3, 0, 1]
  v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false));  // row_half_mirror
  v = op(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false));  // row_mirror
  return v;
}
template <class Op>
__device__ __forceinline__ uint32_t rows_fold(uint32_t v, Op op) {
  v = row_fold(v, op);
  return op(op((uint32_t)__builtin_amdgcn_readlane((int)v, 0), (uint32_t)__builtin_amdgcn_readlane((int)v, 16)),
            op((uint32_t)__builtin_amdgcn_readlane((int)v, 32), (uint32_t)__builtin_amdgcn_readlane((int)v, 48)));
}
__device__ __forceinline__ uint32_t op_add(uint32_t a, uint32_t b) { return a + b; }
__device__ __forceinline__ uint32_t op_max(uint32_t a, uint32_t b) { return a > b ? a : b; }
__device__ __forceinline__ uint32_t op_or(uint32_t a, uint32_t b) { return a | b; }
// the wave's sum of counts below 2^31 in 64 bits: the low 16 bits and the rest
// summed apart (64 x 2^16 and 64 x 2^15 fit 32 bits)
__device__ __forceinline__ uint64_t wave_sum64(uint32_t c) {
  const uint32_t lo = rows_fold(c & 0xFFFFu, op_add), hi = rows_fold(c >> 16, op_add);
  return (uint64_t)lo + ((uint64_t)hi << 16);
}

// LDS row of one pod (32 bytes): [0..1] replicas (64 bits), eligible, room,
// max, then the nodes bound by pods / cpu / memory
constexpr uint32_t CR_ELIG = 2, CR_ROOM = 3, CR_MAX = 4, CR_BOUND = 5, CR_ROW = 8;

// A wave's counts of one pod into the row `cnt` (LDS).  elig / c / term: the
// lane's node; c == 0 and term unread where !elig.  NT: terms that can bind.
template <uint32_t NT>
__device__ __forceinline__ void wave_count(uint32_t *cnt, uint32_t *bound, bool elig, uint32_t c, uint32_t term,
                                           uint32_t lane) {
  const uint64_t em = __ballot(elig);
  if (!em) return;  // wave-uniform
  const uint64_t sum = wave_sum64(c);
  const uint32_t mx = rows_fold(c, op_max);
  const uint32_t room = (uint32_t)__builtin_popcountll(__ballot(c >= 1u));
  if (lane == 0) {
    if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(cnt), (unsigned long long)sum);
    atomicAdd(&cnt[CR_ELIG], (uint32_t)__builtin_popcountll(em));
    if (room) atomicAdd(&cnt[CR_ROOM], room);
    if (mx) atomicMax(&cnt[CR_MAX], mx);
  }
  // the nodes per binding term: a ballot per term some lane holds
  uint32_t any = rows_fold(elig ? 1u << term : 0u, op_or) & ((1u << NT) - 1u);
  while (any) {
    const uint32_t b = (uint32_t)__builtin_ctz(any);
    any &= any - 1;
    const uint32_t k = (uint32_t)__builtin_popcountll(__ballot(elig && term == b));
    if (lane == 0) atomicAdd(&bound[b], k);
  }
}

}  // namespace

// EXT: the group's pods may read the taint / label / name columns (PF_EXT).
template <bool EXT>
__global__ __launch_bounds__(CPB_THREADS) void capacity_pods_kernel(CapPodsArgs a) {
  __shared__ __attribute__((aligned(8))) uint32_t s_cnt[CPB_GROUP * CR_ROW];
  const uint32_t g0 = a.first + blockIdx.y * CPB_GROUP;                  // the group's first pod
  const uint32_t ng = min((uint32_t)CPB_GROUP, a.first + a.count - g0);  // its pods (grid.y covers count: >= 1)
  for (uint32_t i = threadIdx.x; i < ng * CR_ROW; i += CPB_THREADS) s_cnt[i] = 0;
  __syncthreads();
  const uint32_t lane = threadIdx.x % WAVE;
  // every thread of the block takes the same number of turns: the wave reductions sit at convergent points
  for (uint32_t bb = blockIdx.x * CPB_THREADS; bb < a.npos; bb += gridDim.x * CPB_THREADS) {
    const uint32_t pos = bb + threadIdx.x;
    // the node row, once for the group's pods
    NodeRegs r;
    NodeExt e{};
    r.bits = 0;
    r.slot = SLOT_NONE;
    r.free_cpu = r.free_mem = 0.0;
    int64_t fc = 0, fm = 0;  // max(0, Allocatable - Requested)
    double fcd = 0.0, fmd = 0.0;
    uint32_t slots = 0;      // max(0, allocatable pods - pods on the node)
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
        fc = max(acpu - rc, (int64_t)0);
        fm = max(amem - rm, (int64_t)0);
        fcd = fmax(r.free_cpu, 0.0);
        fmd = fmax(r.free_mem, 0.0);
        const int64_t fs = (int64_t)ap - (int64_t)np;
        slots = fs > 0 ? (uint32_t)min(fs, (int64_t)CAP_MAX_SLOTS) : 0u;
        if constexpr (EXT) load_ext(a.t, pos, true, e);
      }
    }
    const bool present = r.bits & 1u;
    for (uint32_t g = 0; g < ng; ++g) {
      PodDev p;
      CapPod cp;
      load_scalar(a.pods + g0 + g, p);
      load_scalar<CapPod, 16>(a.cpods + g0 + g, cp);  // rcp_cpu, rcp_mem
      bool elig = false;
      uint32_t c = 0, term = CAP_PODS;
      if (present) {
        const int s = filter<EXT>(p, a.clauses, r, e);
        if (s == ST_FEASIBLE || s == 4) {
          elig = true;
          c = slots;
          if (p.req_cpu > 0) {  // (wave-uniform)
            const uint32_t q = cap_quot_d(fc, fcd, p.req_cpu, cp.rcp_cpu, c);
            if (q < c) c = q, term = CAP_CPU;
          }
          if (p.req_mem > 0) {
            const uint32_t q = cap_quot_d(fm, fmd, p.req_mem, cp.rcp_mem, c);
            if (q < c) c = q, term = CAP_MEM;
          }
        }
        if (a.per_node) a.per_node[r.slot] = c;  // the single-pod call (count == 1)
      }
      uint32_t *cnt = s_cnt + g * CR_ROW;
      wave_count<3>(cnt, cnt + CR_BOUND, elig, c, term, lane);
    }
  }
  __syncthreads();
  if (threadIdx.x < ng) {
    const uint32_t *cnt = s_cnt + threadIdx.x * CR_ROW;
    CapRec &rec = a.recs[g0 + threadIdx.x];
    const unsigned long long sum = *reinterpret_cast<const unsigned long long *>(cnt);
    if (sum) atomicAdd(&rec.replicas, sum);
    if (cnt[CR_ELIG]) atomicAdd(&rec.eligible, cnt[CR_ELIG]);
    if (cnt[CR_ROOM]) atomicAdd(&rec.room, cnt[CR_ROOM]);
    if (cnt[CR_MAX]) atomicMax(&rec.max_per_node, cnt[CR_MAX]);
#pragma unroll
    for (uint32_t b = 0; b < 3; ++b)
      if (cnt[CR_BOUND + b]) atomicAdd(&rec.bound[b], cnt[CR_BOUND + b]);
  }
}

// PORTS: the pod wants host ports (at most one replica per node; nodes whose
// used ports conflict now are not eligible).
template <bool PORTS>
__global__ __launch_bounds__(SP_THREADS) void capacity_pod_kernel(SpreadArgs a, CapPodArgs g) {
  __shared__ __attribute__((aligned(8))) uint32_t s_cnt[CR_ROW];
  __shared__ uint32_t s_bound[CAP_TERMS];
  __shared__ SoloLds s_solo;
  __shared__ CapPod s_cp;
  const PodDev p = a.pods[a.pod];
  stage_solo(a, p, s_solo);
  if (threadIdx.x == 0) s_cp = g.cpods[a.pod];
  if (threadIdx.x < CR_ROW) s_cnt[threadIdx.x] = 0;
  if (threadIdx.x < CAP_TERMS) s_bound[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t n_xres = min(s_solo.h.n_xres, (uint32_t)MAX_XRES);
  const XResDev *xr = s_solo.xr;
  const bool need_ext = p.flags & PF_EXT;  // taint / label columns: the EXT filter chain alone reads them here
  const uint32_t lane = threadIdx.x % WAVE;
  // every lane of a wave takes the same number of steps: the reductions sit at a convergent point
  for (uint32_t base = blockIdx.x * SP_THREADS + (threadIdx.x - lane); base < a.npos; base += grid_threads()) {
    const uint32_t pos = base + lane;
    bool elig = false;
    uint32_t c = 0, term = CAP_PODS;
    if (pos < a.npos) {
      PosIn in;
      uint64_t used_ports = 0;
      if constexpr (PORTS) used_ports = a.used_ports ? a.used_ports[pos] : 0ull;
      load_pos(a, s_solo.sd, 0u, 0u, pos, true, in);
      NodeRegs r;
      r.bits = 0;
      if (in.slot != SLOT_NONE) pos_regs(a, pos, in, r);
      if (r.bits & 1u) {
        NodeExt e{};
        if (need_ext) load_ext(a.t, pos, true, e);
        const int s = filter<true>(p, a.clauses, r, e);
        bool ok = s == ST_FEASIBLE || s == 4;
        // NodePorts, before NodeResourcesFit: a node whose used ports conflict now is not eligible
        if constexpr (PORTS) ok = ok && !(used_ports & a.ports_conflict);
        if (ok) {
          elig = true;
          const int64_t fs = (int64_t)in.ap - (int64_t)in.np;
          c = fs > 0 ? (uint32_t)min(fs, (int64_t)CAP_MAX_SLOTS) : 0u;
          if (p.req_cpu > 0) {
            const int64_t f = max(in.acpu - in.rc, (int64_t)0);
            const uint32_t q = cap_quot_d(f, fmax(r.free_cpu, 0.0), p.req_cpu, s_cp.rcp_cpu, c);
            if (q < c) c = q, term = CAP_CPU;
          }
          if (p.req_mem > 0) {
            const int64_t f = max(in.amem - in.rm, (int64_t)0);
            const uint32_t q = cap_quot_d(f, fmax(r.free_mem, 0.0), p.req_mem, s_cp.rcp_mem, c);
            if (q < c) c = q, term = CAP_MEM;
          }
          // the extended columns, ties to the lower column (the order ks_diagnose names them in)
          for (uint32_t k = 0; k < n_xres; ++k) {
            if (xr[k].req <= 0) continue;
            const uint32_t col = xr[k].col & (MAX_XRES - 1);
            const size_t ix = (size_t)col * a.npos + pos;
            const int64_t f = max(a.xalloc[ix] - a.xreq[ix], (int64_t)0);
            // (capped one above c: a tie is told from a larger quotient)
            const uint32_t q = cap_quot(f, xr[k].req, s_cp.rcp_x[k], c + 1u);
            if (q < c || (q == c && term > CAP_X + col)) c = q, term = CAP_X + col;
          }
          if constexpr (PORTS) {
            if (c > 1u) c = 1u, term = CAP_PORTS;  // the pod conflicts with itself
          }
        }
        if (g.per_node) g.per_node[in.slot] = c;
      }
    }
    wave_count<CAP_TERMS>(s_cnt, s_bound, elig, c, term, lane);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long sum = *reinterpret_cast<const unsigned long long *>(s_cnt);
    if (sum) atomicAdd(&g.rec->replicas, sum);
    if (s_cnt[CR_ELIG]) atomicAdd(&g.rec->eligible, s_cnt[CR_ELIG]);
    if (s_cnt[CR_ROOM]) atomicAdd(&g.rec->room, s_cnt[CR_ROOM]);
    if (s_cnt[CR_MAX]) atomicMax(&g.rec->max_per_node, s_cnt[CR_MAX]);
  } else if (threadIdx.x >= WAVE && threadIdx.x < WAVE + CAP_TERMS) {
    const uint32_t v = s_bound[threadIdx.x - WAVE];
    if (v) atomicAdd(&g.rec->bound[threadIdx.x - WAVE], v);
  }
}

uint32_t capacity_pods_blocks(uint32_t npos) {
  return std::max<uint32_t>(1, std::min<uint32_t>((npos + CPB_THREADS - 1) / CPB_THREADS, (uint32_t)CPB_MAX_BLOCKS));
}

hipError_t launch_capacity_pods(const CapPodsArgs &a, bool ext, hipStream_t st) {
  if (!a.count) return hipSuccess;
  const dim3 grid(capacity_pods_blocks(a.npos), (a.count + CPB_GROUP - 1) / CPB_GROUP);
  if (ext) capacity_pods_kernel<true><<<grid, CPB_THREADS, 0, st>>>(a);
  else capacity_pods_kernel<false><<<grid, CPB_THREADS, 0, st>>>(a);
  return hipGetLastError();
}

hipError_t launch_capacity_pod(const SpreadArgs &args, const CapPodArgs &g, bool ports, hipStream_t st) {
  SpreadArgs a = args;
  a.no_commit = 1;
  a.win_mode = 0;  // over every present node, whatever the window
  a.dump = nullptr;
  const uint32_t blocks =
      std::max<uint32_t>(1, std::min<uint32_t>((a.npos + SP_THREADS - 1) / SP_THREADS, (uint32_t)SPREAD_MAX_BLOCKS));
  if (ports) capacity_pod_kernel<true><<<blocks, SP_THREADS, 0, st>>>(a, g);
  else capacity_pod_kernel<false><<<blocks, SP_THREADS, 0, st>>>(a, g);
  return hipGetLastError();
}

}  // namespace ks
