// ksched_forget.hip — ks_batch_forget's kernel.
//
// Cache.ForgetPod for pods a batch placed is the inverse of the commit that
// placed them, and everything the commit read is still resident in the batch:
// the PodDev (the requests), the DevResult (the slot) and, for a pod of the
// one-pod chain, its SoloHdr in the clause buffer (extended-resource records,
// host-port bits).  The kernel runs over the caller's index list -- the call's
// only upload, 4 bytes per pod -- one lane per pod: it reads the slot, the
// position and the PodDev, and subtracts with atomics, several pods of one
// call routinely sharing a node.  The walk of a SoloHdr is at most MAX_XRES
// adds and one and, too short to spread over a wave; a lane per pod keeps 64
// pods' scattered atomics in flight per instruction, and the common pod has no
// header at all.  The selector-class and term-class columns are not touched
// here: the host takes them back through spread_pods_delta, which knows the
// classes created after the batch took its masks.
//
// The host hands over a checked list (indices below the batch's pod count,
// pods scheduled on slots that were not reset since); every index read from
// memory is still compared with its bound before it addresses anything, and a
// pod that fails such a check is counted in *missed: the host reads the count
// back with the call's wait and fails the call, so host and device cannot
// disagree in silence.
#include <hip/hip_runtime.h>

#include "ksched_kernels.hpp"

namespace ks {

__global__ __launch_bounds__(FORGET_THREADS) void forget_kernel(ForgetArgs a) {
  const uint32_t k = blockIdx.x * FORGET_THREADS + threadIdx.x;
  if (k >= a.n) return;
  // a bound that does not hold: nothing is addressed, and the host hears of it (ks_debug_forget [4])
  const auto miss = [&] { atomicAdd(a.missed, 1u); };
  const uint32_t i = a.idx[k];
  if (i >= a.npods) return miss();
  const DevResult &r = a.results[i];
  const uint32_t slot = (uint32_t)r.node_index;
  if (r.status != 0 || slot >= a.nslots) return miss();
  const uint32_t pos = a.slot_pos[slot];
  if (pos >= a.t.npos) return miss();
  const PodDev &p = a.pods[i];
  // NodeInfo.RemovePod: Requested, NonZeroRequested, len(Pods) (64-bit adds as apply_deltas_kernel's)
  atomicAdd((unsigned long long *)&a.t.rcpu[pos], 0ull - (unsigned long long)p.req_cpu);
  atomicAdd((unsigned long long *)&a.t.rmem[pos], 0ull - (unsigned long long)p.req_mem);
  atomicAdd((unsigned long long *)&a.t.zcpu[pos], 0ull - (unsigned long long)p.nz_cpu);
  atomicAdd((unsigned long long *)&a.t.zmem[pos], 0ull - (unsigned long long)p.nz_mem);
  atomicAdd(&a.t.npods[pos], -1);
  if (!(p.flags & PF_SOLO)) return;
  // SoloHdr, n_spread SpreadDev, n_xres XResDev, ... (ksched_dev.hpp)
  constexpr uint64_t HDR_WORDS = sizeof(SoloHdr) / 8, XRES_WORDS = sizeof(XResDev) / 8;
  if (p.solo_off + HDR_WORDS > a.n_words) return miss();
  const SoloHdr &h = *reinterpret_cast<const SoloHdr *>(a.clauses + p.solo_off);
  const uint32_t ns = h.n_spread, nx = h.n_xres;
  if (ns > (uint32_t)MAX_SPREAD || nx > (uint32_t)MAX_XRES) return miss();
  if (p.solo_off + HDR_WORDS + ns * (uint64_t)SPREAD_WORDS + nx * XRES_WORDS > a.n_words) return miss();
  if ((nx && !a.xreq) || (h.ports && !a.used_ports)) return miss();  // records of a column that does not exist
  const XResDev *xr = reinterpret_cast<const XResDev *>(reinterpret_cast<const SpreadDev *>(&h + 1) + ns);
  for (uint32_t e = 0; e < nx; ++e)
    atomicAdd((unsigned long long *)&a.xreq[(size_t)(xr[e].col & (MAX_XRES - 1)) * a.t.npos + pos],
              0ull - (unsigned long long)xr[e].req);
  // HostPortInfo.Remove keeps no reference count: the pod's entries leave outright
  if (h.ports) atomicAnd((unsigned long long *)&a.used_ports[pos], (unsigned long long)~h.ports);
}

hipError_t launch_forget(const ForgetArgs &a, hipStream_t st) {
  if (!a.n) return hipSuccess;
  forget_kernel<<<(a.n + FORGET_THREADS - 1) / FORGET_THREADS, FORGET_THREADS, 0, st>>>(a);
  return hipGetLastError();
}

}  // namespace ks
