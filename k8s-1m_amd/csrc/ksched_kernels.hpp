// ksched_kernels.hpp — launch arguments and launchers of the gfx950 kernels.
#pragma once

#include <hip/hip_runtime.h>

#include "ksched_dev.hpp"

namespace ks {

constexpr int MAX_PG = 64;    // pods per sweep block (LDS wave records)
constexpr int MAX_P = 256;    // pods per round (resolve stages the round in LDS)
constexpr int MAX_K = 512;    // candidates per pod record (two list entries per list-wave lane in the resolve)
constexpr uint32_t FIX_NONE = 0xFFFFFFFFu;  // fix_list tail
// device counters of the parallel commit (ksched_resolve.hip): chunk passes,
// rounds it resolved
// entries of cpu-sorted sweep lists whose cpu key equals their predecessor's
// in the same pod group: the sweep keeps its cpu terms for them
constexpr int CTR_CPU_SHARED = 9;
constexpr int CTR_PAR_PASSES = 12, CTR_PAR_ROUNDS = 13, CTR_PAR_BAILS = 14, CTR_PAR_ONESTEP = 15;
// per-pod round marks (ks_batch_marks, include/ksched.h): where the round
// machinery changed course, for tests that place checks there
constexpr uint8_t MARK_FIX = 1;          // re-swept with measured normaliser maxima (FIX sweep)
constexpr uint8_t MARK_ROUND_START = 2;  // first pod of a resolved round
constexpr uint8_t MARK_AFTER_WASTE = 4;  // ... whose previous speculated round was wasted

struct RoundArgs {
  NodeTable t;
  const Shard *shards;        // geometry of every shard, device memory (global ids)
  uint32_t total_shards;      // S
  uint32_t shard0;            // first global shard handled by this launch (grid.z / grid.y)
  uint32_t npl;               // nodes per lane of the sweep kernel
  uint32_t sub;               // layout nodes-per-lane / kernel nodes-per-lane
  uint32_t P;                 // pods per round
  uint32_t pg;                // pods per sweep block
  uint32_t K;                 // candidates per pod record
  uint32_t npods;             // batch size
  uint32_t bstride;           // BlockRec stride between pods (max blocks per shard)
  uint32_t evaluated;         // present nodes (EvaluatedNodes with pct = 100)
  uint32_t lnpl;              // layout nodes per lane (positions of committed slots)
  const PodDev *pods;
  const uint64_t *clauses;
  uint32_t *d_start;          // next unresolved pod of the batch (latest, for the host)
  // Two-stage pipeline (sweep k+1 overlaps resolve k), slots indexed by round parity:
  uint32_t *sstart;           // this round's sweep start (speculative)
  const uint32_t *prev_sstart;  // previous round's sweep start
  uint32_t *act;              // this round's actual start (written by the previous resolve)
  uint32_t *act_next;         // next round's actual start (written by this resolve)
  const uint32_t *prev_act;   // previous round's actual start
  const CarryRec *carry_in;   // nodes the previous round's resolve modified (merged by the patch)
  const uint32_t *carry_in_n;
  CarryRec *carry_out;        // nodes this round's resolve modifies
  uint32_t *carry_out_n;
  uint32_t first;             // first round of a pipeline run (no previous round)
  uint32_t *norm_max;         // [P][2] max raw TaintToleration / NodeAffinity over feasible nodes (norm_check)
  double *norm_inv;           // [P][2] RN(1 / norm_max), 0 for 0 (norm_check; FIX-mode sweep)
  const double *guess_inv;    // [npods][2] RN(1 / tt_guess), RN(1 / na_guess) (host)
  PodStat *pstat;             // [P] measured maxima (merge, all shards); nullptr: no normalising pod
  uint32_t *fix_flag;         // [P] the pod's guessed maxima were wrong: re-swept in FIX mode
  uint32_t *fix_group;        // [P / MAX_PG] FIX-mode pod group g holds flagged pods (g * MAX_PG < count)
  uint32_t *fix_list;         // [P] flagged pods of the round in order, then FIX_NONE
  uint32_t fix;               // FIX-mode launch of sweep / merge
  uint32_t pstat_sweep;       // the sweep (not the merge) folds its maxima into pstat (one rank)
  uint32_t *flag_res;         // resolve: round number `seq` stored here when done (null: the host signals)
  uint32_t seq;
  uint32_t stall_us;          // ks_debug_stall: the resolve holds its signal back this long (0: never)
  // Which commit resolves a round (ksched_resolve.hip resolve_kernel runs the
  // parallel one, then the serial one in the same workgroup when needed),
  // RESOLVE_AUTO: rmode[0]: rounds left for the serial commit (the parallel
  // one steps aside while > 0); rmode[1]: seq of the last round the parallel
  // commit resolved; rmode[2]: the next serial stretch.  A round the parallel
  // commit bails on (more than par_max_passes passes, or too few pods per
  // pass) is handed whole to the serial commit, with the next rmode[2]
  // (>= serial_rounds, doubling per consecutive hand-over) rounds.
  // nullptr: RESOLVE_PARALLEL, or RESOLVE_SERIAL with serial_only set.
  uint32_t *rmode;
  uint32_t par_max_passes, serial_rounds;
  uint32_t serial_only;       // RESOLVE_SERIAL: the resolve kernel skips the parallel commit
  uint64_t *prof;             // ks_debug_set_profile: resolve_par_kernel phase cycle sums (null: off)
  uint8_t *marks;             // [npods] per-pod round marks of the batch (ks_batch_marks): KS_MARK_*
  // Identical pods (resource-only batches; null otherwise): pods of a round
  // with byte-identical descriptors have identical lists, so only the first
  // of each class in the round window is swept, merged, gathered and patched
  // and the others read its record.  cls[i]: the batch index of pod i's
  // first identical pod (host); per round (by parity), written by the
  // advance kernel: rep[r] (the window's first pod of r's class), ulist
  // (the representatives) and nuniq (their count).
  // sort_cpu (every resource-only round, also one without identical pods,
  // where cls and rep are null and each pod represents itself): ulist holds
  // the representatives by cpu key (req_cpu, nz_cpu), then window index, so
  // the sweep's per-node cpu terms serve a run of pods;
  // otherwise ulist is in window order.  Everything after the sweep indexes
  // by the pod's window index r, whatever the list's order.
  const uint32_t *cls;
  uint32_t *rep, *ulist, *nuniq;
  uint32_t sort_cpu;
  BlockRec *brec;             // [local shards][P][bstride]
  uint64_t *srec;             // [S][P][rec_words(K)]
  uint64_t *frec;             // [P][rec_words(K)] (== srec when S == 1)
  void *results;              // DevResult[npods]
  CandRow *crow;              // [P][K] S0 rows of the final candidates
  CandExt *cext;              // [P][K] their label / taint columns (EXT batches)
  const uint32_t *slot_pos;   // slot -> position
  uint64_t *counters;         // [0] rounds, [1] pods resolved, [2] pods swept, [3] wasted rounds,
                              // [4] FIX re-swept pods, [7] identical pods not swept (their class's
                              // representative was; [2] counts representatives), [CTR_CPU_SHARED],
                              // [CTR_PAR_*]
  Weights w;
  FitParams fs;               // NodeResourcesFit strategy of the general kernel variants ...
  uint32_t fit_general;       // ... which the launchers choose when set (not {LeastAllocated, 1, 1}):
                              // 1 LeastAllocated / MostAllocated, 2 RequestedToCapacityRatio
  const uint32_t *fit_table;  // 2: the shape table T[0..100] as FIT_TABLE_WORDS dwords (each kernel stages it in
                              // LDS; last, so the members above keep their kernel-argument offsets)
};

struct DumpArgs {
  NodeTable t;
  const uint32_t *slot_pos;   // position of each slot
  uint32_t nslots;
  const PodDev *pods;         // one pod
  const uint64_t *clauses;
  uint32_t *norm_max;         // [2], zeroed
  int32_t *out;               // [nslots][10]
  Weights w;
  FitParams fs;
  uint32_t fit_general;
  const uint32_t *fit_table;  // as RoundArgs::fit_table
};

// PodTopologySpread path (ksched_spread.hip): one pod per launch chain.
constexpr uint32_t SLOT_NONE = 0xFFFFFFFFu;  // position holding no slot (shard padding)
// status, la, ba, tt raw/score, na raw/score, il, pts raw/score, total lo/hi, ipa raw/score
constexpr int SPREAD_DUMP_WORDS = 14;
// launch_spread_pod passes: prep (PodTopologySpread DoNotSchedule counts,
// InterPodAffinity domain counts), min (criticalPaths), score (ScheduleAnyway)
enum SpreadLaunch : uint32_t {
  SPL_PREP = 1u,
  SPL_MIN = 2u,
  SPL_SCORE = 4u,
  SPL_AFF = 8u,    // InterPodAffinity records
  SPL_XFIT = 16u,  // the strategy in force lists an extended resource the pod requests (decided at launch)
  SPL_BAL = 32u,   // the balanced list in force names a scalar resource the pod requests (decided at launch)
  SPL_PORTS = 64u, // the pod wants host ports (NodePorts; its masks are resolved at launch)
};
struct SpreadArgs {
  NodeTable t;
  const uint32_t *pos_slot;   // position -> slot (SLOT_NONE: padding)
  const uint32_t *slot_pos;   // slot -> position
  uint32_t npos;
  uint32_t pod;               // index of the pod in the batch
  const PodDev *pods;
  const uint64_t *clauses;    // label programs + SpreadDev records
  const uint64_t *cmask;      // [npods][CMASK_WORDS] selector classes each pod of the batch matches
  const uint32_t *dom;        // [MAX_TOPO_KEYS][npos] domain id per position (DOM_NONE: key absent)
  uint32_t *cnt;              // [MAX_CLASSES][npos] matching bound pods per position
  int64_t *xalloc, *xreq;     // [MAX_XRES][npos] extended resources: Allocatable, Requested
  uint32_t *dcnt;             // [MAX_SPREAD][dom_cap] per-constraint domain counts (zero between pods)
  uint32_t *dflag;            // [MAX_SPREAD][dom_cap] bit 0 Filter-eligible domain, bit 1 Score domain
  uint32_t *tcnt;             // [MAX_TERM_CLASSES][npos] bound pods carrying each term class
  uint32_t *adcnt;            // [MAX_AFF][dom_cap] InterPodAffinity domain counts per record (zero between pods)
  int64_t *ipa_raw;           // [npos] InterPodAffinity raw score (filter -> select)
  uint32_t dom_cap;
  uint32_t ndom[MAX_TOPO_KEYS];  // domain ids of every topology-key column (at launch)
  SpreadAcc *acc;
  int8_t *st;                 // [npos] status of every position for this pod
  int64_t *raw;               // [npos] PodTopologySpread raw score
  uint64_t *part;             // [npos] normalisation-free score parts of feasible nodes (filter -> select)
  DevResult *results;
  int32_t *dump;              // ks_plugin_scores: [slots][SPREAD_DUMP_WORDS] (null: schedule)
  uint32_t no_commit;         // dump / reset: no result, no AssumePod
  // SPL_BAL: NodeResourcesBalancedAllocationArgs.resources
  // as this pod sees it -- the entries that take part, in list order, resolved
  // to the pod's records when the chain is launched (ksched_ba.hpp), so a
  // program compiled under one list scores under the run's.  0: score_ba.  Its
  // two halves fill the struct's two alignment holes (here and after pct), so
  // no member moves and the size stays: every kernel compiled before reads its
  // arguments where it did
  uint32_t bal_lo;
  uint64_t *counters;
  Weights w;
  FitParams fs;               // as RoundArgs::fs / fit_general
  uint32_t fit_general;
  int32_t w_pts, w_ipa;
  uint32_t evaluated;         // present nodes
  // percentageOfNodesToScore < 100 (ksched_spread.hip spread_window_kernel):
  // win_mode 0 off, 1 the probe filter pass (writes win_st only), 2 the
  // filter pass over the window; win_st [nslots] bit 0 in the node list, bit 1
  // feasible; win [WIN_WORDS] 0 nextStartNodeIndex, 1 the window's first slot,
  // 2 its end slot (exclusive, round the list), 3 every node visited, then
  // [2 per 1024-slot chunk] the chunk's list / feasible counts
  uint32_t *win;
  uint8_t *win_st;
  uint32_t nslots;
  uint32_t win_mode;
  int32_t pct;
  uint32_t bal_hi;            // (bal_lo above)
  // SPL_PORTS: NodeInfo.UsedPorts as one dictionary bit per
  // (ip, protocol, port) triple and position, and the pod's two masks against
  // the dictionary as it is when the chain is launched: the entries a wanted
  // port conflicts with (ks_host_ports_conflict), and the pod's own entries,
  // which the commit adds to the chosen node.  32 bytes, here: the members
  // below move by 32 and keep their alignment and their order, fit_table
  // stays last (the replica kernels load it with ReplicaArgs' head), so every
  // earlier kernel reads the same arguments at shifted offsets
  uint64_t *used_ports;       // [npos] (null until the context has seen a host port)
  uint64_t ports_conflict, ports_add;
  uint64_t _ports_pad;
  // SPL_XFIT: the strategy's weight of each extended-resource
  // column, 8 bits each (0: not listed), resolved when the chain is launched,
  // so a program compiled under one strategy scores under the run's; and the
  // pod's LeastAllocated / MostAllocated reciprocals fit_weight_rcp(W_x +
  // [cpu present] wc + [memory present] wm) at [has_cpu + 2 has_mem]
  uint64_t xw;
  uint32_t xrcp[4];
  const uint32_t *fit_table;  // as RoundArgs::fit_table (last: the replica kernels load it with ReplicaArgs' head)
};
constexpr uint32_t WIN_WORDS = 4;

// Replica runs (ksched_spread.hip): consecutive identical pods
// whose constraints are ScheduleAnyway (at most one kubernetes.io/hostname and
// one other key; the other may be DoNotSchedule), scheduled by one workgroup
// after one filter pass.  Sort
// key of a feasible node, at its slot: group code (ignored << 19 | domain << 8
// | own hostname count) << s_bits | (2^s_bits - 1 - static score).
constexpr uint32_t RUN_GROUPS = 512;    // groups a run can hold (more: the run is refused)
constexpr uint32_t RUN_TOUCHED = 512;   // distinct nodes one run may take (then it ends)
constexpr uint32_t RUN_MIN_PODS = 4;    // shorter sequences take the per-pod chain
constexpr uint32_t RK_HK_NONE = 255;    // the node lacks the hostname key (counts 0..254)
constexpr uint32_t RK_DZ_NONE = 2047;   // the node lacks the other key (domain ids 0..2046)
constexpr uint32_t RK_IGN = 1u << 19;   // PreScore ignores the node (requireAllTopologies)
// The sort runs over 20 + s_bits bits and an infeasible node's key is ~0 there
// (code 0xFFFFF).  Every feasible code keeps bit 19 clear and the ignored code
// keeps bits 0..18 clear, so no feasible or ignored key equals it, whatever the
// static score (2^s_bits - 1 - S with S = 0 included).
static_assert((RK_DZ_NONE << 8 | RK_HK_NONE) < RK_IGN && (RK_IGN | 0x7FFFFu) == 0xFFFFFu &&
                  RK_IGN != 0xFFFFFu,
              "replica sort keys: feasible / ignored codes stay below the infeasible code");
enum RunStop : uint32_t { RUN_END = 0, RUN_FIT = 1, RUN_FULL = 2, RUN_REFUSED = 3 };
constexpr uint32_t RUN_CTL_WORDS = 8;
struct ReplicaArgs {
  uint64_t *keys, *sorted;  // [npos] sort keys, sorted
  uint64_t *val, *sval;     // [nslots] slot << 32 | position of each key, sorted with the keys
  uint32_t *gstart;         // [RUN_GROUPS] first sorted index of each group (unordered)
  uint32_t *ctl;            // [RUN_CTL_WORDS] 0 groups, 1 refuse (a hostname count beyond RK_HK_NONE - 1, an
                            // ignored candidate of a DoNotSchedule run), 2 next pod, 3 RunStop, 4 candidates
                            // only the skew check rejected (DoNotSchedule runs)
  uint32_t end;             // one past the run's last pod
  uint32_t nslots;          // keys sorted (one per slot)
  uint32_t s_bits;          // bits of the static score (2^s_bits > 100 x the static plugins' weights)
  uint64_t *prof;           // KS_RUN_PROFILE: [0..2] cycles of the pod loop's phases, [3] pods (null: off)
};

hipError_t launch_spread_pod(const SpreadArgs &a, uint32_t passes, hipStream_t st);
hipError_t launch_spread_reset(const SpreadArgs &a, hipStream_t st);
// the chain's prep / min passes alone (passes: SPL_PREP / SPL_MIN)
hipError_t launch_spread_counts(const SpreadArgs &a, uint32_t passes, hipStream_t st);
// ks_diagnose (ksched_diag.hip): [prep + min], the diagnose
// pass in the filter pass's place, then the domain scratch and the
// accumulators cleared as the chain's select / commit leave them.  rec is
// zeroed first; list [list_cap]: slots of the nodes with several untolerated
// taints (rec->n_multi of them).
struct DiagRec;
struct DiagArgs {
  DiagRec *rec;
  uint32_t *list;
  uint32_t list_cap;
};
hipError_t launch_diagnose(const SpreadArgs &a, const DiagArgs &g, uint32_t passes, hipStream_t st);
// ks_diagnose_pods (ksched_diag_batch.hip): the pods
// [first, first + count) of the call, none with a one-pod program, evaluated
// in groups of DPB_GROUP on every node row: recs[i] is pod i's record (zeroed
// by the caller); list [list_cap]: (pod, slot) of every node with several
// untolerated taints for a pod, *list_n (zeroed by the caller) the pairs
// produced, which may exceed list_cap; recs[i].n_multi counts pod i's.
constexpr int DPB_THREADS = 512;      // lanes of a block, one node position each per grid-stride turn
constexpr int DPB_GROUP = 64;         // pods per group (grid.y): LDS 64 x 89 counters = 22,784 B
constexpr int DPB_STAGE = 2048;       // (pod, slot) pairs a block stages per turn before it reserves list room: 16 KB
constexpr int DPB_MAX_BLOCKS = 512;   // grid.x: more positions take further turns of the grid-stride loop
struct DiagPair {
  uint32_t pod, slot;
};
struct DiagPodsArgs {
  NodeTable t;
  const uint32_t *pos_slot;   // position -> slot (SLOT_NONE: padding)
  uint32_t npos;
  uint32_t first, count;
  const PodDev *pods;
  const uint64_t *clauses;
  DiagRec *recs;
  DiagPair *list;
  unsigned long long *list_n;
  uint32_t list_cap;
};
// ext: the pods read taint / label / name columns (all of them have PF_EXT, or none)
hipError_t launch_diagnose_pods(const DiagPodsArgs &a, bool ext, hipStream_t st);
uint32_t diagnose_pods_blocks(uint32_t npos);  // grid.x of a launch over npos positions
// ks_capacity (ksched_capacity.hip): the pods [first, first +
// count) of the call, none with a one-pod program, evaluated in groups of
// CPB_GROUP on every node row, in launch_diagnose_pods' geometry: recs[i] is
// pod i's record (zeroed by the caller), cpods[i] its reciprocals; per_node
// [slots] (null, or zeroed by the caller and count == 1): c of every present
// node at its slot.
constexpr int CPB_THREADS = 512;      // lanes of a block, one node position each per grid-stride turn
constexpr int CPB_GROUP = 64;         // pods per group (grid.y): LDS 64 x 8 counters = 2,048 B
constexpr int CPB_MAX_BLOCKS = 512;   // grid.x: more positions take further turns of the grid-stride loop
struct CapPod;
struct CapRec;
struct CapPodsArgs {
  NodeTable t;
  const uint32_t *pos_slot;   // position -> slot (SLOT_NONE: padding)
  uint32_t npos;
  uint32_t first, count;
  const PodDev *pods;
  const CapPod *cpods;
  const uint64_t *clauses;
  CapRec *recs;
  uint32_t *per_node;
};
// ext: the pods read taint / label / name columns (all of them have PF_EXT, or none)
hipError_t launch_capacity_pods(const CapPodsArgs &a, bool ext, hipStream_t st);
uint32_t capacity_pods_blocks(uint32_t npos);  // grid.x of a launch over npos positions
// the per-pod pass for a.pod, a pod with a one-pod program, in launch_diagnose's
// place (no prep / min pass: the call refuses what would need one): cpods
// indexed as a.pods; ports: the pod wants host ports (a.ports_conflict the
// entries they conflict with now); rec zeroed by the caller
struct CapPodArgs {
  CapRec *rec;
  const CapPod *cpods;
  uint32_t *per_node;
};
hipError_t launch_capacity_pod(const SpreadArgs &a, const CapPodArgs &g, bool ports, hipStream_t st);
// the chain's front for a.pod without a window: [prep + min], the filter pass
// launch_spread_pod would choose for `passes`, [score]; the accumulators and
// the per-position columns (st, part, raw, ipa_raw) stay as the select pass
// finds them
hipError_t launch_spread_front(const SpreadArgs &a, uint32_t passes, hipStream_t st);
// ks_explain (ksched_explain.hip): the chain's front, the
// top-k pass in the select pass's place, the one-workgroup merge, the gather
// of the winners' ks_node_score records, then the accumulators reset.
// blk_keys [SPREAD_MAX_BLOCKS][KS_EXPLAIN_MAX_CANDIDATES], blk_best
// [SPREAD_MAX_BLOCKS], keys [KS_EXPLAIN_MAX_CANDIDATES]; a.nslots: the slots
// of slot_pos.
struct TopkBest;
struct ExplainOut;
struct ExplainArgs {
  uint64_t *blk_keys;
  TopkBest *blk_best;
  uint64_t *keys;
  ExplainOut *out;
  uint32_t k;
};
hipError_t launch_explain(const SpreadArgs &a, const ExplainArgs &x, uint32_t passes, hipStream_t st);
// [prep + min passes (passes: SPL_PREP / SPL_MIN, a DoNotSchedule
// constraint)], the filter pass for a.pod, keys, sort, groups, the run
// kernel; ctl zeroed first
hipError_t launch_replica_run(const SpreadArgs &a, const ReplicaArgs &r, void *sort_tmp, size_t sort_tmp_bytes,
                              uint32_t passes, hipStream_t st);
hipError_t launch_sort_pairs(const uint64_t *kin, uint64_t *kout, const uint64_t *vin, uint64_t *vout, uint32_t n,
                             uint32_t end_bit, void *tmp, size_t *tmp_bytes, hipStream_t st);
hipError_t launch_class_commit(const DevResult *res, const uint64_t *cmask, const uint32_t *slot_pos, uint32_t *cnt,
                               uint32_t npos, uint32_t lo, uint32_t hi, hipStream_t st);
hipError_t launch_scatter_u32(uint32_t *col, const uint64_t *idx, const uint32_t *val, uint32_t n, hipStream_t st);
hipError_t launch_add_u32(uint32_t *col, const uint64_t *idx, const int32_t *delta, uint32_t n, hipStream_t st);
hipError_t launch_umax_u32(uint32_t *dst, const uint32_t *src, uint32_t n, hipStream_t st);
hipError_t launch_scatter_i64(int64_t *col, const uint64_t *idx, const int64_t *val, uint32_t n, bool add,
                              hipStream_t st);
// used-ports column: col[pos[i]] |= bits[i] (clear: &= ~bits[i]); positions may repeat
hipError_t launch_ports_update(uint64_t *col, const uint32_t *pos, const uint64_t *bits, uint32_t n, bool clear,
                               hipStream_t st);

hipError_t launch_norm_check(const RoundArgs &a, hipStream_t st);
// Label-word variant of the label / taint sweep (sweep_kernel's LWU): the
// words per node it reads, by the dictionary's width.  NPL 8 is compiled for
// 4 words only.  launch_sweep dispatches by it and ks_debug_sweep_geometry
// reports it.
inline uint32_t sweep_label_words(uint32_t knpl, uint32_t lw) {
  return knpl == 8 ? 4u : lw <= 1 ? 1u : lw <= 2 ? 2u : 4u;
}
hipError_t launch_sweep(const RoundArgs &a, bool ext, uint32_t nblocks, uint32_t ngroups, uint32_t nshards,
                        hipStream_t st);
hipError_t launch_merge(const RoundArgs &a, uint32_t nshards, hipStream_t st);
hipError_t launch_merge_shards(const RoundArgs &a, hipStream_t st);
hipError_t launch_gather_cand(const RoundArgs &a, bool ext, hipStream_t st);
hipError_t launch_patch(const RoundArgs &a, bool ext, hipStream_t st);
hipError_t launch_resolve(const RoundArgs &a, bool ext, hipStream_t st);
hipError_t launch_advance(const RoundArgs &a, hipStream_t st);
hipError_t launch_advance_writeback(const RoundArgs &a, const CarryRec *carry, const uint32_t *n, hipStream_t st);
hipError_t launch_writeback(const NodeTable &t, const CarryRec *carry, const uint32_t *n, hipStream_t st);
hipError_t launch_scatter_rows(const NodeTable &t, const uint32_t *pos, const int64_t *core, const uint64_t *ext,
                               uint32_t n, uint32_t flags, hipStream_t st);
hipError_t launch_apply_deltas(const NodeTable &t, const uint32_t *pos, const int64_t *delta, uint32_t n,
                               hipStream_t st);
hipError_t launch_gather_rows(const NodeTable &t, const uint32_t *pos, int64_t *out, uint32_t n, hipStream_t st);
hipError_t launch_scatter_u64(uint64_t *col, const uint32_t *pos, const uint64_t *val, uint32_t n,
                              hipStream_t st);
hipError_t launch_dump(const DumpArgs &a, hipStream_t st);
// ks_batch_forget (ksched_forget.hip): the pods idx[0..n) of a
// batch that ran, taken back from the rows they were bound to: Requested,
// NonZeroRequested and the pod count from the PodDev, the extended-resource
// columns and the used-port bits from the pod's SoloHdr.  One lane per pod,
// atomics throughout (pods of one call share nodes).  xreq / used_ports may be
// null (no column / no dictionary entry yet: no pod of the batch has either).
struct ForgetArgs {
  NodeTable t;
  const uint32_t *slot_pos;  // [nslots]
  const DevResult *results;  // the batch's, [npods]
  const PodDev *pods;        // [npods]
  const uint64_t *clauses;   // the batch's clause buffer, n_words words
  const uint32_t *idx;       // [n] batch indices
  int64_t *xreq;             // [MAX_XRES][npos]
  uint64_t *used_ports;      // [npos]
  uint32_t *missed;          // += pods a bound check of the kernel turned away (zeroed by the caller; 0 unless
                             // host and device disagree)
  uint64_t n_words;
  uint32_t n, npods, nslots;
};
constexpr uint32_t FORGET_THREADS = 256;
hipError_t launch_forget(const ForgetArgs &a, hipStream_t st);
// ks_debug_stall: one wave that waits `usec` microseconds of wall clock, then exits
hipError_t launch_stall(uint32_t usec, hipStream_t st);

}  // namespace ks
