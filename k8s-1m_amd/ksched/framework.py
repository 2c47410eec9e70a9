"""Host-side mirror of the scheduler framework surface this path sits behind.

The reference calls the forked kube-scheduler's ``Scheduler.SchedulePod``
(upstream k8s.io/kubernetes v1.31.3 pkg/scheduler/schedule_one.go#schedulePod)
from ``ScheduleOne`` (dist-scheduler/cmd/dist-scheduler/scheduler.go:543) and
reads its outcome in two places:

* ``DistPermit.Permit`` reads ``framework.NodePluginScoresState`` from the
  CycleState and sends the chosen node's ``TotalScore`` as int32
  (dist-scheduler/pkg/distpermit/distpermit.go:51-72, :106);
* ``podScheduleFailure`` type-asserts ``*framework.FitError`` and reads
  ``Diagnosis.UnschedulablePlugins`` (scheduler.go:383-395).

``Scheduler`` below keeps those names, argument meanings and error behaviour:
``schedule_pod`` returns a ``ScheduleResult`` and writes
``NodePluginScoresState`` into the CycleState, or raises ``FitError``
(no feasible node) / ``FrameworkError`` (an Error status).  Every call goes to
libksched.so (HIP); there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from enum import IntEnum
from typing import Dict, List, Optional, Sequence, Union

from . import _abi
from .objects import Arena, Node, Pod, nodes_array, pods_array

FILTER_PLUGINS = ["NodeUnschedulable", "NodeName", "TaintToleration", "NodeAffinity", "NodeResourcesFit",
                  "PodTopologySpread", "InterPodAffinity"]
NODE_PLUGIN_SCORES_STATE_KEY = "NodePluginScores"  # fork: framework.NodePluginScoresStateKey
DEFAULT_WEIGHTS = {  # apis/config/v1 default plugin weights (v1.31)
    "NodeResourcesFit": 1,
    "NodeResourcesBalancedAllocation": 1,
    "TaintToleration": 3,
    "NodeAffinity": 2,
    "ImageLocality": 1,
    "PodTopologySpread": 2,
    "InterPodAffinity": 2,
}


class Code(IntEnum):  # framework.Code
    Success = 0
    Error = 1
    Unschedulable = 2
    UnschedulableAndUnresolvable = 3
    Wait = 4
    Skip = 5


@dataclass
class ScheduleResult:  # scheduler.ScheduleResult
    suggested_host: str
    evaluated_nodes: int
    feasible_nodes: int
    node_index: int = -1
    total_score: int = 0
    single_feasible: bool = False


@dataclass
class Diagnosis:  # framework.Diagnosis (NodeToStatus summarised per plugin)
    node_to_status: Dict[str, int] = field(default_factory=dict)
    unschedulable_plugins: set = field(default_factory=set)


class FitError(Exception):  # framework.FitError
    def __init__(self, pod: str, num_all_nodes: int, diagnosis: Diagnosis):
        self.pod = pod
        self.num_all_nodes = num_all_nodes
        self.diagnosis = diagnosis
        super().__init__(f"0/{num_all_nodes} nodes are available for pod {pod}: {diagnosis.node_to_status}")


@dataclass
class FitDiagnosis:  # what a FitError says: Diagnosis' reasons as a histogram over the nodes (ks_diagnose)
    num_all_nodes: int
    feasible_nodes: int
    plugin_nodes: List[int]      # nodes by first failing plugin (FILTER_PLUGINS, then the PreFilterResult's)
    node_ports_nodes: int        # ... by NodePorts
    reasons: Dict[str, int]      # upstream's reason string -> nodes whose status carries it
    prefilter_msg: Optional[str]
    message: str                 # FitError.Error() without the PostFilter part


class _NodeCapacity(int):
    """``Scheduler.capacity``: the context's node capacity (an int, as before),
    callable as the capacity query ``capacity(pod, per_node=False)``."""
    query = None

    def __call__(self, pod, per_node: bool = False):
        return self.query(pod, per_node)


@dataclass
class Capacity:  # how many more replicas of a pod the cluster holds (ks_capacity_pod)
    num_all_nodes: int
    eligible_nodes: int          # nodes passing every filter before NodeResourcesFit
    nodes_with_room: int         # ... of those, the nodes holding at least one more replica
    max_per_node: int
    replicas: int                # the sum over the nodes
    bound_by: Dict[str, int]     # eligible nodes per binding term: "pods", "cpu", "memory", a resource name, "ports"
    per_node: Optional[object] = None  # numpy uint32 [capacity]: replicas per slot (``per_node=True``)


def fit_error_message(num_all_nodes: int, reasons, prefilter_msg: Optional[str] = None) -> str:
    """FitError.Error() of (reason, count) pairs (ks_fit_error_message: pure host code)."""
    lib = _abi.ksched_lib()
    pairs = list(reasons.items()) if isinstance(reasons, dict) else list(reasons)
    arr = (_abi.KsReason * max(1, len(pairs)))(*[_abi.KsReason(0, int(c), str(r).encode()) for r, c in pairs])
    pm = None if prefilter_msg is None else prefilter_msg.encode()
    n = C.c_size_t()
    lib.ks_fit_error_message(num_all_nodes, pm, arr, len(pairs), None, 0, C.byref(n))  # sizes the buffer
    buf = C.create_string_buffer(n.value + 1)
    st = lib.ks_fit_error_message(num_all_nodes, pm, arr, len(pairs), buf, n.value + 1, C.byref(n))
    if st != 0:
        raise _abi.KschedError(st, "ks_fit_error_message")
    return buf.value.decode()


class FrameworkError(Exception):
    """A plugin returned an Error status (e.g. NodeAffinity PreScore parse error)."""


@dataclass
class PluginScore:
    name: str
    score: int


@dataclass
class NodePluginScores:  # framework.NodePluginScores
    name: str
    scores: List[PluginScore]
    total_score: int
    slot: int = -1                             # Scheduler.explain: the node's slot
    raw: Optional[_abi.KsNodeScore] = None     # ... and its ks_node_score record


@dataclass
class NodePluginScoresState:  # fork-only framework.NodePluginScoresState
    node_plugin_scores: List[NodePluginScores]


# The normalised score of each score plugin of DEFAULT_WEIGHTS in a ks_node_score record.
SCORE_FIELDS = {
    "NodeResourcesFit": "least_allocated",
    "NodeResourcesBalancedAllocation": "balanced_allocation",
    "TaintToleration": "taint_score",
    "NodeAffinity": "affinity_score",
    "ImageLocality": "image_locality",
    "PodTopologySpread": "spread_score",
    "InterPodAffinity": "affinity_pod_score",
}


@dataclass
class Explanation:  # a pod's best nodes with their NodePluginScores (ks_explain)
    num_all_nodes: int
    feasible_nodes: int
    top_score: int                 # 0 when no node is feasible
    top_score_nodes: int           # feasible nodes at top_score: selectHost's tie set
    candidates: List[NodePluginScores]  # TotalScore descending, then slot ascending


class CycleState(dict):  # framework.CycleState (Read / Write)
    def write(self, key, value):
        self[key] = value

    def read(self, key):
        if key not in self:
            raise KeyError(f"{key} not found")
        return self[key]


def _check(lib, ctx, st: int):
    if st != 0:
        msg = lib.ks_last_error(ctx).decode() if ctx else "error"
        raise _abi.KschedError(st, msg)


class Scheduler:
    """One shard's scheduling core on one GPU (a ks_ctx)."""

    def __init__(self, node_capacity: int, *, device: int = 0, pods_per_round: int = 256, topk: int = 0,
                 nodes_per_lane: int = 4, world_size: int = 1, rank: int = 0, virtual_shards: int = 1,
                 weights: Optional[Dict[str, int]] = None, options: Optional[Dict[str, int]] = None,
                 percentage_of_nodes_to_score: int = 100, fit_strategy: str = "LeastAllocated",
                 fit_resource_weights: Optional[Dict[str, int]] = None, fit_shape=None,
                 balanced_resources=None, hard_pod_affinity_weight: int = 1):
        """weights: the profile's score plugin weights by plugin name, over
        DEFAULT_WEIGHTS.  hard_pod_affinity_weight: InterPodAffinityArgs.
        hardPodAffinityWeight.  A weight of 0 multiplies by 0 (ksched.h).
        options: ks_config execution options by field name (_abi.OPTION_FIELDS),
        e.g. {"resolve_mode": _abi.RESOLVE_SERIAL, "dedup_identical_pods": 0};
        none of them changes a result.  percentage_of_nodes_to_score: the
        profile's percentageOfNodesToScore (ksched.h; below 100 one shard only).
        fit_strategy / fit_resource_weights / fit_shape:
        NodeResourcesFitArgs.scoringStrategy (set_fit_strategy).
        balanced_resources: NodeResourcesBalancedAllocationArgs.resources, an
        ordered list of names (set_balanced_resources)."""
        self.lib = _abi.ksched_lib()
        cfg = _abi.KsConfig()
        self.lib.ks_config_default(C.byref(cfg))
        for k, v in (options or {}).items():
            if k not in _abi.OPTION_FIELDS:
                raise ValueError(f"unknown ks_config option {k}")
            setattr(cfg, k, int(v))
        cfg.device = device
        cfg.node_capacity = node_capacity
        cfg.pods_per_round = pods_per_round
        cfg.topk = topk
        cfg.nodes_per_lane = nodes_per_lane
        cfg.world_size = world_size
        cfg.rank = rank
        cfg.virtual_shards = virtual_shards
        w = dict(DEFAULT_WEIGHTS, **(weights or {}))
        cfg.weight_fit = w["NodeResourcesFit"]
        cfg.weight_balanced = w["NodeResourcesBalancedAllocation"]
        cfg.weight_taint = w["TaintToleration"]
        cfg.weight_affinity = w["NodeAffinity"]
        cfg.weight_image = w["ImageLocality"]
        cfg.weight_topology_spread = w["PodTopologySpread"]
        cfg.weight_inter_pod_affinity = w["InterPodAffinity"]
        cfg.hard_pod_affinity_weight = hard_pod_affinity_weight
        cfg.percentage_of_nodes_to_score = percentage_of_nodes_to_score
        self.weights = w
        # the node capacity, as it always was (an int: range(s.capacity), ctypes array sizes), which is also the
        # capacity query: s.capacity(pod, per_node=False)
        self.capacity = _NodeCapacity(node_capacity)
        self.capacity.query = self._capacity_of
        self.ctx = C.c_void_p()
        st = self.lib.ks_open(C.byref(cfg), C.byref(self.ctx))
        if st != 0:
            raise _abi.KschedError(st, "ks_open failed (no usable HIP device?)")
        self.names: Dict[int, str] = {}
        self.slots: Dict[str, int] = {}
        self.slot_gen: Dict[int, int] = {}  # last NodeInfo.Generation applied per slot (snapshot_update)
        if fit_strategy != "LeastAllocated" or fit_resource_weights is not None or fit_shape is not None:
            try:
                self.set_fit_strategy(fit_strategy, fit_resource_weights, fit_shape)
            except Exception:
                self.close()
                raise
        if balanced_resources is not None:
            try:
                self.set_balanced_resources(balanced_resources)
            except Exception:
                self.close()
                raise

    def set_balanced_resources(self, resources=None):
        """NodeResourcesBalancedAllocationArgs.resources: the ordered names the
        plugin balances, e.g. ["cpu", "memory", "amd.com/gpu"]; a scalar
        resource is scored for the pods that request it, and the order is the
        float64 summation order.  None or an empty list restores ["cpu",
        "memory"].  Applies to every batch run after the call
        (ks_set_balanced_resources, which judges the names)."""
        names = [str(r).encode() for r in (resources or [])]
        arr = (C.c_char_p * max(1, len(names)))(*names)
        self._ok(self.lib.ks_set_balanced_resources(self.ctx, arr if names else None, len(names)))

    def get_balanced_resources(self):
        """The list in force, ["cpu", "memory"] by default."""
        arr = (C.c_char_p * _abi.BALANCED_MAX_RESOURCES)()
        n = C.c_uint32()
        self._ok(self.lib.ks_get_balanced_resources(self.ctx, arr, _abi.BALANCED_MAX_RESOURCES, C.byref(n)))
        return [arr[i].decode() for i in range(n.value)]

    def set_fit_strategy(self, strategy: str = "LeastAllocated", resource_weights: Optional[Dict[str, int]] = None,
                         shape=None):
        """NodeResourcesFitArgs.scoringStrategy: type "LeastAllocated",
        "MostAllocated" or "RequestedToCapacityRatio", resources {"cpu": w,
        "memory": w} (1..100 each; a resource left out is not scored; default
        both 1); further names are scalar resources, {"amd.com/gpu": 3}, scored
        for the pods that request them (ks_set_fit_strategy_resources, which
        judges the names).  RequestedToCapacityRatio takes shape, a sequence of
        (utilization 0..100, score 0..10) with strictly increasing
        utilizations, e.g. [(0, 0), (100, 10)] for bin packing; the other two
        take none.  Applies to every batch run after the call
        (ks_set_fit_strategy / ks_set_fit_strategy_shape)."""
        if strategy not in _abi.FIT_TYPES:
            raise ValueError(f"unknown NodeResourcesFit scoring strategy {strategy}")
        w = {"cpu": 1, "memory": 1} if resource_weights is None else dict(resource_weights)
        fs = _abi.KsFitStrategy(_abi.FIT_TYPES[strategy], int(w.get("cpu", 0)), int(w.get("memory", 0)), 0)
        ext = [(str(k), int(v)) for k, v in w.items() if k not in ("cpu", "memory")]
        if ext:  # scalar resources in the list: the library judges the names
            pts = [] if shape is None else [(int(u), int(v)) for u, v in shape]
            arr = (_abi.KsFitShapePoint * max(1, len(pts)))(*[_abi.KsFitShapePoint(u, v) for u, v in pts])
            res = (_abi.KsFitResource * len(ext))(*[_abi.KsFitResource(k.encode(), v, 0) for k, v in ext])
            self._ok(self.lib.ks_set_fit_strategy_resources(self.ctx, C.byref(fs), None if shape is None else arr,
                                                            len(pts), res, len(ext)))
            return
        if shape is None:
            # (RequestedToCapacityRatio without a shape: KS_ERR_INVALID, the library's answer)
            self._ok(self.lib.ks_set_fit_strategy(self.ctx, C.byref(fs)))
            return
        pts = [(int(u), int(v)) for u, v in shape]
        arr = (_abi.KsFitShapePoint * max(1, len(pts)))(*[_abi.KsFitShapePoint(u, v) for u, v in pts])
        self._ok(self.lib.ks_set_fit_strategy_shape(self.ctx, C.byref(fs), arr, len(pts)))

    def get_fit_shape(self):
        """The RequestedToCapacityRatio shape in force as [(utilization, score)];
        [] under the other two strategies."""
        arr = (_abi.KsFitShapePoint * _abi.FIT_SHAPE_MAX_POINTS)()
        n = C.c_uint32()
        self._ok(self.lib.ks_get_fit_shape(self.ctx, arr, _abi.FIT_SHAPE_MAX_POINTS, C.byref(n)))
        return [(int(arr[i].utilization), int(arr[i].score)) for i in range(n.value)]

    def get_fit_strategy(self):
        """(strategy name, {"cpu": w, "memory": w}) in force; the dict also
        carries the extended resources when the strategy lists any."""
        fs = _abi.KsFitStrategy()
        self._ok(self.lib.ks_get_fit_strategy(self.ctx, C.byref(fs)))
        name = next(k for k, v in _abi.FIT_TYPES.items() if v == fs.type)
        w = {"cpu": int(fs.weight_cpu), "memory": int(fs.weight_memory)}
        res = (_abi.KsFitResource * _abi.FIT_MAX_RESOURCES)()
        n = C.c_uint32()
        self._ok(self.lib.ks_get_fit_resources(self.ctx, res, _abi.FIT_MAX_RESOURCES, C.byref(n)))
        for i in range(n.value):
            w[res[i].name.decode()] = int(res[i].weight)
        return name, w

    def next_start_index(self) -> int:
        """Scheduler.nextStartNodeIndex (percentageOfNodesToScore < 100)."""
        v = C.c_uint64()
        _check(self.lib, self.ctx, self.lib.ks_next_start_index(self.ctx, C.byref(v)))
        return int(v.value)

    # ------------------------------------------------------------ lifecycle
    def close(self):
        if self.ctx:
            self.lib.ks_close(self.ctx)
            self.ctx = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _ok(self, st):
        _check(self.lib, self.ctx, st)

    # ------------------------------------------------- node cache (informer)
    def upsert_nodes(self, nodes: Sequence[Node], slots: Optional[Sequence[int]] = None):
        """AddNode / UpdateNode for k8s-shaped nodes; returns their slots."""
        if slots is None:
            slots = [self.slots.get(n.name, None) for n in nodes]
            free = (s for s in range(self.capacity) if s not in self.names)
            slots = [s if s is not None else next(free) for s in slots]
        a = Arena()
        arr, n = nodes_array(list(nodes), a)
        sl = (C.c_uint32 * max(1, n))(*slots)
        self._ok(self.lib.ks_nodes_upsert(self.ctx, arr, sl, n))
        for node, s in zip(nodes, slots):
            old = self.names.get(s)
            if old is not None:
                self.slots.pop(old, None)
            self.names[s] = node.name
            self.slots[node.name] = s
        return list(slots)

    def upsert_nodes_raw(self, arr, slots, n: int, names: Optional[Sequence[str]] = None):
        self._ok(self.lib.ks_nodes_upsert(self.ctx, arr, slots, n))

    def snapshot_update(self, items):
        """Cache.UpdateSnapshot: items = [(slot, generation, Node or None for
        RemoveNode)]; returns (snapshot generation, items applied).

        The slot -> name mirror follows what ks_snapshot_update applies, not
        every item it is handed: per slot only the highest generation above
        the slot's last applied one counts (stale or replayed items are
        skipped), deletions go first, and an upsert that renames a slot drops
        the old name's reverse entry."""
        a = Arena()
        live = [(sl, g, nd) for sl, g, nd in items]
        arr, _ = nodes_array([nd for _, _, nd in live if nd is not None], a) if any(
            nd is not None for _, _, nd in live) else (None, 0)
        infos = (_abi.KsNodeInfo * max(1, len(live)))()
        k = 0
        for i, (sl, g, nd) in enumerate(live):
            infos[i].slot, infos[i].generation = sl, g
            if nd is None:
                infos[i].deleted = 1
            else:
                infos[i].node = C.pointer(arr[k])
                k += 1
        # the items the library will apply (its filter, restated)
        best: Dict[int, int] = {}
        for i, (sl, g, nd) in enumerate(live):
            if g <= self.slot_gen.get(sl, -(1 << 63)):
                continue
            if sl not in best or live[best[sl]][1] < g:
                best[sl] = i
        order = sorted(best.values())
        gen, applied = C.c_int64(), C.c_uint32()
        try:
            self._ok(self.lib.ks_snapshot_update(self.ctx, infos, len(live), C.byref(gen), C.byref(applied)))
        except _abi.KschedError as e:
            if "deletions were applied" in str(e):  # the upserts failed after the deletions went in
                self._mirror_snapshot([i for i in order if live[i][2] is None], live)
            raise
        self._mirror_snapshot(order, live)
        return gen.value, applied.value

    def _mirror_snapshot(self, order, live):
        for i in order:  # deletions first, as the library applies them
            sl, g, nd = live[i]
            if nd is None:
                old = self.names.pop(sl, None)
                if old is not None and self.slots.get(old) == sl:
                    self.slots.pop(old, None)
        for i in order:
            sl, g, nd = live[i]
            if nd is not None:
                old = self.names.get(sl)
                if old is not None and old != nd.name and self.slots.get(old) == sl:
                    self.slots.pop(old, None)
                self.names[sl] = nd.name
                self.slots[nd.name] = sl
        for i in order:
            self.slot_gen[live[i][0]] = live[i][1]

    def delete_nodes(self, names: Sequence[str]):
        slots = [self.slots[n] for n in names]
        sl = (C.c_uint32 * max(1, len(slots)))(*slots)
        self._ok(self.lib.ks_nodes_delete(self.ctx, sl, len(slots)))
        for n, s in zip(names, slots):
            self.slots.pop(n, None)
            self.names.pop(s, None)

    def delete_slots(self, slots: Sequence[int]):
        sl = (C.c_uint32 * max(1, len(slots)))(*slots)
        self._ok(self.lib.ks_nodes_delete(self.ctx, sl, len(slots)))
        for s in slots:
            n = self.names.pop(s, None)
            if n is not None:
                self.slots.pop(n, None)

    def _pods_event(self, fn, pods: Sequence[Pod], slots: Sequence[int]):
        a = Arena()
        arr, n = pods_array(list(pods), a)
        sl = (C.c_uint32 * max(1, n))(*slots)
        self._ok(fn(self.ctx, arr, sl, n))

    def add_pods(self, pods: Sequence[Pod], slots: Sequence[int]):
        """NodeInfo.AddPod for pods already bound to (or assumed on) nodes."""
        self._pods_event(self.lib.ks_pods_add, pods, slots)

    def remove_pods(self, pods: Sequence[Pod], slots: Sequence[int]):
        """NodeInfo.RemovePod (pod deleted / ForgetPod)."""
        self._pods_event(self.lib.ks_pods_remove, pods, slots)

    # --------------------------------------------------------- scheduling
    def _results(self, raw, n) -> List[Union[ScheduleResult, FitError, FrameworkError]]:
        out = []
        for i in range(n):
            r = raw[i]
            if r.status == 0:
                out.append(ScheduleResult(self.names.get(r.node_index, str(r.node_index)), r.evaluated_nodes,
                                          r.feasible_nodes, r.node_index, r.total_score, bool(r.flags & 1)))
            elif r.status == 1:
                counts = {FILTER_PLUGINS[k]: int(r.fail_counts[k]) for k in range(7) if r.fail_counts[k]}
                if r.fail_node_ports:  # nodes whose first failing plugin is NodePorts (ks_result.fail_node_ports)
                    counts["NodePorts"] = int(r.fail_node_ports)
                out.append(FitError(f"pod#{i}", r.evaluated_nodes, Diagnosis(counts, set(counts))))
            else:
                out.append(FrameworkError(f"pod#{i}: plugin Error status"))
        return out

    def schedule_pods(self, pods: Sequence[Pod]):
        """Sequential schedulePod + assume for each pod, in queue order."""
        a = Arena()
        arr, n = pods_array(list(pods), a)
        raw = (_abi.KsResult * max(1, n))()
        self._ok(self.lib.ks_schedule(self.ctx, arr, n, raw))
        return self._results(raw, n)

    def schedule_raw(self, arr, n: int):
        raw = (_abi.KsResult * max(1, n))()
        self._ok(self.lib.ks_schedule(self.ctx, arr, n, raw))
        return raw

    def schedule_pod(self, state: CycleState, pod: Pod) -> ScheduleResult:
        """The ``SchedulePod`` hook: schedule one pod, assume it, write NodePluginScoresState."""
        res = self.schedule_pods([pod])[0]
        if isinstance(res, Exception):
            raise res
        state.write(NODE_PLUGIN_SCORES_STATE_KEY, NodePluginScoresState(
            [NodePluginScores(res.suggested_host, [], res.total_score)]))
        return res

    def plugin_scores(self, pod: Pod) -> List[_abi.KsNodeScore]:
        a = Arena()
        arr, _ = pods_array([pod], a)
        out = (_abi.KsNodeScore * self.capacity)()
        self._ok(self.lib.ks_plugin_scores(self.ctx, arr, out))
        return list(out)

    def diagnose(self, pod: Pod) -> FitDiagnosis:
        """Why the pod has no node, as upstream's FitError tells it: the nodes
        carrying each status reason, counted by one pass on the device against
        the cache as it is (ks_diagnose).  Nothing is committed; it also
        answers for a pod that has feasible nodes."""
        a = Arena()
        arr, _ = pods_array([pod], a)
        d = _abi.KsDiagnosis()
        out = (_abi.KsReason * _abi.DIAG_MAX_REASONS)()
        n = C.c_uint32()
        self._ok(self.lib.ks_diagnose(self.ctx, arr, C.byref(d), out, _abi.DIAG_MAX_REASONS, C.byref(n)))
        rows = [(out[i].reason.decode(), int(out[i].count)) for i in range(n.value)]
        reasons: Dict[str, int] = {}
        for r, c in rows:
            reasons[r] = reasons.get(r, 0) + c
        pm = d.prefilter_msg.decode() if d.prefilter_msg else None
        return FitDiagnosis(int(d.num_all_nodes), int(d.feasible_nodes), [int(v) for v in d.plugin_nodes],
                            int(d.node_ports_nodes), reasons, pm, fit_error_message(int(d.num_all_nodes), rows, pm))

    def diagnose_many(self, pods: Sequence[Pod], strict: bool = True) -> List[Optional[FitDiagnosis]]:
        """``diagnose`` for a list of pods in one call (ks_diagnose_pods): one
        compile, one upload and one wait; every entry is what ``diagnose``
        returns for that pod against the cache as the call finds it.  A pod the
        library refuses raises KschedError when ``strict``; otherwise its entry
        is None and the rest are still answered."""
        a = Arena()
        arr, n = pods_array(list(pods), a)
        out = (_abi.KsPodDiagnosis * max(1, n))()
        cap = max(1, n) * _abi.DIAG_MAX_REASONS
        rows = (_abi.KsReason * cap)()
        total = C.c_uint32()
        st = self.lib.ks_diagnose_pods(self.ctx, arr, n, out, rows, cap, C.byref(total))
        if st != 0 and (strict or not any(out[i].status == st for i in range(n))):
            self._ok(st)
        res: List[Optional[FitDiagnosis]] = []
        for i in range(n):
            if out[i].status != 0:
                res.append(None)
                continue
            d, lo = out[i].d, out[i].first_reason
            mine = [(rows[lo + k].reason.decode(), int(rows[lo + k].count)) for k in range(d.n_reasons)]
            reasons: Dict[str, int] = {}
            for r, c in mine:
                reasons[r] = reasons.get(r, 0) + c
            pm = d.prefilter_msg.decode() if d.prefilter_msg else None
            res.append(FitDiagnosis(int(d.num_all_nodes), int(d.feasible_nodes), [int(v) for v in d.plugin_nodes],
                                    int(d.node_ports_nodes), reasons, pm,
                                    fit_error_message(int(d.num_all_nodes), mine, pm)))
        return res

    def diagnose_pods_counters(self) -> List[int]:
        """ks_debug_diagnose_pods: which paths the last ``diagnose_many`` took."""
        out = (C.c_uint64 * 8)()
        self._ok(self.lib.ks_debug_diagnose_pods(self.ctx, out))
        return [int(v) for v in out]

    @staticmethod
    def _capacity(c: _abi.KsCapacity, per_node=None) -> Capacity:
        names = {_abi.CAP_PODS: "pods", _abi.CAP_CPU: "cpu", _abi.CAP_MEMORY: "memory", _abi.CAP_PORTS: "ports"}
        bound: Dict[str, int] = {}
        for b in range(_abi.CAP_BOUNDS):
            if not c.bound_by[b]:
                continue
            if b >= _abi.CAP_X:
                x = c.x_names[b - _abi.CAP_X]
                name = x.decode() if x else f"x{b - _abi.CAP_X}"
            else:
                name = names[b]
            bound[name] = bound.get(name, 0) + int(c.bound_by[b])
        return Capacity(int(c.num_all_nodes), int(c.eligible_nodes), int(c.nodes_with_room), int(c.max_per_node),
                        int(c.replicas), bound, per_node)

    def _capacity_of(self, pod: Pod, per_node: bool = False) -> Capacity:
        """``Scheduler.capacity(pod, per_node=False)``: how many more replicas
        of the pod the cluster holds and what runs out first, from one pass on
        the device against the cache as it is (ks_capacity_pod).  Nothing is
        committed.  With ``per_node`` the result carries the count of every
        slot as a numpy uint32 array."""
        a = Arena()
        arr, _ = pods_array([pod], a)
        c = _abi.KsCapacity()
        pn = None
        ptr = None
        if per_node:
            import numpy as np

            pn = np.zeros(int(self.capacity), dtype=np.uint32)
            ptr = pn.ctypes.data_as(C.POINTER(C.c_uint32))
        self._ok(self.lib.ks_capacity_pod(self.ctx, arr, C.byref(c), ptr))
        return self._capacity(c, pn)

    def capacity_many(self, pods: Sequence[Pod], strict: bool = True) -> List[Optional[Capacity]]:
        """``capacity`` for a list of pods in one call (ks_capacity_pods), each
        pod answered on its own (not the joint capacity of the mix).  A pod the
        library refuses raises KschedError when ``strict``; otherwise its entry
        is None and the rest are still answered."""
        a = Arena()
        arr, n = pods_array(list(pods), a)
        out = (_abi.KsPodCapacity * max(1, n))()
        st = self.lib.ks_capacity_pods(self.ctx, arr, n, out)
        if st != 0 and (strict or not any(out[i].status == st for i in range(n))):
            self._ok(st)
        return [None if out[i].status != 0 else self._capacity(out[i].c) for i in range(n)]

    def capacity_counters(self) -> List[int]:
        """ks_debug_capacity: which paths the last ``capacity`` / ``capacity_many`` took."""
        out = (C.c_uint64 * 8)()
        self._ok(self.lib.ks_debug_capacity(self.ctx, out))
        return [int(v) for v in out]

    def explain(self, pod: Pod, k: int = 16) -> Explanation:
        """Why this node, and what were the alternatives: the pod's k feasible
        nodes with the highest TotalScore and their per-plugin scores, selected
        on the device against the cache as it is (ks_explain).  Nothing is
        committed.  ``candidates[0]`` is the node ``schedule_pod`` would pick
        (percentageOfNodesToScore 100); ``top_score_nodes`` of them tie for it,
        among which upstream's selectHost picks at random."""
        a = Arena()
        arr, _ = pods_array([pod], a)
        e = _abi.KsExplanation()
        out = (_abi.KsCandidate * max(1, k))()
        self._ok(self.lib.ks_explain(self.ctx, arr, k, C.byref(e), out))
        cands = []
        for i in range(e.n_candidates):
            sc = _abi.KsNodeScore.from_buffer_copy(out[i].score)
            cands.append(NodePluginScores(
                self.names.get(out[i].slot, str(out[i].slot)),
                [PluginScore(p, int(getattr(sc, f))) for p, f in SCORE_FIELDS.items()],
                int(sc.total_score), int(out[i].slot), sc))
        return Explanation(int(e.num_all_nodes), int(e.feasible_nodes), int(e.top_score), int(e.top_score_nodes), cands)

    def node_states(self, slots: Sequence[int]) -> List[_abi.KsNodeState]:
        sl = (C.c_uint32 * max(1, len(slots)))(*slots)
        out = (_abi.KsNodeState * max(1, len(slots)))()
        self._ok(self.lib.ks_node_states(self.ctx, sl, len(slots), out))
        return list(out)[: len(slots)]

    def node_used_ports(self, slot: int) -> List[tuple]:
        """NodeInfo.UsedPorts of a slot, sanitised: [(hostIP, protocol, hostPort)]
        (ks_node_used_ports; the device column's entries)."""
        out = (_abi.KsHostPort * _abi.MAX_PORT_ENTRIES)()
        n = C.c_uint32()
        self._ok(self.lib.ks_node_used_ports(self.ctx, slot, out, _abi.MAX_PORT_ENTRIES, C.byref(n)))
        return [(out[i].host_ip.decode(), out[i].protocol.decode(), int(out[i].host_port)) for i in range(n.value)]

    # ---------------------------------------------------------- batches
    def prepare(self, arr, n: int):
        b = C.c_void_p()
        self._ok(self.lib.ks_batch_prepare(self.ctx, arr, n, C.byref(b)))
        return b

    def run(self, batch):
        self._ok(self.lib.ks_batch_run(self.ctx, batch))

    def results(self, batch, n: int):
        raw = (_abi.KsResult * max(1, n))()
        self._ok(self.lib.ks_batch_results(self.ctx, batch, raw))
        return raw

    def marks(self, batch, n: int) -> bytes:
        """Per-pod round marks of a finished batch (ks_batch_marks: KS_MARK_* bits)."""
        out = (C.c_uint8 * max(1, n))()
        self._ok(self.lib.ks_batch_marks(self.ctx, batch, out))
        return bytes(out)[:n]

    def forget(self, batch, indices: Sequence[int]) -> int:
        """Cache.ForgetPod for pods ``batch`` placed (ks_batch_forget): ``indices``
        are batch indices, strictly increasing (a numpy uint32 array is passed
        as it is).  Returns how many were skipped because their node has left
        since the batch ran."""
        n = len(indices)
        if hasattr(indices, "ctypes"):  # a numpy array
            arr = indices.astype("uint32", order="C", copy=False)
            ptr = arr.ctypes.data_as(C.POINTER(C.c_uint32))
        else:
            arr = (C.c_uint32 * max(1, n))(*indices)
            ptr = arr
        skipped = C.c_uint32()
        self._ok(self.lib.ks_batch_forget(self.ctx, batch, ptr, n, C.byref(skipped)))
        return int(skipped.value)

    def forget_counters(self) -> List[int]:
        """ks_debug_forget: the last ``forget`` ([0] pods taken back, [1] skipped,
        [2] of [0] with a one-pod program, [3] launches of the forget kernel)."""
        out = (C.c_uint64 * 8)()
        self._ok(self.lib.ks_debug_forget(self.ctx, out))
        return [int(v) for v in out]

    def free(self, batch):
        self.lib.ks_batch_free(self.ctx, batch)

    # ---------------------------------------------------------- measurement
    def set_timing(self, on: bool):
        self._ok(self.lib.ks_set_timing(self.ctx, 1 if on else 0))

    def stats(self) -> _abi.KsStats:
        s = _abi.KsStats()
        self._ok(self.lib.ks_get_stats(self.ctx, C.byref(s)))
        return s

    def debug_topology(self, key: str):
        """(domain ids, scratch entries per constraint, renumberings, domains of
        two or more nodes) of a topology key's column (ks_debug_topology); all
        zero while no constraint or term has named the key."""
        out = (C.c_uint64 * 4)()
        self._ok(self.lib.ks_debug_topology(self.ctx, key.encode(), out))
        return tuple(int(v) for v in out)

    def reset_stats(self):
        self._ok(self.lib.ks_reset_stats(self.ctx))

    # ---------------------------------------------------------- multi-GPU
    @staticmethod
    def comm_unique_id() -> bytes:
        lib = _abi.ksched_lib()
        buf = (C.c_uint8 * 128)()
        st = lib.ks_comm_unique_id(buf)
        if st != 0:
            raise _abi.KschedError(st, "ncclGetUniqueId failed")
        return bytes(buf)

    def comm_init(self, uid: bytes):
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        self._ok(self.lib.ks_comm_init(self.ctx, buf))

    @staticmethod
    def comm_init_local(scheds: Sequence["Scheduler"]):
        """In-process communicator over contexts of this process (rank r =
        scheds[r]; one GPU may hold them all): the multi-rank path without
        RCCL, for tests.  Each rank must then be driven from its own thread."""
        lib = _abi.ksched_lib()
        arr = (C.c_void_p * len(scheds))(*[s.ctx.value for s in scheds])
        st = lib.ks_comm_init_local(arr, len(scheds))
        if st != 0:
            raise _abi.KschedError(st, lib.ks_last_error(scheds[0].ctx).decode())

    def allreduce_max(self, values):
        """Element-wise max over ranks (RCCL); doubles as a barrier."""
        arr = (C.c_double * max(1, len(values)))(*values)
        self._ok(self.lib.ks_comm_allreduce_max(self.ctx, arr, len(values)))
        return list(arr)[: len(values)]


def results_to_arrays(raw, n: int):
    """(node_index[int32], total_score[int64], status[int32], feasible[uint32]) numpy views."""
    import numpy as np

    buf = np.frombuffer(C.string_at(C.addressof(raw), n * C.sizeof(_abi.KsResult)), dtype=np.uint8)
    dt = np.dtype([("node_index", "<i4"), ("status", "<i4"), ("total_score", "<i8"), ("feasible", "<u4"),
                   ("evaluated", "<u4"), ("fail", "<u4", (8,)), ("flags", "<u4"), ("_pad", "<u4")])
    return buf.view(dt)
