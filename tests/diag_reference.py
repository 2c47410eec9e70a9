"""Reference for ks_diagnose: the reasons of every node's status for one pod,
as upstream v1.31.3's FitError counts them, restated in plain Python over
ksched.objects Nodes and Pods.  Nothing here comes from the product code.

A node's FIRST FAILING PLUGIN comes from the existing reference stack
(pyoracle's plugin_scores under PortsReference, which adds NodePorts); the
reasons of that plugin come from this file's own bookkeeping -- the node's
taints in their order, its allocatable and the reference's node states, the
scalar resources its bound pods request, its labels, and the pods bound to
every node:

  NodeUnschedulable / NodeName / NodeAffinity / NodePorts / PreFilterResult
      one fixed string each; NodeAffinity's PreFilter conflict ("pod affinity
      terms conflict") when every node fails NodeAffinity for a pod whose
      required terms all name nodes by matchFields and none can match
  TaintToleration   v1helper.FindMatchingUntoleratedTaint: the first taint
      with effect NoSchedule / NoExecute, in the node's order, that no
      toleration tolerates
  NodeResourcesFit  fitsRequest: "Too many pods" when len(Pods) + 1 >
      allowed; nothing more for a pod requesting nothing; else every resource
      with request > 0 and request > Allocatable - Requested
  PodTopologySpread filtering.go#Filter: the first DoNotSchedule constraint,
      in order, whose key the node lacks (missing required label) or whose skew
      matchNum + selfMatch - minMatchNum exceeds maxSkew; calPreFilterState
      restated (required keys, inclusion policies, minDomains)
  InterPodAffinity  the first failing of satisfyPodAffinity,
      satisfyPodAntiAffinity, satisfyExistingPodsAntiAffinity

The reason strings are the issue's transcription of v1.31.3, written out again
here (not imported).  A node counts once per reason it carries."""
import ctypes as C

import numpy as np

from ksched import _abi
from ksched.objects import Arena, nodes_array, pods_array
from ports_reference import PortsReference

UNSCHEDULABLE = "node(s) were unschedulable"
NODE_NAME = "node(s) didn't match the requested node name"
TAINT = "node(s) had untolerated taint {%s: %s}"
AFFINITY = "node(s) didn't match Pod's node affinity/selector"
CONFLICT = "pod affinity terms conflict"
PREFILTERED = "node is filtered out by the prefilter result"
PORTS = "node(s) didn't have free ports for the requested pod ports"
TOO_MANY_PODS = "Too many pods"
INSUFFICIENT = "Insufficient %s"
SPREAD_LABEL = "node(s) didn't match pod topology spread constraints (missing required label)"
SPREAD_SKEW = "node(s) didn't match pod topology spread constraints"
IPA_AFF = "node(s) didn't match pod affinity rules"
IPA_ANTI = "node(s) didn't match pod anti-affinity rules"
IPA_EXIST = "node(s) didn't satisfy existing pods anti-affinity rules"


def u32(xs):
    return (C.c_uint32 * max(1, len(xs)))(*xs)


# ------------------------------------------------------------------ taints
def tolerates(tol, taint):
    """v1.Toleration.ToleratesTaint."""
    if tol.effect and tol.effect != taint.effect:
        return False
    if tol.key and tol.key != taint.key:
        return False
    if tol.operator == "Exists":
        return True
    return tol.operator in ("", "Equal") and tol.value == taint.value


def first_untolerated(node, pod):
    for t in node.taints:
        if t.effect in ("NoSchedule", "NoExecute") and not any(tolerates(tol, t) for tol in pod.tolerations):
            return t
    return None


# ---------------------------------------------------------------- requests
def pod_requests(pod):
    """resourcehelper.PodRequests: containers summed, init containers' running
    maximum (sidecars add to both), plus overhead; every resource name."""
    def add(d, r):
        for k, v in r.items():
            d[k] = d.get(k, 0) + v
    total, side, init = {}, {}, {}
    for c in pod.containers:
        add(total, c.requests)
    for c in pod.init_containers:
        if c.restart_policy_always:
            add(total, c.requests)
            add(side, c.requests)
            use = dict(side)
        else:
            use = dict(side)
            add(use, c.requests)
        for k, v in use.items():
            init[k] = max(init.get(k, 0), v)
    for k, v in init.items():
        total[k] = max(total.get(k, 0), v)
    add(total, pod.overhead or {})
    return total


# --------------------------------------------------------------- selectors
def selector_matches(sel, labels):
    """metav1.LabelSelector as a selector: None is Nothing(), an empty one Everything()."""
    if sel is None:
        return False
    for k, v in sel.match_labels.items():
        if labels.get(k) != v:
            return False
    for r in sel.match_expressions:
        has = r.key in labels
        if r.operator == "In" and not (has and labels[r.key] in r.values):
            return False
        if r.operator == "NotIn" and has and labels[r.key] in r.values:
            return False
        if r.operator == "Exists" and not has:
            return False
        if r.operator == "DoesNotExist" and has:
            return False
    return True


def selector_empty(sel):
    return sel is not None and not sel.match_labels and not sel.match_expressions


def node_term_matches(term, node):
    """One NodeSelectorTerm (an empty one matches nothing)."""
    if not term.match_expressions and not term.match_fields:
        return False
    for r in term.match_expressions:
        has = r.key in node.labels
        v = node.labels.get(r.key)
        if r.operator == "In":
            ok = has and v in r.values
        elif r.operator == "NotIn":
            ok = not (has and v in r.values)
        elif r.operator == "Exists":
            ok = has
        elif r.operator == "DoesNotExist":
            ok = not has
        else:  # Gt / Lt: one integer value
            try:
                ok = has and len(r.values) == 1 and (int(v) > int(r.values[0]) if r.operator == "Gt"
                                                     else int(v) < int(r.values[0]))
            except ValueError:
                ok = False
        if not ok:
            return False
    for r in term.match_fields:
        assert r.key == "metadata.name" and r.operator in ("In", "NotIn")
        if len(r.values) != 1:  # a field selector takes one value: the term fails to parse and never matches
            return False
        if (node.name in r.values) != (r.operator == "In"):
            return False
    return True


def required_affinity_matches(pod, node):
    """nodeaffinity.GetRequiredNodeAffinity(pod).Match(node)."""
    if any(node.labels.get(k) != v for k, v in pod.node_selector.items()):
        return False
    if pod.required_terms is None:
        return True
    return any(node_term_matches(t, node) for t in pod.required_terms)


def affinity_conflict(pod):
    """nodeaffinity.PreFilter: every required term names nodes through
    matchFields metadata.name In (a term's several name sets intersect), and
    the union of the terms' name sets is empty."""
    if not pod.required_terms:
        return False
    names = set()
    for t in pod.required_terms:
        sets = [set(r.values) for r in t.match_fields if r.key == "metadata.name" and r.operator == "In"]
        if not sets:
            return False  # a term without a name set: no PreFilterResult at all
        names |= set.intersection(*sets)
    return not names


# ------------------------------------------------------------ the reference
class DiagReference:
    """The reference stack plus the Python-side cluster (nodes by slot, bound pods by slot)."""

    def __init__(self, capacity, pairs=(), ips=(), **kw):
        self.n = capacity
        self.o = PortsReference(capacity, pairs, ips, **kw)
        self.a = Arena()
        self.nodes = {}   # slot -> Node
        self.bound = {}   # slot -> [Pod]

    def close(self):
        self.o.close()

    # ---- cache events
    def upsert(self, nodes, slots):
        na, k = nodes_array(list(nodes), self.a)
        self.o.upsert(na, u32(slots), k)
        for nd, s in zip(nodes, slots):
            self.nodes[s] = nd
            self.bound.setdefault(s, [])

    def delete(self, slots):
        self.o.delete(u32(slots), len(slots))
        for s in slots:
            self.nodes.pop(s, None)
            self.bound.pop(s, None)

    def add(self, pods, slots, sign=1):
        if not pods:
            return
        pa, k = pods_array(list(pods), self.a)
        (self.o.add_pods if sign > 0 else self.o.remove_pods)(pa, u32(slots), k)
        for p, s in zip(pods, slots):
            if sign > 0:
                self.bound[s].append(p)
            else:
                self.bound[s] = [q for q in self.bound[s] if q is not p]

    def schedule(self, pods):
        """schedulePod + assume for each pod in order; the ks_result array."""
        pa, m = pods_array(list(pods), self.a)
        out = (_abi.KsResult * max(1, m))()
        for i, p in enumerate(pods):
            out[i] = self.o.schedule_one(C.cast(C.addressof(pa[i]), C.POINTER(_abi.KsPod)))
            if out[i].status == 0:
                self.bound[int(out[i].node_index)].append(p)
        return out

    def statuses(self, pod):
        """Per slot: -2 empty, -1 feasible, else the first failing plugin (8 NodePorts, 7 outside the PreFilterResult)."""
        pa, _ = pods_array([pod], self.a)
        return self.o.plugin_scores(pa)["status"].astype(np.int64)

    # ---- reasons
    def fit_reasons(self, pod, slot, state):
        nd = self.nodes[slot]
        out = []
        if int(state["pod_count"]) + 1 > int(nd.allocatable.get("pods", 0)):
            out.append(TOO_MANY_PODS)
        req = {k: v for k, v in pod_requests(pod).items() if v > 0}
        if not req:
            return out
        xreq = {}
        for q in self.bound[slot]:
            for k, v in pod_requests(q).items():
                xreq[k] = xreq.get(k, 0) + v
        for name in ["cpu", "memory"] + sorted(k for k in req if k not in ("cpu", "memory")):
            if name not in req:
                continue
            if name == "cpu":
                free = int(state["alloc_cpu"]) - int(state["req_cpu"])
            elif name == "memory":
                free = int(state["alloc_mem"]) - int(state["req_mem"])
            else:
                free = int(nd.extended.get(name, 0)) - xreq.get(name, 0)
            if req[name] > free:
                out.append(INSUFFICIENT % name)
        return out

    def _spread_state(self, pod):
        """calPreFilterState: per DoNotSchedule constraint {domain value: matchNum} over the eligible nodes."""
        cons = [c for c in pod.topology_spread if c.when_unsatisfiable == "DoNotSchedule"]
        keys = [c.topology_key for c in cons]
        counts = [dict() for _ in cons]
        sels = []
        for c in cons:
            sel = c.label_selector
            if sel is not None and c.match_label_keys:
                from ksched.objects import LabelSelector, LabelSelectorRequirement
                extra = [LabelSelectorRequirement(k, "In", [pod.labels[k]]) for k in c.match_label_keys if k in pod.labels]
                sel = LabelSelector(dict(sel.match_labels), list(sel.match_expressions) + extra)
            sels.append(sel)
        for slot, nd in self.nodes.items():
            if any(k not in nd.labels for k in keys):
                continue
            for i, c in enumerate(cons):
                if (c.node_affinity_policy or "Honor") == "Honor" and not required_affinity_matches(pod, nd):
                    continue
                if (c.node_taints_policy or "Ignore") == "Honor" and first_untolerated(nd, pod) is not None:
                    continue
                sel = sels[i]
                cnt = 0
                if sel is not None and not selector_empty(sel):  # countPodsMatchSelector: Empty() counts nothing
                    cnt = sum(1 for q in self.bound[slot] if q.namespace == pod.namespace and selector_matches(sel, q.labels))
                v = nd.labels[c.topology_key]
                counts[i][v] = counts[i].get(v, 0) + cnt
        return cons, sels, counts

    def spread_reason(self, pod, slot, st):
        cons, sels, counts = st
        nd = self.nodes[slot]
        for i, c in enumerate(cons):
            if c.topology_key not in nd.labels:
                return SPREAD_LABEL
            dom = counts[i]
            min_match = min(dom.values()) if dom else 0  # (no eligible domain: criticalPaths stay at MaxInt32 ...
            if not dom:
                min_match = (1 << 31) - 1                 # ... so no skew can exceed maxSkew)
            if len(dom) < (c.min_domains or 1):
                min_match = 0
            self_match = 1 if sels[i] is not None and selector_matches(sels[i], pod.labels) else 0
            if dom.get(nd.labels[c.topology_key], 0) + self_match - min_match > c.max_skew:
                return SPREAD_SKEW
        raise AssertionError(f"slot {slot}: the reference stack fails PodTopologySpread, the restatement does not")

    @staticmethod
    def term_matches(term, owner, target):
        """framework.AffinityTerm.Matches(target, its namespace's labels) for a term of `owner`."""
        nss = term.namespaces
        if not nss and term.namespace_selector is None:
            nss = [owner.namespace]
        ns_ok = target.namespace in nss or (term.namespace_selector is not None and
                                             selector_matches(term.namespace_selector, target.namespace_labels))
        return ns_ok and selector_matches(term.label_selector, target.labels)

    def _ipa_state(self, pod):
        aff = [t for t in pod.affinity_terms if t.kind == "affinity"]
        anti = [t for t in pod.affinity_terms if t.kind == "anti-affinity"]
        aff_pairs, anti_pairs, exist_pairs = set(), set(), set()
        for slot, nd in self.nodes.items():
            for q in self.bound[slot]:
                if aff and all(self.term_matches(t, pod, q) for t in aff):
                    aff_pairs |= {(t.topology_key, nd.labels[t.topology_key]) for t in aff if t.topology_key in nd.labels}
                for t in anti:
                    if self.term_matches(t, pod, q) and t.topology_key in nd.labels:
                        anti_pairs.add((t.topology_key, nd.labels[t.topology_key]))
                for t in q.affinity_terms:
                    if t.kind == "anti-affinity" and self.term_matches(t, q, pod) and t.topology_key in nd.labels:
                        exist_pairs.add((t.topology_key, nd.labels[t.topology_key]))
        self_ok = bool(aff) and all(self.term_matches(t, pod, pod) for t in aff)
        return aff, anti, aff_pairs, anti_pairs, exist_pairs, self_ok

    def ipa_reason(self, slot, st):
        aff, anti, aff_pairs, anti_pairs, exist_pairs, self_ok = st
        lab = self.nodes[slot].labels
        if aff:
            if any(t.topology_key not in lab for t in aff):
                return IPA_AFF
            if not all((t.topology_key, lab[t.topology_key]) in aff_pairs for t in aff) and not (not aff_pairs and self_ok):
                return IPA_AFF
        if any((t.topology_key, lab.get(t.topology_key)) in anti_pairs for t in anti):
            return IPA_ANTI
        if any((k, v) in exist_pairs for k, v in lab.items()):
            return IPA_EXIST
        raise AssertionError(f"slot {slot}: the reference stack fails InterPodAffinity, the restatement does not")

    def diagnose(self, pod):
        status = self.statuses(pod)
        states = self.o.states()
        conflict = affinity_conflict(pod)
        reasons = {}
        plugin_nodes = [0] * 8
        ports = feasible = 0
        spread = ipa = None

        def count(r):
            reasons[r] = reasons.get(r, 0) + 1
        for slot in sorted(self.nodes):
            s = int(status[slot])
            assert s != -2, slot
            if s == -1:
                feasible += 1
                continue
            if s == 8:
                ports += 1
                count(PORTS)
                continue
            plugin_nodes[s] += 1
            if s == 0:
                count(UNSCHEDULABLE)
            elif s == 1:
                count(NODE_NAME)
            elif s == 2:
                t = first_untolerated(self.nodes[slot], pod)
                assert t is not None, slot
                count(TAINT % (t.key, t.value))
            elif s == 3:
                count(CONFLICT if conflict else AFFINITY)
            elif s == 4:
                rs = self.fit_reasons(pod, slot, states[slot])
                assert rs, f"slot {slot}: the reference stack fails NodeResourcesFit, the restatement does not"
                for r in rs:
                    count(r)
            elif s == 5:
                spread = spread or self._spread_state(pod)
                count(self.spread_reason(pod, slot, spread))
            elif s == 6:
                ipa = ipa or self._ipa_state(pod)
                count(self.ipa_reason(slot, ipa))
            elif s == 7:
                count(PREFILTERED)
        if conflict:
            assert plugin_nodes[3] == len(self.nodes)
        return dict(num_all_nodes=len(self.nodes), feasible_nodes=feasible, plugin_nodes=plugin_nodes,
                    node_ports_nodes=ports, reasons=reasons, prefilter_msg=CONFLICT if conflict else None,
                    message=message(len(self.nodes), reasons, CONFLICT if conflict else None))


def message(num_all_nodes, reasons, prefilter_msg=None):
    """FitError.Error() without the PostFilter part."""
    msg = f"0/{num_all_nodes} nodes are available:"
    if prefilter_msg:
        return msg + f" {prefilter_msg}."
    parts = sorted((f"{c} {r}" for r, c in reasons.items()), key=lambda s: s.encode())
    return msg + (" " + ", ".join(parts) + "." if parts else "")


def same(got, want):
    """A FitDiagnosis (ksched.framework) against this reference's dict; returns the differing fields."""
    return [k for k in want if getattr(got, k) != want[k]]
