"""Reference for the NodePorts filter plugin.

Upstream v1.31.3, restated from the public tree:

  * pkg/scheduler/framework/types.go HostPortInfo: a set of (ip, protocol,
    port).  sanitize: an empty ip is "0.0.0.0", an empty protocol "TCP"; both
    are compared as strings.  Add and Remove ignore port <= 0.  Remove deletes
    the entry outright (no reference count).  CheckConflict(ip, proto, port):
    false for port <= 0; for ip "0.0.0.0" true when any ip's set holds
    (proto, port); otherwise true when the set of "0.0.0.0" or of ip holds it.
  * NodeInfo.updateUsedPorts: the ports of pod.Spec.Containers, on AddPod
    (AssumePod) and RemovePod.
  * plugins/nodeports: PreFilter collects the container ports with HostPort >
    0 (none: the plugin is skipped); Filter fails a node when any of them
    conflicts with NodeInfo.UsedPorts.  Its place in the first-failure order
    is after NodeAffinity and before NodeResourcesFit.

HostPortInfo below is that set in plain Python; nothing here comes from the
product code.

PortsReference gets the exact feasible set by emulation.  The oracle filters
scalar resources in NodeResourcesFit, the plugin right after NodePorts, so
over the test's known universe of ips each (proto, port, ip) maps to a scalar
resource ports.test/<proto>-<port>-<k>, a wildcard want maps to all of that
(proto, port)'s resources plus a -any one, the reference's own copy of every
node has allocatable 1 of each, and the oracle is given a twin of each pod
that requests its de-duplicated resource set on one container.  The feasible
set is then exact, and with it the normalisation maxima, the spread PreScore
counts, the single-feasible-node shortcut and every score downstream (scalar
resources enter no score under the default strategy and lists).  Beside the
emulation runs the mirror, one HostPortInfo per slot; per pod the two must
agree on every node that the pod without its ports passes through
NodeAffinity on.  The results are then rewritten: status 4 with a mirror
conflict becomes 8 (KS_STATUS_NODE_PORTS), fail_counts[4] loses those nodes
and fail_node_ports gets them.

The emulation keeps a reference count per resource where HostPortInfo keeps
none, so it is exact only while no two pods bound to one node hold the same
triple; add_pods asserts that (the Remove quirk itself is tested on the mirror
and on the device column alone).

The class sits on top of BaReference (tests/ba_reference.py), so the same
reference serves contexts under another NodeResourcesFit strategy or balanced
list; with the defaults that composition reproduces oracle.schedule.
"""
import ctypes as C

import numpy as np

from ba_reference import BaReference
from fit_reference import pod_at
from ksched import _abi

WILDCARD, TCP = "0.0.0.0", "TCP"
ST_FIT, ST_PORTS = 4, 8  # KS_PLUGIN_NODE_RESOURCES_FIT, KS_STATUS_NODE_PORTS


def sanitize(ip, proto):
    return (ip or WILDCARD), (proto or TCP)


class HostPortInfo:
    """framework.HostPortInfo: {ip: {(protocol, port)}}."""

    def __init__(self):
        self.m = {}

    def add(self, ip, proto, port):
        if port <= 0:
            return
        ip, proto = sanitize(ip, proto)
        self.m.setdefault(ip, set()).add((proto, port))

    def remove(self, ip, proto, port):
        if port <= 0:
            return
        ip, proto = sanitize(ip, proto)
        if ip in self.m:
            self.m[ip].discard((proto, port))
            if not self.m[ip]:
                del self.m[ip]

    def check_conflict(self, ip, proto, port):
        if port <= 0:
            return False
        ip, proto = sanitize(ip, proto)
        if ip == WILDCARD:
            return any((proto, port) in s for s in self.m.values())
        return any((proto, port) in self.m.get(k, ()) for k in (WILDCARD, ip))

    def holds(self, ip, proto, port):
        ip, proto = sanitize(ip, proto)
        return (proto, port) in self.m.get(ip, ())

    def entries(self):
        """Sorted [(ip, protocol, port)]."""
        return sorted((ip, proto, port) for ip, s in self.m.items() for proto, port in s)

    def __len__(self):
        return sum(len(s) for s in self.m.values())


def pod_wants(pod_ptr):
    """The (ip, protocol, port) entries of one ks_pod with port > 0, sanitised, in order."""
    p = pod_ptr[0]
    out = []
    for i in range(p.n_containers):  # Spec.Containers alone: init containers do not count
        c = p.containers[i]
        for k in range(c.n_host_ports):
            hp = c.host_ports[k]
            if hp.host_port > 0:
                ip, proto = sanitize((hp.host_ip or b"").decode(), (hp.protocol or b"").decode())
                out.append((ip, proto, int(hp.host_port)))
    return out


class PortsReference(BaReference):
    """BaReference with NodePorts.  pairs: the universe's (protocol, port)
    pairs; ips: its specific ips (the wildcard needs no entry).  track: record
    for every pod with host ports where the reference would place it with its
    ports stripped, at the same state (self.placed: [(stripped, actual)])."""

    def __init__(self, capacity, pairs, ips=(), track=False, **kw):
        super().__init__(capacity, **kw)
        self.pairs, self.ips = list(pairs), list(ips)
        self.mirror = {}
        self.track, self.placed = track, []
        self._keep = []
        self._twin_wants = {}  # address of a twin's struct -> (the real pod's wants, the real pod)
        self._port_fails = 0
        names = [self.resource(pr, po, k) for pr, po in self.pairs for k in list(range(len(self.ips))) + ["any"]]
        self._node_ext = [(nm.encode(), 1) for nm in names]

    # ---- the emulation's resources
    @staticmethod
    def resource(proto, port, k):
        return f"ports.test/{proto}-{port}-{k}"

    def resources(self, wants):
        """The de-duplicated scalar resources the twin of a pod with `wants` requests."""
        out = []
        for ip, proto, port in wants:
            assert (proto, port) in self.pairs, (proto, port)
            ks = list(range(len(self.ips))) + ["any"] if ip == WILDCARD else [self.ips.index(ip)]
            for k in ks:
                nm = self.resource(proto, port, k)
                if nm not in out:
                    out.append(nm)
        return out

    def _twin(self, pod_ptr):
        """(twin pointer, wants, the pod itself): the pod with its port
        resources requested on container 0.  A pod without host ports, and a
        twin, is its own twin."""
        addr = C.addressof(pod_ptr[0])
        if addr in self._twin_wants:
            return (pod_ptr,) + self._twin_wants[addr]
        wants = pod_wants(pod_ptr)
        if not wants:
            return pod_ptr, wants, pod_ptr
        p = pod_ptr[0]
        assert p.n_containers >= 1
        q = _abi.KsPod.from_buffer_copy(p)
        cs = (_abi.KsContainer * p.n_containers)(*[p.containers[i] for i in range(p.n_containers)])
        names = [nm.encode() for nm in self.resources(wants)]
        ext = (_abi.KsResource * (cs[0].n_extended + len(names)))(
            *([cs[0].extended[j] for j in range(cs[0].n_extended)] + [_abi.KsResource(b, 1) for b in names]))
        cs[0].extended = C.cast(ext, C.POINTER(_abi.KsResource))
        cs[0].n_extended = len(ext)
        q.containers = C.cast(cs, C.POINTER(_abi.KsContainer))
        self._keep.append((q, cs, ext, names))
        self._twin_wants[C.addressof(q)] = (wants, pod_ptr)
        return C.pointer(q), wants, pod_ptr

    def _twins(self, arr, n):
        tw = (_abi.KsPod * max(1, n))()
        wants = []
        for i in range(n):
            t, w, _ = self._twin(pod_at(arr, i))
            tw[i] = t[0]
            wants.append(w)
        self._keep.append(tw)
        return tw, wants

    # ---- cache events: the emulation's, and the mirror
    def upsert(self, arr, slots, n):
        tw = (_abi.KsNode * max(1, n))()
        for i in range(n):
            tw[i] = arr[i]
            ext = (_abi.KsResource * (arr[i].n_extended + len(self._node_ext)))(
                *([arr[i].extended[j] for j in range(arr[i].n_extended)] +
                  [_abi.KsResource(b, v) for b, v in self._node_ext]))
            tw[i].extended = C.cast(ext, C.POINTER(_abi.KsResource))
            tw[i].n_extended = len(ext)
            self._keep.append(ext)
        super().upsert(tw, slots, n)

    def delete(self, slots, n):
        super().delete(slots, n)
        for i in range(n):
            self.mirror.pop(int(slots[i]), None)

    def add_pods(self, arr, slots, n):
        tw, wants = self._twins(arr, n)
        super().add_pods(tw, slots, n)
        for i in range(n):
            info = self.mirror.setdefault(int(slots[i]), HostPortInfo())
            for w in set(wants[i]):
                assert not info.holds(*w), ("outside the emulation: two bound pods of one node hold", w)
                info.add(*w)

    def remove_pods(self, arr, slots, n):
        tw, wants = self._twins(arr, n)
        super().remove_pods(tw, slots, n)
        for i in range(n):
            info = self.mirror.get(int(slots[i]))
            for w in wants[i]:
                if info is not None:
                    info.remove(*w)

    def used_ports(self, slot):
        """The mirror's entries of a slot, sorted (what ks_node_used_ports returns, sorted)."""
        info = self.mirror.get(slot)
        return info.entries() if info else []

    def conflicts(self, wants):
        """Per slot: some wanted port conflicts with the slot's mirror."""
        out = np.zeros(self.capacity, dtype=bool)
        for slot, info in self.mirror.items():
            out[slot] = any(info.check_conflict(*w) for w in wants)
        return out

    # ---- the plugin
    def plugin_scores(self, pod_ptr):
        tw, wants, real = self._twin(pod_ptr)
        sc = super().plugin_scores(tw)
        self._port_fails = 0
        if not wants:
            return sc
        conflict = self.conflicts(wants)
        # the emulation and the mirror agree wherever the plain pod gets past NodeAffinity and its own Fit
        plain = super().plugin_scores(real)["status"]
        through = (plain == -1) | (plain == 5) | (plain == 6)
        assert np.array_equal((sc["status"] == ST_FIT)[through], conflict[through]), "emulation and mirror disagree"
        ports = (sc["status"] == ST_FIT) & conflict
        sc["status"] = np.where(ports, ST_PORTS, sc["status"])
        self._port_fails = int(ports.sum())
        return sc

    def schedule_one(self, pod_ptr):
        tw, wants, _ = self._twin(pod_ptr)
        stripped = None
        if wants and self.track:
            sc = BaReference.plugin_scores(self, pod_ptr)
            feas = np.nonzero(sc["status"] == -1)[0]
            stripped = int(feas[np.argmax(sc["total_score"][feas])]) if len(feas) else -1
        r = super().schedule_one(tw)  # (its plugin_scores is the one above; it commits the twin)
        r.fail_node_ports = self._port_fails
        if r.status == 0 and wants:
            info = self.mirror.setdefault(int(r.node_index), HostPortInfo())
            for w in wants:
                info.add(*w)
        if stripped is not None:
            self.placed.append((stripped, int(r.node_index)))
        return r
