"""Inter-pod affinity plugin (reference: predicates wraps the k8s
interpodaffinity filter, plugins/predicates/predicates.go:34-47).

Simplified hard semantics, expressed through the existing kernel
machinery — no per-(pod,pod) matching in the hot loop.  Pod spec::

    affinity = {"podAffinity":     {"group": G, "topologyKey": K}}
    affinity = {"podAntiAffinity": {"group": G, "topologyKey": K}}

``topologyKey`` is optional; without it, or with
``kubernetes.io/hostname``, the rule is per node.  Members of G are the
tasks that declare the same kind and group.  A domain is one value of node
label K; a node without the label belongs to no domain and never takes a
member of a keyed rule (the topologyspread convention — for anti-affinity
stricter than k8s, which lets such nodes pass).

Cycle-granular path (default; backfill, preempt, reclaim and the
nominated fast path always use it) — bits computed at session open:

* **anti-affinity at hostname**: handled structurally, not by this
  plugin — group G is a synthetic unit resource dim (``paa:G``): every
  node offers 1 (tensors.py pack), every member requests 1
  (TaskInfo.from_pod), so the score/cap kernel's ordinary capacity math
  enforces at-most-one-member-per-node, exactly, per placement.  Keyed
  anti-affinity pods keep the dim too (the domain rule implies it).
* **anti-affinity over a key**: a forbid bit over every node of a domain
  that already holds a member, plus the unlabelled nodes.
* **affinity**: a require bit over the nodes already hosting a member of
  G (no key) or over all nodes of the hosting domains (key); a keyed rule
  also forbids the unlabelled nodes.  While the group has no placed
  member the rule is vacuous — the first member anchors — so k replicas
  submitted in ONE cycle all see an empty group and scatter by score.

Plugin argument ``exact`` (default ``false``): with ``exact: true`` the
allocate action enforces the rule before EVERY single placement, on the
device (``ops/reference.py affinity_select_commit`` / ``domain_mask_kernel``
+ ``select_commit`` + ``domain_count_add_kernel``): the first instance of
an empty group anchors its domain and every later instance — of the same
class, of later classes and jobs of the group in the cycle — follows; a
keyed anti-affinity placement closes its domain at once.  The plugin then
publishes ``ssn.affinity_exact``: per (kind, group, key) the domain map
(the key's values in sorted order → dense ids, unlabelled nodes → -1; for
a hostname rule the identity map with D = N), the placed counts per
domain, the session-open bit (the plan builder takes it off the classes it
routes exactly) and a memoised resolver from a task class to
``(group index, mode)`` with mode 1 = affinity, 2 = anti-affinity.  A
class carries one domain rule: exact topology spread wins, then affinity,
then keyed anti-affinity; any further rule of the class stays on its
cycle-granular bit.  A gang that reverts gives its counts back.

``exact`` is ignored — the cycle-granular path above is used — for jobs
with a SubGroupPolicy and for runs under the soft-shard coordinator: both
can drop placements after the kernel has counted them.
"""

from __future__ import annotations

import json
from typing import Dict, List, Optional, Set, Tuple

import numpy as np

from ...api.types import TaskStatus
from ..tensors import set_plane_bit
from .base import Plugin, register

OCCUPY = (TaskStatus.ALLOCATED, TaskStatus.BINDING, TaskStatus.BOUND,
          TaskStatus.RUNNING)

HOSTNAME_KEY = "kubernetes.io/hostname"
AFFINITY, ANTI = 1, 2
_KIND = {"podAffinity": AFFINITY, "podAntiAffinity": ANTI}


def _rule(pod, kind: str) -> Optional[tuple]:
    """(kind, group, key) of a pod's rule; key None = per node."""
    aff = pod.affinity if pod is not None else None
    spec = aff.get(kind) if isinstance(aff, dict) else None
    if not isinstance(spec, dict) or not spec.get("group"):
        return None
    key = spec.get("topologyKey")
    if not key or key == HOSTNAME_KEY:
        key = None
    return (kind, spec["group"], key)


def _keyed_name(prefix: str, *parts) -> str:
    """Dynamic-bit name of a keyed rule.  The prefixes differ from the
    per-node ``paff:`` and the JSON quoting keeps (group, key) pairs apart
    whatever characters the names hold."""
    return f"{prefix}:{json.dumps(list(parts))}"


def _truthy(v) -> bool:
    if isinstance(v, str):
        return v.strip().lower() in ("1", "true", "yes", "on")
    return bool(v)


class AffinityExact:
    """What ``exact: true`` publishes on the session
    (``ssn.affinity_exact``)."""

    def __init__(self):
        self.keys: List[tuple] = []          # (kind, group, key) per index
        self.dom_of: List[np.ndarray] = []   # [N] i32 per rule
        self.count: List[np.ndarray] = []    # [D] i32 per rule
        self.mode: List[int] = []            # 1 = affinity, 2 = anti
        # session-open bit of the rule (require plane for affinity, forbid
        # plane for anti-affinity), or None
        self.open_bit: List[Optional[int]] = []
        self._index: Dict[tuple, int] = {}
        self._memo: Dict[object, Optional[tuple]] = {}

    def add(self, rule, dom_of, count, mode, open_bit) -> None:
        self._index[rule] = len(self.keys)
        self.keys.append(rule)
        self.dom_of.append(dom_of)
        self.count.append(count)
        self.mode.append(mode)
        self.open_bit.append(open_bit)

    def resolve_task(self, task) -> Optional[Tuple[int, int]]:
        """(group index, mode) of a task's class, or None.  Affinity
        before keyed anti-affinity: a class carries one domain rule."""
        sig = task.class_signature()
        got = self._memo.get(sig, self)
        if got is not self:
            return got
        out = None
        for kind in ("podAffinity", "podAntiAffinity"):
            rule = _rule(task.pod, kind)
            g = self._index.get(rule) if rule is not None else None
            if g is not None:
                out = (g, self.mode[g])
                break
        self._memo[sig] = out
        return out


@register("interpodaffinity")
class InterPodAffinityPlugin(Plugin):
    def on_session_open(self, ssn) -> None:
        nt = ssn.node_tensors
        exact = _truthy(self.args.get("exact", False))

        # (kind, group) → node ids hosting a placed member; every declared
        # rule, placed or pending
        hosts: Dict[tuple, List[int]] = {}
        rules: Set[tuple] = set()
        for job in ssn.jobs.values():
            for t in job.tasks.values():
                pod = t.pod
                if pod is None or not pod.affinity:
                    continue        # the common case: no affinity at all
                for kind in _KIND:
                    rule = _rule(pod, kind)
                    if rule is None:
                        continue
                    rules.add(rule)
                    if t.status in OCCUPY and t.node_name in ssn.nodes:
                        hosts.setdefault(rule[:2], []).append(
                            ssn.nodes[t.node_name].node_id)
        if not rules:
            return

        keys = {r[2] for r in rules if r[2] is not None}
        nodes_by_val: Dict[str, Dict[str, list]] = {k: {} for k in keys}
        unlabelled: Dict[str, list] = {k: [] for k in keys}
        for ni in ssn.nodes.values():
            for k in keys:
                val = ni.node.meta.labels.get(k)
                if val is None:
                    unlabelled[k].append(ni.node_id)
                else:
                    nodes_by_val[k].setdefault(val, []).append(ni.node_id)

        require_bits: Dict[tuple, List[int]] = {}
        forbid_bits: Dict[tuple, List[int]] = {}
        published = AffinityExact() if exact else None

        for rule in sorted(rules, key=lambda r: (r[0], r[1], r[2] or "")):
            kind, group, key = rule
            mode = _KIND[kind]
            placed = hosts.get((kind, group), [])
            if key is None:
                # per node.  Anti-affinity is the structural paa: dim.
                if mode == ANTI:
                    continue
                open_bit = None
                if placed:
                    open_bit = nt.add_dynamic_bit(
                        f"paff:{group}", sorted(set(placed)))
                    require_bits.setdefault(rule, []).append(open_bit)
                if published is not None:
                    count = np.bincount(
                        np.asarray(placed, dtype=np.int64),
                        minlength=nt.n).astype(np.int32)
                    if nt.n:
                        published.add(rule, np.arange(nt.n, dtype=np.int32),
                                      count, mode, open_bit)
                continue

            vals = nodes_by_val[key]
            order = sorted(vals)
            dense = {v: d for d, v in enumerate(order)}
            dom_of = np.full(nt.n, -1, dtype=np.int32)
            for v, ids in vals.items():
                dom_of[np.asarray(ids, dtype=np.int64)] = dense[v]
            count = np.zeros(max(len(order), 1), dtype=np.int32)
            for nid in placed:
                if dom_of[nid] >= 0:
                    count[dom_of[nid]] += 1
            occupied_ids = [nid for v in order if count[dense[v]] > 0
                            for nid in vals[v]]
            open_bit = None
            if mode == AFFINITY:
                if unlabelled[key]:
                    forbid_bits.setdefault(rule, []).append(
                        nt.add_dynamic_bit(_keyed_name("paff-unl", key),
                                           sorted(unlabelled[key])))
                if occupied_ids:
                    open_bit = nt.add_dynamic_bit(
                        _keyed_name("paff-key", group, key),
                        sorted(occupied_ids))
                    require_bits.setdefault(rule, []).append(open_bit)
            else:
                ids = occupied_ids + unlabelled[key]
                if ids:
                    open_bit = nt.add_dynamic_bit(
                        _keyed_name("panti-key", group, key),
                        sorted(set(ids)))
                    forbid_bits.setdefault(rule, []).append(open_bit)
            if published is not None and nt.n:
                published.add(rule, dom_of, count, mode, open_bit)

        if require_bits or forbid_bits:
            def hook(tclass, job, require, forbid):
                pod = tclass.tasks[0].pod
                for kind in _KIND:
                    rule = _rule(pod, kind)
                    if rule is None:
                        continue
                    for bit in require_bits.get(rule, ()):
                        set_plane_bit(require, bit)
                    for bit in forbid_bits.get(rule, ()):
                        set_plane_bit(forbid, bit)

            ssn.class_constraint_hooks.append(hook)
        if published is not None and published.keys:
            ssn.affinity_exact = published
