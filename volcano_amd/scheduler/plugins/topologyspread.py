"""Topology-spread plugin (reference: predicates wraps the k8s
podtopologyspread filter).

Simplified hard semantics: pods declaring
``affinity = {"topologySpread": {"group": G, "topologyKey": K,
"maxSkew": s}}`` must spread across the values of node label K so that
no value's member count exceeds the minimum count by more than
``maxSkew``.

Mapping: at session open the plugin counts placed members of G per
topology value and forbids (dynamic bit) the nodes of every value that
is already at ``min_count + maxSkew``.  Enforcement is cycle-granular:
the counts refresh per cycle, so a class of k instances placed in one
cycle can transiently overshoot inside the cycle — exact for the
pod-per-cycle arrival pattern, convergent otherwise (documented
approximation; the within-class least-requested spread keeps instances
apart in practice).

Plugin argument ``exact`` (default ``false``): with ``exact: true`` the
allocate action enforces ``maxSkew`` before EVERY single placement, on
the device (``ops/reference.py spread_select_commit`` /
``spread_select_kernel``).  The plugin then also publishes
``ssn.spread_exact``: per (group, topologyKey) the domain map (the key's
values in sorted order → dense ids, unlabeled nodes → -1) and the placed
counts per domain, plus a resolver from a task class to
``(group, maxSkew)`` (``maxSkew`` clamped to >= 1).  Counts carry across
all classes of a group inside the cycle, a domain that was saturated at
session open reopens as soon as the minimum rises, and a gang that
reverts gives its counts back.  A class placed this way does not carry
the session-open saturation bit (unlabeled nodes stay forbidden);
backfill, preempt, reclaim and the nominated fast path keep the
cycle-granular bit.

``exact`` is ignored — the cycle-granular path above is used — for jobs
with a SubGroupPolicy and for runs under the soft-shard coordinator:
both can drop placements after the kernel has counted them.
"""

from __future__ import annotations

from collections import defaultdict
from typing import Dict, List, Optional, Tuple

import numpy as np

from ...api.types import TaskStatus
from ..tensors import set_plane_bit
from .base import Plugin, register

OCCUPY = (TaskStatus.ALLOCATED, TaskStatus.BINDING, TaskStatus.BOUND,
          TaskStatus.RUNNING)


def _spec(pod):
    aff = pod.affinity if pod is not None else None
    if isinstance(aff, dict):
        s = aff.get("topologySpread")
        if isinstance(s, dict) and s.get("group") and s.get("topologyKey"):
            return s
    return None


def _truthy(v) -> bool:
    if isinstance(v, str):
        return v.strip().lower() in ("1", "true", "yes", "on")
    return bool(v)


class SpreadExact:
    """What ``exact: true`` publishes on the session (``ssn.spread_exact``)."""

    def __init__(self):
        self.keys: List[tuple] = []          # (group, topologyKey) per index
        self.dom_of: List[np.ndarray] = []   # [N] i32 per group
        self.count: List[np.ndarray] = []    # [D] i32 per group
        self.sat_bit: List[Optional[int]] = []
        self._index: Dict[tuple, int] = {}
        self._memo: Dict[object, Optional[tuple]] = {}

    def add(self, gk, dom_of, count, sat_bit) -> None:
        self._index[gk] = len(self.keys)
        self.keys.append(gk)
        self.dom_of.append(dom_of)
        self.count.append(count)
        self.sat_bit.append(sat_bit)

    def resolve_task(self, task) -> Optional[Tuple[int, int]]:
        """(group index, maxSkew >= 1) of a task's class, or None."""
        sig = task.class_signature()
        got = self._memo.get(sig, self)
        if got is not self:
            return got
        out = None
        s = _spec(task.pod)
        if s is not None:
            g = self._index.get((s["group"], s["topologyKey"]))
            if g is not None:
                out = (g, max(1, int(s.get("maxSkew", 1))))
        self._memo[sig] = out
        return out

    def resolve(self, tclass, job=None) -> Optional[Tuple[int, int]]:
        return self.resolve_task(tclass.tasks[0])


@register("topologyspread")
class TopologySpreadPlugin(Plugin):
    def on_session_open(self, ssn) -> None:
        nt = ssn.node_tensors
        exact = _truthy(self.args.get("exact", False))

        # group → topology value → placed member count
        counts: Dict[tuple, Dict[str, int]] = defaultdict(
            lambda: defaultdict(int))
        specs: Dict[tuple, dict] = {}
        for job in ssn.jobs.values():
            for t in job.tasks.values():
                s = _spec(t.pod)
                if s is None:
                    continue
                gk = (s["group"], s["topologyKey"])
                specs[gk] = s
                if t.status in OCCUPY and t.node_name in ssn.nodes:
                    ni = ssn.nodes[t.node_name]
                    val = ni.node.meta.labels.get(s["topologyKey"])
                    if val is not None:
                        counts[gk][val] += 1
        if not specs:
            return

        # nodes per topology value (per key)
        nodes_by_val: Dict[str, Dict[str, list]] = defaultdict(
            lambda: defaultdict(list))
        for ni in ssn.nodes.values():
            for (_, key) in specs:
                val = ni.node.meta.labels.get(key)
                if val is not None:
                    nodes_by_val[key][val].append(ni.node_id)

        bits: Dict[tuple, int] = {}
        unl_bits: Dict[tuple, int] = {}
        published = SpreadExact() if exact else None
        for gk, s in specs.items():
            group, key = gk
            max_skew = int(s.get("maxSkew", 1))
            vals = nodes_by_val.get(key, {})
            if not vals:
                continue
            cnt = counts.get(gk, {})
            floor = min((cnt.get(v, 0) for v in vals), default=0)
            saturated = [v for v in vals
                         if cnt.get(v, 0) >= floor + max_skew]
            # nodes without the topology label are always out of bounds
            unlabeled = [ni.node_id for ni in ssn.nodes.values()
                         if ni.node.meta.labels.get(key) is None]
            if not exact:
                ids = unlabeled + [nid for v in saturated
                                   for nid in vals[v]]
                if ids:
                    bits[gk] = nt.add_dynamic_bit(
                        f"tsp:{group}:{key}:{floor}", sorted(set(ids)))
                continue
            # exact: the saturation set gets a bit of its own, so the
            # allocate plan builder can leave it off the classes it routes
            # through the per-placement select
            if unlabeled:
                unl_bits[gk] = nt.add_dynamic_bit(
                    f"tsp-unl:{group}:{key}", sorted(set(unlabeled)))
            sat_ids = [nid for v in saturated for nid in vals[v]]
            if sat_ids:
                bits[gk] = nt.add_dynamic_bit(
                    f"tsp:{group}:{key}:{floor}", sorted(set(sat_ids)))
            order = sorted(vals)
            dom_of = np.full(nt.n, -1, dtype=np.int32)
            for d, v in enumerate(order):
                dom_of[np.asarray(vals[v], dtype=np.int64)] = d
            count = np.array([cnt.get(v, 0) for v in order], dtype=np.int32)
            published.add(gk, dom_of, count, bits.get(gk))

        def hook(tclass, job, require, forbid):
            s = _spec(tclass.tasks[0].pod)
            if s is None:
                return
            gk = (s["group"], s["topologyKey"])
            for bit in (bits.get(gk), unl_bits.get(gk)):
                if bit is not None:
                    set_plane_bit(forbid, bit)

        ssn.class_constraint_hooks.append(hook)
        if published is not None and published.keys:
            ssn.spread_exact = published
