"""Topology-spread plugin (reference: predicates wraps the k8s
podtopologyspread filter).

Simplified hard semantics: pods declaring
``affinity = {"topologySpread": {"group": G, "topologyKey": K,
"maxSkew": s}}`` must spread across the values of node label K so that
no value's member count exceeds the minimum count by more than
``maxSkew``.  ``topologySpread`` may also be a list of such dicts — zone
``maxSkew: 1`` together with ``kubernetes.io/hostname`` ``maxSkew: 1`` is
the textbook pair: every entry must hold, a member counts in every
``(group, topologyKey)`` it names, and a node that lacks the label of any
entry is out of bounds.

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

A class with a list of 2 to 4 entries resolves to all its rules,
``[(group, maxSkew), ...]``, and is placed by the multi-rule select
(``spread_multi_select_commit`` / ``spread_multi_select_kernel``), which
holds every ``maxSkew`` before every placement.  A list longer than 4, or
one whose rules have more than ``SPREAD_MULTI_LDS_DOMAINS`` domains in all,
keeps the cycle-granular bits for that class (logged once).

``exact`` is ignored — the cycle-granular path above is used — for jobs
with a SubGroupPolicy and for runs under the soft-shard coordinator:
both can drop placements after the kernel has counted them.

An entry with ``whenUnsatisfiable: "ScheduleAnyway"`` is SOFT (anything
else, absence included, is ``DoNotSchedule``).  It never filters on counts:
it sets no saturation bit and does not enter the session-open floor; only
its unlabeled nodes stay out of bounds.  With ``exact: true`` it is scored
per placement on the device (``spread_soft_select_commit`` /
``spread_soft_select_kernel``): every member already in a node's domain
costs the node ``soft.weight / 100`` of score (plugin argument
``soft.weight``, default 2.0 — the reference's podtopologyspread weight on
its 0-100 scale against the 0-1 score terms here).  ``resolve_task`` names a
soft rule with ``SPREAD_SOFT_SKEW`` as a maxSkew that never binds, and
``soft_weights`` gives the per-rule weights beside it (0 = hard).  Without
``exact``, where ``exact`` is ignored, or when the soft rules of a class have
more than ``SPREAD_SOFT_LDS_DOMAINS`` domains in all, a soft entry adds no
score (logged once).
"""

from __future__ import annotations

from collections import defaultdict
import logging
from typing import Dict, List, Optional, Tuple

import numpy as np

from ...api.types import TaskStatus
from ...ops.reference import (SPREAD_MAX_RULES, SPREAD_MULTI_LDS_DOMAINS,
                              SPREAD_SOFT_LDS_DOMAINS, SPREAD_SOFT_SKEW)
from ..tensors import set_plane_bit
from .base import Plugin, register

OCCUPY = (TaskStatus.ALLOCATED, TaskStatus.BINDING, TaskStatus.BOUND,
          TaskStatus.RUNNING)


log = logging.getLogger(__name__)
# classes already reported as cycle-granular.  Per process on purpose: the
# plugin and what it publishes are rebuilt at every session open, so state
# kept on either would repeat the line every cycle.
_LOGGED: set = set()


def _specs(pod) -> list:
    """The pod's spread constraints: ``topologySpread`` is one dict or a
    list of them; one entry per (group, topologyKey), the first wins."""
    aff = pod.affinity if pod is not None else None
    s = aff.get("topologySpread") if isinstance(aff, dict) else None
    out, seen = [], set()
    for e in (s if isinstance(s, (list, tuple)) else (s,)):
        if isinstance(e, dict) and e.get("group") and e.get("topologyKey") \
                and (e["group"], e["topologyKey"]) not in seen:
            seen.add((e["group"], e["topologyKey"]))
            out.append(e)
    return out


def _soft(e) -> bool:
    """``whenUnsatisfiable: ScheduleAnyway`` — everything else is hard."""
    return e.get("whenUnsatisfiable") == "ScheduleAnyway"


def _log_once(specs, why: str,
              then: str = "the class keeps the cycle-granular path") -> None:
    key = tuple((e["group"], e["topologyKey"]) for e in specs)
    if (key, then) not in _LOGGED:
        _LOGGED.add((key, then))
        log.warning("topologyspread: %s for %s; %s", why, list(key), then)


_UNSCORED = "its ScheduleAnyway entries add no score"


def _truthy(v) -> bool:
    if isinstance(v, str):
        return v.strip().lower() in ("1", "true", "yes", "on")
    return bool(v)


class SpreadExact:
    """What ``exact: true`` publishes on the session (``ssn.spread_exact``)."""

    def __init__(self, soft_tw: float = 0.02):
        self.soft_tw = soft_tw               # score per member, soft rules
        self._soft_memo: Dict[object, Optional[list]] = {}
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

    def resolve_task(self, task):
        """(group index, maxSkew >= 1) of a task's class; with several
        constraints the list of all of them; None when there is none or
        the class stays cycle-granular.  A soft entry is a rule with
        ``SPREAD_SOFT_SKEW``; ``soft_weights`` tells which."""
        sig = task.class_signature()
        got = self._memo.get(sig, self)
        if got is not self:
            return got
        out = None
        specs = _specs(task.pod)
        gs = [self._index.get((s["group"], s["topologyKey"])) for s in specs]
        soft = [g for g, s in zip(gs, specs) if _soft(s) and g is not None]
        if sum(len(self.count[g]) for g in soft) > SPREAD_SOFT_LDS_DOMAINS:
            # the soft entries leave; the hard ones stay exact
            _log_once(specs, f"more than {SPREAD_SOFT_LDS_DOMAINS} domains "
                             "over the soft constraints", _UNSCORED)
            keep = [i for i, s in enumerate(specs) if not _soft(s)]
            specs, gs = [specs[i] for i in keep], [gs[i] for i in keep]
        tws = None
        if specs and None not in gs:
            rules = [(g, SPREAD_SOFT_SKEW if _soft(s)
                      else max(1, int(s.get("maxSkew", 1))))
                     for g, s in zip(gs, specs)]
            if any(_soft(s) for s in specs):
                tws = [self.soft_tw if _soft(s) else 0.0 for s in specs]
            if len(rules) == 1:
                out = rules[0]
            elif len(rules) > SPREAD_MAX_RULES:
                _log_once(specs, f"more than {SPREAD_MAX_RULES} constraints")
            elif sum(len(self.count[g]) for g in gs) \
                    > SPREAD_MULTI_LDS_DOMAINS:
                _log_once(specs, f"more than {SPREAD_MULTI_LDS_DOMAINS} "
                                 "domains in all")
            else:
                out = rules
        self._memo[sig] = out
        self._soft_memo[sig] = tws if out is not None else None
        return out

    def soft_weights(self, task) -> Optional[list]:
        """One f32 weight per rule of ``resolve_task(task)``, 0 for a hard
        rule; None when the class has no soft rule."""
        self.resolve_task(task)
        return self._soft_memo.get(task.class_signature())

    def resolve(self, tclass, job=None):
        return self.resolve_task(tclass.tasks[0])


@register("topologyspread")
class TopologySpreadPlugin(Plugin):
    def on_session_open(self, ssn) -> None:
        nt = ssn.node_tensors
        exact = _truthy(self.args.get("exact", False))
        soft_tw = float(np.float32(
            float(self.args.get("soft.weight", 2.0)) / 100.0))

        # group → topology value → placed member count
        counts: Dict[tuple, Dict[str, int]] = defaultdict(
            lambda: defaultdict(int))
        specs: Dict[tuple, dict] = {}
        for job in ssn.jobs.values():
            for t in job.tasks.values():
                for s in _specs(t.pod):
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
        published = SpreadExact(soft_tw) if exact else None
        for gk, s in specs.items():
            group, key = gk
            max_skew = int(s.get("maxSkew", 1))
            vals = nodes_by_val.get(key, {})
            if not vals:
                continue
            cnt = counts.get(gk, {})
            floor = min((cnt.get(v, 0) for v in vals), default=0)
            # a soft constraint never filters on counts
            saturated = [] if _soft(s) else [
                v for v in vals if cnt.get(v, 0) >= floor + max_skew]
            # nodes without the topology label are always out of bounds
            unlabeled = [ni.node_id for ni in ssn.nodes.values()
                         if ni.node.meta.labels.get(key) is None]
            if not exact:
                if _soft(s):
                    _log_once([s], "exact is off", _UNSCORED)
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
            for s in _specs(tclass.tasks[0].pod):
                gk = (s["group"], s["topologyKey"])
                # exact: a soft entry takes the unlabeled bit alone
                sat = None if exact and _soft(s) else bits.get(gk)
                for bit in (sat, unl_bits.get(gk)):
                    if bit is not None:
                        set_plane_bit(forbid, bit)

        ssn.class_constraint_hooks.append(hook)
        if published is not None and published.keys:
            ssn.spread_exact = published
