"""Network-topology-aware plugin (reference
``plugins/network-topology-aware`` + the allocate action's hypernode
gradient search; design "Network Topology Aware
Scheduling").

A job whose PodGroup sets ``networkTopology`` ({"mode": "hard"|"soft",
"highestTierAllowed": t}) is confined to ONE network domain (hypernode)
of tier ≤ t.  MI355X mapping: every hypernode's member set is a dynamic
bit plane; the per-job domain choice (the "gradient" — prefer the
lowest-tier feasible domain, then the one already hosting the job's
tasks) is a cheap host-side scan over per-domain free-capacity vectors,
and the chosen domain rides the predicate kernel as one require bit.

Hard mode: no feasible domain ⇒ the job's classes get an impossible
require bit (never placed this cycle).  Soft mode: feasible domain
preferred, otherwise unconstrained.

Plugin argument ``exact`` (default ``false``): with ``exact: true`` the
domain is chosen ON THE DEVICE, per class, from the live per-node
capacity the score kernel just computed (``ops/reference.py
hypernode_mask`` / mode 3 of ``vamd_domain_mask``).  The choice then sees
everything placed earlier in the same cycle, fragmentation (a rack whose
free memory no single pod fits has capacity 0) and every predicate, and
within the lowest feasible tier it takes the tightest fit.  The plugin
publishes ``ssn.hypernode_exact``: the depth-first leaf numbering that
makes every hypernode one contiguous leaf range, ``leaf_of[N]``, the
``(lo, hi)`` lists per tier and ``resolve_job``.  A direct ``Node`` member
of a non-leaf hypernode gets a pseudo-leaf inside its parent's range.

The allocate action routes this way the jobs that plan as ONE single-class
gang and every SubGroupPolicy subgroup with a ``networkTopology`` override
(each subgroup its own rule, no pin, no reservation ledger).  The host
choice above stays in force for multi-class jobs (the first class's choice
would have to reach the later classes on the device), for jobs with a
placed task on a node outside every hypernode, for HyperNode sets that are
not laminar (a node in two hypernodes neither of which contains the other;
logged once), under the soft-shard coordinator, and for backfill, preempt
and the nominated fast path.
"""

from __future__ import annotations

import logging
from typing import Dict, List, Optional, Tuple

import numpy as np

from ...api.hypernode import HyperNodeTree
from ..tensors import set_plane_bit
from .base import Plugin, register


log = logging.getLogger(__name__)


def _truthy(v) -> bool:
    if isinstance(v, str):
        return v.strip().lower() in ("1", "true", "yes", "on")
    return bool(v)


class HypernodeExact:
    """What ``exact: true`` publishes on the session
    (``ssn.hypernode_exact``)."""

    def __init__(self, leaf_of: np.ndarray, n_leaves: int,
                 tiers: List[int], ranges: List[List[Tuple[int, int]]],
                 leaf_by_node: Dict[str, int]):
        self.leaf_of = leaf_of          # [N] i32, -1 = in no hypernode
        self.n_leaves = n_leaves        # D
        self.tiers = tiers              # distinct tier values, ascending
        self.ranges = ranges            # per tier: (lo, hi), ascending lo
        self.leaf_by_node = leaf_by_node

    def tiers_upto(self, max_tier) -> List[List[Tuple[int, int]]]:
        return [r for t, r in zip(self.tiers, self.ranges)
                if max_tier is None or t <= max_tier]

    def resolve_spec(self, spec, placed_nodes=()):
        """(tier lists, pin or None, soft) of a networkTopology spec, or
        None when the host path must decide (no tier allowed, or a placed
        task outside every hypernode)."""
        if not spec:
            return None
        tiers = self.tiers_upto(spec.get("highestTierAllowed"))
        if not tiers:
            return None
        pin = None
        if placed_nodes:
            leaves = [self.leaf_by_node.get(n) for n in placed_nodes]
            if any(l is None for l in leaves):
                return None
            pin = (min(leaves), max(leaves) + 1)
        return tiers, pin, spec.get("mode", "hard") != "hard"

    def resolve_job(self, job):
        """``resolve_spec`` of the job's PodGroup, pinned to the leaf range
        its already-placed tasks span."""
        spec = job.podgroup.spec.network_topology \
            if job is not None and job.podgroup is not None else None
        if not spec:
            return None
        return self.resolve_spec(
            spec, {t.node_name for t in job.tasks.values() if t.node_name})


def number_leaves(tree: HyperNodeTree, node_ids: Dict[str, int],
                  n: int) -> Optional[HypernodeExact]:
    """Depth-first leaf numbering of the HyperNode tree: afterwards every
    hypernode of every tier is one contiguous leaf range.  None when the
    set is not laminar or holds no node."""
    children: Dict[str, List[str]] = {}
    for child, parent in tree.parent.items():
        children.setdefault(parent, []).append(child)
    leaf_by_node: Dict[str, int] = {}
    span: Dict[str, Tuple[int, int]] = {}
    nxt = 0

    def walk(h: str) -> bool:
        nonlocal nxt
        lo = nxt
        below = set()
        for c in sorted(children.get(h, ())):
            if c in span or not walk(c):
                return False
            below |= tree.members[c]
        direct = sorted(m for m in tree.members[h] - below if m in node_ids)
        if direct:                      # (pseudo-)leaf of the direct nodes
            for m in direct:
                if m in leaf_by_node:
                    return False
                leaf_by_node[m] = nxt
            nxt += 1
        span[h] = (lo, nxt)
        return True

    roots = sorted(h for h in tree.members if h not in tree.parent)
    if not all(walk(r) for r in roots) or nxt == 0:
        return None
    # every hypernode must own exactly the nodes of its leaf range
    for h, (lo, hi) in span.items():
        mine = {m for m in tree.members[h] if m in node_ids}
        if mine != {m for m, l in leaf_by_node.items() if lo <= l < hi}:
            return None
    if len(span) != len(tree.members):
        return None
    leaf_of = np.full(n, -1, dtype=np.int32)
    for m, l in leaf_by_node.items():
        leaf_of[node_ids[m]] = l
    tiers = sorted(set(tree.tier[h] for h in span))
    ranges = [sorted((span[h] for h in span if tree.tier[h] == t))
              for t in tiers]
    return HypernodeExact(leaf_of, nxt, tiers, ranges, leaf_by_node)


@register("network-topology-aware")
class NetworkTopologyAwarePlugin(Plugin):
    def on_session_open(self, ssn) -> None:
        store = getattr(ssn.cache, "store", None)
        hypernodes = store.list("HyperNode") if store is not None else []
        if not hypernodes:
            return
        nt = ssn.node_tensors
        tree = HyperNodeTree(
            hypernodes, list(ssn.nodes),
            {n: ni.node.meta.labels for n, ni in ssn.nodes.items()})
        ssn.hypernode_tree = tree
        if _truthy(self.args.get("exact", False)):
            published = number_leaves(
                tree, {n: ni.node_id for n, ni in ssn.nodes.items()}, nt.n)
            if published is None:
                log.warning("network-topology-aware: the HyperNode set is "
                            "not laminar; exact domain choice is off for "
                            "this session")
            else:
                ssn.hypernode_exact = published

        # per-domain: node ids, free capacity vector, membership bit
        self.domain_ids: Dict[str, list] = {}
        self.domain_bit: Dict[str, int] = {}
        free = {}
        for hname, nodes in tree.members.items():
            ids = [ssn.nodes[n].node_id for n in nodes if n in ssn.nodes]
            self.domain_ids[hname] = ids
            self.domain_bit[hname] = nt.add_dynamic_bit(f"hn:{hname}", ids)
            vec = np.zeros(nt.r, dtype=np.float64)
            for n in nodes:
                ni = ssn.nodes.get(n)
                if ni is not None:
                    vec += nt.resource_vector(ni.idle)
            free[hname] = vec

        impossible_bit = nt.nowhere_bit()
        choice: Dict[str, Optional[str]] = {}

        def choose_domain(job) -> Optional[str]:
            if job.key in choice:
                return choice[job.key]
            spec = job.podgroup.spec.network_topology if job.podgroup else None
            if not spec:
                choice[job.key] = None
                return None
            max_tier = spec.get("highestTierAllowed")
            need = np.zeros(nt.r, dtype=np.float64)
            for t in job.pending_tasks:
                v = nt.req_vector(t)
                if v is not None:
                    need += v
            # nodes already hosting the job pin candidate domains
            running_nodes = {t.node_name for t in job.tasks.values()
                             if t.node_name}
            best = None
            for hname in tree.domains_by_tier(max_tier):
                members = tree.members[hname]
                if running_nodes and not running_nodes <= members:
                    continue
                if (free[hname] + 0.1 >= need).all():
                    best = hname
                    break
            choice[job.key] = best
            return best

        # per-SUBGROUP domains (SubGroupPolicy networkTopology): classes
        # carrying a topology override pick their own domain against a
        # build-time reservation ledger, so several subgroups of one job
        # spread across racks within ONE cycle (a failed subgroup's
        # reservation is simply re-chosen next cycle)
        free_resv = {h: f.copy() for h, f in free.items()}

        def choose_domain_for_class(tclass):
            spec = tclass.topology
            max_tier = spec.get("highestTierAllowed")
            v = nt.req_vector(tclass.tasks[0])
            if v is None:
                return None
            need = v.astype(np.float64) * len(tclass.tasks)
            for hname in tree.domains_by_tier(max_tier):
                if (free_resv[hname] + 0.1 >= need).all():
                    free_resv[hname] = free_resv[hname] - need
                    return hname
            return None

        def hook(tclass, job, require, forbid):
            spec2 = getattr(tclass, "topology", None)
            if spec2:
                best = choose_domain_for_class(tclass)
                if best is not None:
                    set_plane_bit(require, self.domain_bit[best])
                elif spec2.get("mode", "hard") == "hard":
                    set_plane_bit(require, impossible_bit)
                return
            if job is None or job.podgroup is None:
                return
            spec = job.podgroup.spec.network_topology
            if not spec:
                return
            best = choose_domain(job)
            if best is not None:
                set_plane_bit(require, self.domain_bit[best])
            elif spec.get("mode", "hard") == "hard":
                set_plane_bit(require, impossible_bit)
            # soft + no feasible domain: unconstrained

        hook.is_topology = True       # preempt domain trials strip it
        domain_sets = {h: set(ids) for h, ids in self.domain_ids.items()}

        def on_allocate(tclass, node_ids, counts, tasks=None):
            """Keep per-domain free capacity current within the cycle."""
            if not tclass.tasks:
                return
            req = nt.req_vector(tclass.tasks[0])
            if req is None:
                return
            placed_per_node = dict(zip(node_ids, counts))
            for hname, ids in domain_sets.items():
                hit = sum(c for nid, c in placed_per_node.items()
                          if nid in ids)
                if hit:
                    free[hname] -= hit * req.astype(np.float64)

        handler = type("NtaHandler", (), {"on_allocate":
                                          staticmethod(on_allocate)})()
        ssn.class_constraint_hooks.append(hook)
        ssn.event_handlers.append(handler)
        self.tree = tree
