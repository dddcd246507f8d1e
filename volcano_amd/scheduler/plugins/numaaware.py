"""Numaaware plugin (reference ``plugins/numaaware``: topology-manager
policies none/best-effort/restricted/single-numa-node against the
Numatopology CRD; cpuset assignment providers).

Pods opt in with the annotation ``volcano.sh/numa-topology-policy``
("single-numa-node"/"restricted"/"best-effort").  single-numa-node /
restricted: the pod's CPU request must fit inside one NUMA zone's free
capacity — nodes that can't are a dynamic forbid bit per request shape;
on commit the chosen zone is pinned via the ``volcano.sh/numa-node``
annotation and the zone's usage tracked across cycles.

Plugin argument ``exact`` (default ``false``): the forbid bit is frozen at
session open and sees nothing the cycle places, and the kernels' capacity
comes from the aggregate CPU dim alone — a cycle can bind more pods to a
node than its zones hold, the surplus without a ``volcano.sh/numa-node``,
which the kubelet's topology manager then rejects.  With ``exact: true`` the
plugin publishes ``ssn.numa_exact``: the free millicores per zone of the
inventory as an int32 plane ``[Z, N]`` built from the ``NumaState`` ledger.
The allocate action attaches the request to every class that carries a
policy and drops its ``numa-unfit:`` bit; the cycle then pins per zone, per
placement (``numa_cap`` for the hard policies, ``numa_commit`` for all
three), and ``on_allocate`` pins the zones the cycle chose — ``take``,
cpuset and both annotations — instead of asking ``best_zone`` again.  The
``NumaState`` objects and their cpuset providers stay the ledger across
cycles.

``exact`` stays on the host path (logged once) for an inventory with a node
above 8 zones or a zone whose free value is not a whole number of
millicores in [0, 2^28), and for a class whose CPU request is not a whole
number of millicores in [1, 2^28).  ``SubGroupPolicy`` jobs, preempt/reclaim,
backfill, the nominated fast path and the soft-shard coordinator keep the
session-open bit (under ``exact`` built from the plane in one array pass)
and the host choice."""

from __future__ import annotations

import logging
from typing import Dict, List, Optional, Tuple

import numpy as np

from ...api.resource import CPU
from ...ops.reference import (NUMA_BEST_EFFORT, NUMA_FREE_LIMIT, NUMA_HARD,
                              NUMA_MAX_ZONES, numa_slots)
from ..tensors import set_plane_bit
from .base import Plugin, register

ANN_POLICY = "volcano.sh/numa-topology-policy"
ANN_PINNED = "volcano.sh/numa-node"
ANN_CPUSET = "volcano.sh/cpuset"

POLICIES = {"single-numa-node": NUMA_HARD, "restricted": NUMA_HARD,
            "best-effort": NUMA_BEST_EFFORT}

log = logging.getLogger(__name__)
_warned_host_path = set()


def _truthy(v) -> bool:
    return v is True or str(v).strip().lower() in ("true", "1", "yes")


def _warn_once(key: str, msg: str, *args) -> None:
    if key not in _warned_host_path:
        _warned_host_path.add(key)
        log.warning(msg, *args)


def _whole(x: float) -> Optional[int]:
    """x as an integer when it is within 1e-6 of one."""
    r = int(round(x))
    return r if abs(x - r) <= 1e-6 else None


class CpusetProvider:
    """cpuset assignment provider (reference ``numaaware/provider``):
    hands out SPECIFIC CPU ids from a pinned zone's pool — the contract
    the node-side cpumanager enforces via cgroup cpuset.cpus.  Whole
    cores only (ceil of millicores/1000); released ids return to the
    pool (cache._release_devices analog is the pod-delete path)."""

    def __init__(self, topo):
        self.pools: Dict[int, List[int]] = {}
        for z in topo.zones:
            cpus = list(z.cpus) if z.cpus else list(range(
                z.id * 1000, z.id * 1000 + int(z.cpu_milli // 1000)))
            self.pools[z.id] = cpus

    def assign(self, zone: int, cpu_milli: float) -> List[int]:
        need = max(1, int(-(-cpu_milli // 1000)))     # ceil cores
        pool = self.pools.get(zone, [])
        if len(pool) < need:
            return []
        out, self.pools[zone] = pool[:need], pool[need:]
        return out

    def release(self, zone: int, cpus: List[int]) -> None:
        self.pools.setdefault(zone, []).extend(cpus)


class NumaState:
    """Per-node free millicores per NUMA zone (persists on the cache)."""

    def __init__(self, topo):
        self.free: List[float] = [z.cpu_milli for z in topo.zones]
        self.cpuset = CpusetProvider(topo)

    def best_zone(self, cpu_milli: float):
        best = None
        for i, f in enumerate(self.free):
            if f + 0.1 >= cpu_milli and (best is None
                                         or f < self.free[best]):
                best = i
        return best

    def take(self, zone: int, cpu_milli: float) -> None:
        self.free[zone] -= cpu_milli

    def give(self, zone: int, cpu_milli: float) -> None:
        self.free[zone] += cpu_milli


class NumaExact:
    """What ``exact: true`` publishes on the session (``ssn.numa_exact``)."""

    def __init__(self, plane, unfit_bits) -> None:
        self.plane = plane              # zone_free [Z, N] i32
        self.unfit_bits = unfit_bits    # cpu request -> forbid bit
        # id(tclass) -> one zone (or None) per placed task (set by allocate
        # after the cycle, consumed by on_allocate)
        self.zones: Dict[int, List[Optional[int]]] = {}

    def unfit_nodes(self, cpu: int) -> List[int]:
        """Node ids none of whose zones holds one pod of the shape now."""
        import torch
        slots = numa_slots(torch.from_numpy(self.plane), cpu)
        return np.nonzero(slots.sum(0) < 1)[0].tolist()

    def request_of(self, task) -> Optional[Tuple[int, int]]:
        """(cpu millicores, policy) of a task with a topology policy, when
        the plane can express the request."""
        if task.pod is None:
            return None
        policy = POLICIES.get(task.pod.meta.annotations.get(ANN_POLICY, ""))
        if policy is None:
            return None
        cpu = _whole(task.request.get(CPU))
        if cpu is None or not 1 <= cpu < NUMA_FREE_LIMIT:
            _warn_once("class", "numaaware: a class asks for %s millicores, "
                       "not a whole number in [1, 2^28); it keeps the host "
                       "path", task.request.get(CPU))
            return None
        return cpu, policy


def zone_plane(states, nodes, n: int):
    """The ledger as an int32 plane [Z, N] (0 for a missing zone and for a
    node without a Numatopology), or None when the inventory does not fit it
    (Z > 8, a free value that is no whole number in [0, 2^28))."""
    Z = max((len(st.free) for st in states.values()), default=0)
    if Z == 0 or Z > NUMA_MAX_ZONES:
        return None
    plane = np.zeros((Z, n), dtype=np.int32)
    for name, st in states.items():
        ni = nodes.get(name)
        if ni is None or not 0 <= ni.node_id < n:
            continue
        free = [_whole(f) for f in st.free]
        if any(f is None or not 0 <= f < NUMA_FREE_LIMIT for f in free):
            return None
        plane[:len(free), ni.node_id] = free
    return plane


@register("numaaware")
class NumaAwarePlugin(Plugin):
    def on_session_open(self, ssn) -> None:
        from ...utils.features import enabled
        if not enabled("ResourceTopology"):
            return
        store = getattr(ssn.cache, "store", None)
        topos = store.list("Numatopology") if store is not None else []
        if not topos:
            return
        nt = ssn.node_tensors
        states: Dict[str, NumaState] = getattr(ssn.cache, "_numa_states", {})
        for topo in topos:
            if topo.meta.name not in states:
                states[topo.meta.name] = NumaState(topo)
        ssn.cache._numa_states = states

        unfit_bits: Dict[float, int] = {}

        published = None
        if _truthy(self.args.get("exact", False)):
            plane = zone_plane(states, ssn.nodes, nt.n)
            if plane is not None:
                published = NumaExact(plane, unfit_bits)
                ssn.numa_exact = published
            else:
                _warn_once("session", "numaaware: exact is off — the "
                           "inventory has a node above %d NUMA zones or a "
                           "zone whose free CPU is no whole number of "
                           "millicores in [0, 2^28); zones are chosen on the "
                           "host path", NUMA_MAX_ZONES)

        def policy_of(tclass) -> str:
            pod = tclass.tasks[0].pod
            return pod.meta.annotations.get(ANN_POLICY, "") if pod else ""

        def hook(tclass, job, require, forbid):
            policy = policy_of(tclass)
            if policy not in ("single-numa-node", "restricted"):
                return
            cpu = tclass.request.get(CPU)
            bit = unfit_bits.get(cpu)
            if bit is None:
                # The words are memoized and shared with the consumers that
                # keep the host path under exact (preempt/reclaim, backfill,
                # nomination, subgroups), so the bit is built either way —
                # under exact from the plane in one array pass (a node fits
                # one pod iff some zone has a slot)
                rq = published.request_of(tclass.tasks[0]) \
                    if published is not None else None
                if rq is not None:
                    unfit = published.unfit_nodes(rq[0])
                else:
                    unfit = []
                    for name, ni in ssn.nodes.items():
                        st = states.get(name)
                        if st is None or st.best_zone(cpu) is None:
                            unfit.append(ni.node_id)
                bit = nt.add_dynamic_bit(f"numa-unfit:{cpu}", unfit)
                unfit_bits[cpu] = bit
            set_plane_bit(forbid, bit)

        node_by_id = {ni.node_id: ni for ni in ssn.nodes.values()}

        def on_allocate(tclass, node_ids, counts, tasks=None):
            if policy_of(tclass) not in ("single-numa-node", "restricted",
                                         "best-effort"):
                return
            cpu = tclass.request.get(CPU)
            # exact: one zone (or None) per placed task, in log order —
            # popped, because the walk fires once per NUMA class
            # (allocate.py states the two invariants); a class the cycle
            # did not pack (nomination, subgroups) finds nothing and chooses
            # here
            chosen = published.zones.pop(id(tclass), None) \
                if published is not None else None
            chosen = iter(chosen) if chosen is not None else None
            it = iter(tasks if tasks is not None else tclass.tasks)
            for nid, cnt in zip(node_ids, counts):
                ni = node_by_id.get(nid)
                st = states.get(ni.name) if ni else None
                for _ in range(cnt):
                    task = next(it, None)
                    if task is None:
                        return
                    picked = next(chosen, None) if chosen is not None else None
                    if st is None:
                        continue
                    zone = picked if chosen is not None \
                        else st.best_zone(cpu)
                    if zone is not None:
                        st.take(zone, cpu)
                        if task.pod is not None:
                            ann = task.pod.meta.annotations
                            ann[ANN_PINNED] = str(zone)
                            ids = st.cpuset.assign(zone, cpu)
                            if ids:
                                ann[ANN_CPUSET] = ",".join(
                                    str(c) for c in ids)

        handler = type("NumaHandler", (), {"on_allocate":
                                           staticmethod(on_allocate)})()
        ssn.class_constraint_hooks.append(hook)
        ssn.event_handlers.append(handler)
