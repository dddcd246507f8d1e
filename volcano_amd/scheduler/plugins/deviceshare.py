"""Deviceshare plugin (reference ``plugins/deviceshare``): GPU sharing /
vGPU slicing through per-node device pools (api/devices.py).

The dense kernel handles the aggregate resource fit; this plugin adds
the per-card packing predicate: for each distinct device request shape,
nodes whose pool cannot pack the slices get a dynamic forbid bit; on
commit the pool assigns card indices (written into the task's pod
annotations — the ``volcano.sh/gpu-index`` contract the device plugin
on the node consumes).

Plugin argument ``exact`` (default ``false``): the forbid bit is frozen at
session open and sees nothing the cycle places, and the kernels' capacity
comes from the aggregate dims alone — a cycle can bind more pods to a node
than its cards pack, the surplus without a card.  With ``exact: true`` the
plugin publishes ``ssn.device_exact``: the card planes of the inventory
(``plan.DeviceState``) built from the pools.  The allocate action attaches
the request to every class that carries one and drops its ``dev-unfit:``
bit; the cycle then packs per card, per placement (``device_cap`` /
``device_commit``), and ``on_allocate`` takes the cards the cycle chose
instead of choosing again.  The pools stay the ledger across cycles.

``exact`` stays on the host path (logged once) for an inventory with a node
above 16 cards, a card of 2^28 MiB or more, or a card whose ledger holds
what the planes do not (negative usage, 2^28 slices or more), and is
ignored under the soft-shard coordinator and by preempt/reclaim."""

from __future__ import annotations

import logging
from typing import Dict, List, Optional

import numpy as np

from ...api.devices import ANN_ASSIGNED, DeviceRequest, GPUDevicePool
from ...ops.reference import (DEV_GONE, DEV_MAX_CARDS, DEV_MEM_LIMIT,
                              device_slots)
from ..tensors import set_plane_bit
from .base import Plugin, register

log = logging.getLogger(__name__)
_warned_host_path = False


def _truthy(v) -> bool:
    return v is True or str(v).strip().lower() in ("true", "1", "yes")


class DeviceExact:
    """What ``exact: true`` publishes on the session
    (``ssn.device_exact``)."""

    def __init__(self, planes, unfit_bits) -> None:
        self.planes = planes            # mem_used, cores_used, state, total
        self.unfit_bits = unfit_bits    # request signature -> forbid bit
        # id(tclass) -> one card list per placed task (set by allocate
        # after the cycle, consumed by on_allocate)
        self.cards: Dict[int, List[List[int]]] = {}

    def unfit_nodes(self, sig) -> List[int]:
        """Node ids whose cards cannot pack one pod of the shape now."""
        import torch
        slots = device_slots(*(torch.from_numpy(a) for a in self.planes),
                             sig)
        return np.nonzero(slots.sum(0) < sig[0])[0].tolist()

    def request_of(self, task) -> Optional[DeviceRequest]:
        """The device request of a task, when the planes can express it."""
        if task.pod is None:
            return None
        rq = DeviceRequest.from_annotations(task.pod.meta.annotations)
        # a request the planes cannot express keeps the host bit
        if rq is None or rq.count < 1 or not 0 <= rq.cores <= 100 \
                or not 0 <= rq.memory < DEV_MEM_LIMIT:
            return None
        return rq


def card_planes(pools, nodes, n: int):
    """The pools as int32 card planes [K, N] + mem_total [N], or None when
    the inventory does not fit them (K > 16, a card of >= 2^28 MiB, a card
    with negative usage or with 2^28 slices or more: the ranges
    ``plan.set_device_state`` checks)."""
    K = max((len(p.cards) for p in pools.values()), default=0)
    if K == 0 or K > DEV_MAX_CARDS:
        return None
    mem_used = np.zeros((K, n), dtype=np.int32)
    cores_used = np.zeros((K, n), dtype=np.int32)
    state = np.full((K, n), DEV_GONE, dtype=np.int32)
    mem_total = np.zeros(n, dtype=np.int32)
    for name, pool in pools.items():
        ni = nodes.get(name)
        if ni is None or not 0 <= ni.node_id < n or not pool.cards:
            continue
        total = pool.cards[0].mem_total
        if any(c.mem_total != total for c in pool.cards) or \
                not 0 <= total < DEV_MEM_LIMIT:
            return None
        mem_total[ni.node_id] = total
        for k, c in enumerate(pool.cards):
            if not 0 <= c.mem_used < 1 << 31 or \
                    not 0 <= c.cores_used < 1 << 31 or \
                    not 0 <= c.slices < DEV_MEM_LIMIT:
                return None
            mem_used[k, ni.node_id] = c.mem_used
            cores_used[k, ni.node_id] = c.cores_used
            state[k, ni.node_id] = c.slices | (DEV_GONE if c.exclusive else 0)
    return mem_used, cores_used, state, mem_total


@register("deviceshare")
class DeviceSharePlugin(Plugin):
    def on_session_open(self, ssn) -> None:
        nt = ssn.node_tensors
        # pools persist across cycles on the cache (usage carries over)
        pools: Dict[str, GPUDevicePool] = getattr(
            ssn.cache, "_device_pools", None) or {}
        for name, ni in ssn.nodes.items():
            if name not in pools:
                pool = GPUDevicePool(ni.node)
                if pool.cards:
                    pools[name] = pool
        ssn.cache._device_pools = pools
        if not pools:
            return
        self.pools = pools
        unfit_bits: Dict[tuple, int] = {}

        def request_of(tclass) -> DeviceRequest:
            pod = tclass.tasks[0].pod
            if pod is None:
                return None
            return DeviceRequest.from_annotations(pod.meta.annotations)

        def hook(tclass, job, require, forbid):
            req = request_of(tclass)
            if req is None:
                return
            sig = req.signature()
            bit = unfit_bits.get(sig)
            if bit is None:
                # The words are memoized per (signature, queue) and shared
                # with the consumers that keep the host path under exact
                # (preempt/reclaim, nomination, subgroups), so the bit is
                # built either way — under exact from the card planes in
                # one array pass (a node fits one pod iff S >= count)
                if published is not None and \
                        published.request_of(tclass.tasks[0]) is not None:
                    unfit = published.unfit_nodes(sig)
                else:
                    unfit = []
                    for name, ni in ssn.nodes.items():
                        pool = pools.get(name)
                        if pool is None or pool.fit(req) is None:
                            unfit.append(ni.node_id)
                bit = nt.add_dynamic_bit(f"dev-unfit:{sig}", unfit)
                unfit_bits[sig] = bit
            set_plane_bit(forbid, bit)

        node_by_id = {ni.node_id: ni for ni in ssn.nodes.values()}

        published = None
        if _truthy(self.args.get("exact", False)):
            planes = card_planes(pools, ssn.nodes, nt.n)
            if planes is not None:
                published = DeviceExact(planes, unfit_bits)
                ssn.device_exact = published
            else:
                global _warned_host_path
                if not _warned_host_path:
                    _warned_host_path = True
                    log.warning(
                        "deviceshare: exact is off — the inventory has a "
                        "node above %d cards, cards of unequal size on one "
                        "node, a card of 2^28 MiB or more, or a card with "
                        "negative usage or 2^28 slices or more; per-card "
                        "packing stays on the host path", DEV_MAX_CARDS)

        def take_chosen(pool, req, cards):
            """The cards the cycle chose for one pod join the ledger."""
            for idx in cards:
                pool.cards[idx].take(req)
            return cards

        def on_allocate(tclass, node_ids, counts, tasks=None):
            req = request_of(tclass)
            if req is None:
                return
            # exact: one card list per placed task, in log order — popped,
            # because the walk fires once per device class (allocate.py
            # states the two invariants); a class the cycle did not pack
            # (nomination, subgroups) finds nothing and chooses here
            chosen = published.cards.pop(id(tclass), None) \
                if published is not None else None
            chosen = iter(chosen) if chosen is not None else None
            it = iter(tasks if tasks is not None else tclass.tasks)
            for nid, cnt in zip(node_ids, counts):
                ni = node_by_id.get(nid)
                pool = pools.get(ni.name) if ni else None
                for _ in range(cnt):
                    task = next(it, None)
                    if task is None:
                        return
                    if chosen is not None:
                        cards = next(chosen, None)
                        picked = take_chosen(pool, req, cards) \
                            if pool and cards else None
                    else:
                        picked = pool.allocate(req) if pool else None
                    if picked is not None and task.pod is not None:
                        task.pod.meta.annotations[ANN_ASSIGNED] = \
                            ",".join(str(i) for i in picked)

        handler = type("DevHandler", (), {"on_allocate":
                                          staticmethod(on_allocate)})()
        ssn.class_constraint_hooks.append(hook)
        ssn.event_handlers.append(handler)

        # GPU binpack/spread node scoring (reference deviceshare.go:233-285
        # NodeOrder): classes carrying a device request get a bias plane
        # favoring fuller (binpack, default) or emptier (spread) nodes'
        # device pools — per-card fill averaged per node.
        import numpy as np
        mode = str(self.args.get("deviceshare.schedule-policy", "binpack"))
        weight = float(self.args.get("deviceshare.gpu-score-weight", 0.05))
        if weight > 0:
            N = nt.n
            fill = np.zeros(N, dtype=np.float32)
            pooled = np.zeros(N, dtype=bool)
            for name, pool in pools.items():
                ni = ssn.nodes.get(name)
                if ni is None or ni.node_id < 0 or not pool.cards:
                    continue
                f = sum((c.mem_used / max(c.mem_total, 1)) if not c.exclusive
                        else 1.0 for c in pool.cards) / len(pool.cards)
                fill[ni.node_id] = f
                pooled[ni.node_id] = True
            bias_row = (weight * fill if mode == "binpack"
                        else -weight * fill).astype(np.float32)
            bias_row[~pooled] = 0.0

            def gpu_bias(tclass, job):
                return bias_row if request_of(tclass) is not None else None

            ssn.class_bias_fns.append(gpu_bias)
