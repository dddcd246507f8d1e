"""Worlds, driver and host truth for the device-state coherence tests.

After an action has run, ``NodeTensors.used_t`` and ``ssn.queue_alloc`` are
what the in-kernel commits and discards left, corrected by the host give-backs
of the apply (``AllocateAction._revert_pieces``) and the direct writes of
``_try_nominated``.  Nothing re-packs the device before the next action of
the session reads those tensors, so they have to equal what the host applied.
This module builds small scheduler worlds (store -> ``SchedulerCache`` ->
``Scheduler``), runs a session one action at a time and, after each action,
compares the device tensors and the ledger with a *host truth* that is summed
in float64 from the task objects alone:

* ``used[node, dim]``  = sum of the requests of the node's tasks whose status
  occupies the node or is ``RELEASING`` (what ``NodeInfo.add_task``
  accounts), plus the node's ``remote_used``;
* ``queue[q, dim]``    = sum of the requests of the queue's jobs' tasks in
  ``ALLOCATED_STATUSES`` (what ``JobInfo.allocated_resource`` counts).

Why the inputs are exact.  Every scenario requests CPU in whole millicores,
memory in whole GiB and one pod per task.  Per node the CPU sums stay below
2^24 millicores, the memory sums are k * 2^30 with k < 2^24, and the pod
counts are small integers; per queue the largest sums of any scenario are
1536 tasks of 1000 millicores and 1 GiB.  All of these, and every partial
sum and every ``count * request`` product on the way, are integers (or an
integer times 2^30) with fewer than 24 significant bits, so each f32 add,
subtract and multiply of the kernels, of the torch oracle and of
``_revert_pieces`` is exact in any order, fused or not.  The assertions are
therefore plain equality: ``used_t.double() == truth`` and
``queue_alloc.double() == truth``.  The one byte-scale twin
(``bundle_short_bytes``: memory ``1500M``) is where f32 rounds; its bound is
derived in ``byte_bound``.

This is a plain module: no fixtures, no collection hooks.
"""

from __future__ import annotations

import contextlib
from dataclasses import dataclass, field
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

import volcano_amd.scheduler.actions.allocate as alloc_mod
import volcano_amd.scheduler.actions.backfill as backfill_mod
from volcano_amd.api.ledger import USED
from volcano_amd.api.types import ALLOCATED_STATUSES, TaskStatus
from volcano_amd.scheduler import (FakeBinder, Scheduler, SchedulerCache,
                                   default_config)
from volcano_amd.scheduler.actions.allocate import AllocateAction
from volcano_amd.scheduler.config import PluginOption, Tier
from volcano_amd.store import ObjectStore
from volcano_amd.utils import synth
from volcano_amd.utils.metrics import METRICS

GI = 1024 ** 3
MB = 1000 ** 2


# -- host truth ---------------------------------------------------------------

def host_truth(cache, ssn):
    """(used [N, R], queue [Q, R]) in float64, from the task objects alone."""
    nt = cache.node_tensors
    didx = nt.dims.index
    R = nt.r
    used = np.zeros((nt.n, R), dtype=np.float64)
    queue = np.zeros((len(ssn.queue_index), R), dtype=np.float64)
    for job in cache.jobs.values():
        qi = ssn.queue_index.get(job.queue)
        for t in job.tasks.values():
            vec = np.zeros(R, dtype=np.float64)
            for k, v in t.request.q.items():
                i = didx.get(k)
                if i is not None:
                    vec[i] = v
            if t.node_name and (t.status.occupies_node
                                or t.status == TaskStatus.RELEASING):
                nid = nt.index.get(t.node_name)
                if nid is not None:
                    used[nid] += vec
            if qi is not None and t.status in ALLOCATED_STATUSES:
                queue[qi] += vec
    for ni in cache.nodes.values():
        for k, v in ni.remote_used.q.items():
            i = didx.get(k)
            if i is not None and ni.node_id >= 0:
                used[ni.node_id, i] += v
    return used, queue


@dataclass
class Report:
    """State after one action of one session.  ``used_t`` is read first:
    nothing below it touches the device."""
    cycle: int
    action: str
    used_t: np.ndarray          # [N, R] f32 -> f64, the device tensor
    queue_alloc: np.ndarray     # [Q, R] f32 -> f64
    ledger_used: np.ndarray     # [N, R] f64, the ledger's USED plane
    truth_used: np.ndarray      # [N, R] f64
    truth_queue: np.ndarray     # [Q, R] f64
    queue_checked: bool = True


def take_report(world, ssn, cycle: int, action: str) -> Report:
    nt = ssn.node_tensors
    used_t = nt.used_t.detach().cpu().double().numpy().T.copy()
    qa = ssn.queue_alloc.detach().cpu().double().numpy().copy()
    R = nt.r
    led = world.cache.ledger.planes[USED, :, :R].copy()
    tu, tq = host_truth(world.cache, ssn)
    if qa.shape[1] < R:     # dims a plugin added after the queue rows
        qa = np.pad(qa, ((0, 0), (0, R - qa.shape[1])))
    # evict and pipeline move the statuses but not the queue rows
    return Report(cycle, action, used_t, qa, led, tu, tq,
                  queue_checked=action not in world.scenario.queue_unchecked)


def assert_coherent(rep: Report) -> None:
    """Equality of all three ``used`` sources and of the queue rows."""
    where = f"cycle {rep.cycle} after {rep.action}"
    for name, got in (("ledger", rep.ledger_used), ("used_t", rep.used_t)):
        bad = np.argwhere(got != rep.truth_used)
        assert bad.size == 0, (
            f"{where}: {name} != truth at {len(bad)} (node, dim) cells, "
            f"first {bad[0].tolist()}: {got[tuple(bad[0])]} vs "
            f"{rep.truth_used[tuple(bad[0])]}")
    if rep.queue_checked:
        bad = np.argwhere(rep.queue_alloc != rep.truth_queue)
        assert bad.size == 0, (
            f"{where}: queue_alloc != truth at {bad.tolist()}: "
            f"{rep.queue_alloc[tuple(bad[0])]} vs "
            f"{rep.truth_queue[tuple(bad[0])]}")


# -- what a run records -----------------------------------------------------------

@dataclass
class Run:
    """One runner call: the plan and copies of the result arrays as the
    runner returned them (the apply mutates the originals)."""
    action: str
    plan: object
    job_flag: np.ndarray
    class_placed: np.ndarray
    log_len: np.ndarray
    log_nodes: np.ndarray
    log_counts: np.ndarray

    def entries(self, c: int):
        cp = self.plan.classes[c]
        n = int(self.log_len[c])
        sl = slice(cp.log_off, cp.log_off + n)
        return self.log_nodes[sl], self.log_counts[sl]

    def class_index(self, cp) -> int:
        for c, x in enumerate(self.plan.classes):
            if x is cp:
                return c
        return -1


@dataclass
class Revert:
    """One ``_revert_pieces`` call."""
    job_key: str
    bundle: bool
    pieces: list
    partial_first: bool     # pieces[0] gives back less than its log entry


# -- scenarios ----------------------------------------------------------------------

@dataclass
class Scenario:
    name: str
    populate: Callable          # (store) -> None: nodes, queues, jobs
    conditions: Callable        # (world) -> {name: bool}
    actions: List[str] = field(
        default_factory=lambda: ["enqueue", "allocate", "backfill"])
    cycles: int = 1
    between: Optional[Callable] = None     # (world, finished cycle) -> None
    tiers: Optional[Callable] = None       # () -> List[Tier]
    coordinator: bool = False
    give_back: bool = False     # the condition involves a host give-back
    queue_unchecked: tuple = ()
    n_nodes: int = 0


def gang(store, name, replicas, *, cpu=1000, mem=GI, min_member=None,
         queue="default", priority=0, role="worker", policy=None,
         affinity=None, bound_on=None):
    """PodGroup + pods.  No ``minResources``: enqueue admits every gang, the
    shortage is left to the allocate cycle.  ``bound_on`` binds the first
    pods to the named nodes before the scheduler ever sees them."""
    pg = synth.make_podgroup(
        name, queue=queue,
        min_member=replicas if min_member is None else min_member)
    if policy is not None:
        pg.spec.sub_group_policy = policy
    store.create("PodGroup", pg)
    for i in range(replicas):
        p = synth.make_pod(f"{name}-{role}-{i}", name, queue=queue,
                           cpu_milli=cpu, mem=mem, role=role,
                           priority=priority)
        if affinity is not None:
            p.affinity = dict(affinity)
        if bound_on and i < len(bound_on):
            p.node_name = bound_on[i]
        store.create("Pod", p)


def roles_gang(store, name, roles, *, priority=0, min_member=None,
               affinity_of=None):
    """One gang of several roles: roles = [(role, replicas, cpu), ...]."""
    total = sum(n for _, n, _ in roles)
    pg = synth.make_podgroup(
        name, min_member=total if min_member is None else min_member,
        min_task_member={r: n for r, n, _ in roles})
    store.create("PodGroup", pg)
    for role, n, cpu in roles:
        for i in range(n):
            p = synth.make_pod(f"{name}-{role}-{i}", name, cpu_milli=cpu,
                               mem=GI, role=role, priority=priority)
            if affinity_of and role in affinity_of:
                p.affinity = dict(affinity_of[role])
            store.create("Pod", p)


def nodes(store, n, cpu, mem=64 * GI, prefix="node", labels=None):
    for node in synth.make_nodes(n, prefix=prefix, cpu_milli=cpu, mem=mem,
                                 labels=labels):
        store.create("Node", node)


def bound_tasks(world, prefix=""):
    return sum(1 for k in world.binder.binds
               if k.startswith(f"default/{prefix}"))


def allocate_runs(world):
    return [r for r in world.runs if r.action == "allocate"]


# 1. small gangs ------------------------------------------------------------------

SMALL_GANGS = 40


def _small_gangs(store):
    """64 nodes x 4 cores; 40 gangs of 4..9 tasks of 1 or 2 cores, each with
    a priority of its own (the priority is part of the class signature, so
    no two gangs fuse).  Demand exceeds the 256 cores: the gangs at the end
    of the order find partial room and are discarded in-kernel, smaller ones
    behind them still commit."""
    nodes(store, 64, cpu=4000)
    store.create("Queue", synth.make_queue("default"))
    rng = np.random.RandomState(5)
    for j in range(SMALL_GANGS):
        gang(store, f"sg-{j:02d}", int(rng.randint(4, 10)),
             cpu=int(rng.choice([1000, 2000])), priority=100 - j)


def _small_gangs_cond(world):
    run = allocate_runs(world)[0]
    plan = run.plan
    single = [j for j, jp in enumerate(plan.jobs)
              if jp.class_end - jp.class_begin == 1]
    discarded = [j for j in single
                 if not run.job_flag[j]
                 and run.class_placed[plan.jobs[j].class_begin] == 0
                 and run.log_len[plan.jobs[j].class_begin] > 0]
    committed = [j for j in single if run.job_flag[j]
                 and run.class_placed[plan.jobs[j].class_begin] > 0]
    last_commit = max(committed, default=-1)
    return {
        "at least 32 single-class jobs": len(single) >= 32,
        "gangs discarded in-kernel after partial placement":
            len(discarded) >= 2,
        "gangs commit": len(committed) >= 8,
        "a gang commits behind a discarded one":
            any(j < last_commit for j in discarded),
    }


# 2. two-role gang, second role short ---------------------------------------------

def _two_role(store):
    """Role ``a`` (2 x 1 core) places, role ``b`` (3 x 4 cores) finds only
    two empty nodes: the job reverts on the device.  A plain gang behind it
    commits on what the revert gave back."""
    nodes(store, 3, cpu=4000)
    store.create("Queue", synth.make_queue("default"))
    roles_gang(store, "short", [("a", 2, 1000), ("b", 3, 4000)], priority=10)
    gang(store, "after", 3, cpu=4000, priority=1)


def _two_role_cond(world):
    run = allocate_runs(world)[0]
    plan = run.plan
    multi = [j for j, jp in enumerate(plan.jobs)
             if jp.class_end - jp.class_begin > 1]
    reverted = [j for j in multi if not run.job_flag[j] and any(
        run.log_len[c] > 0 for c in range(plan.jobs[j].class_begin,
                                          plan.jobs[j].class_end))]
    return {
        "multi-class job reverted on device after placements":
            len(reverted) == 1,
        "nothing of it bound": bound_tasks(world, "short") == 0,
        "the gang behind it commits": bound_tasks(world, "after") == 3,
        "no host give-back": not world.reverts,
    }


# 3. bundle with a short cluster -----------------------------------------------------

BUNDLE_GANGS = 400


def _bundle_short(mem):
    def populate(store):
        """512 nodes with room for 3 tasks (one of them for 1), 400 identical
        gangs of 4: one fused run of 1600 tasks over 1534 slots.  Pieces
        straddle log entries; 383 gangs commit, the 384th misses and
        recycles, and the 2 slots left over begin inside a 3-entry."""
        nodes(store, 511, cpu=3000, mem=8 * GI)
        nodes(store, 1, cpu=1000, mem=8 * GI, prefix="small")
        store.create("Queue", synth.make_queue("default"))
        for j in range(BUNDLE_GANGS):
            gang(store, f"bg-{j:03d}", 4, cpu=1000, mem=mem)
    return populate


def tail_position(run, c, gang_size):
    """(slots, committed gangs, tail slots, tail begins mid-entry)."""
    _, lc = run.entries(c)
    total = int(lc.sum())
    kept = total // gang_size * gang_size
    mid = kept < total and kept not in set(np.cumsum(lc).tolist())
    return total, total // gang_size, total - kept, mid


def _bundle_short_cond(world):
    run = allocate_runs(world)[0]
    plan = run.plan
    big = [c for c, cp in enumerate(plan.classes)
           if cp.bundle is not None and cp.ntasks >= 512]
    out = {"one fused run of >= 512 tasks on N = 512":
           len(big) == 1 and plan.nt.n == 512}
    if not big:
        return out
    total, gangs, tail, mid = tail_position(run, big[0], 4)
    tails = [r for r in world.reverts if r.bundle]
    out.update({
        "room is short of demand": total < plan.classes[big[0]].ntasks,
        "pieces straddle log entries": int(run.entries(big[0])[1].max()) < 4,
        "unclaimed tail begins mid-entry": tail > 0 and mid,
        "_revert_pieces got the partial first piece":
            len(tails) == 1 and tails[0].partial_first
            and sum(c for _, c in tails[0].pieces) == tail,
        "a gang missed and recycled its slots":
            bound_tasks(world) == gangs * 4 and gangs < BUNDLE_GANGS,
    })
    stats = getattr(world.allocate, "last_walk_stats", None)
    if stats is not None:       # native walk: (committed, missed, lost, tail)
        out["native walk counted the miss and the tail"] = \
            stats[0] == gangs and stats[1] >= 1 and stats[3] >= 1
    return out


# 4. bundle cut by queue capability ---------------------------------------------------

def _bundle_quota(store):
    """Room for everything, but the queue's capability is 10 cores: the
    fused run of 5 gangs of 4 stops after 10 tasks, inside the third gang,
    whose 2 slots the walk gives back."""
    nodes(store, 16, cpu=3000)
    store.create("Queue", synth.make_queue(
        "default", capability={"cpu": 10000}))
    for j in range(5):
        gang(store, f"qg-{j}", 4)


def _bundle_quota_cond(world):
    run = allocate_runs(world)[0]
    plan = run.plan
    fused = [c for c, cp in enumerate(plan.classes)
             if cp.bundle is not None and len(cp.bundle) == 5]
    out = {"one fused run of the 5 gangs": len(fused) == 1}
    if not fused:
        return out
    total, gangs, tail, _ = tail_position(run, fused[0], 4)
    tails = [r for r in world.reverts if r.bundle]
    out.update({
        "the quota ends the fill inside a gang": (total, gangs, tail)
            == (10, 2, 2),
        "the tail gang is given back":
            len(tails) == 1 and sum(c for _, c in tails[0].pieces) == 2,
        "two gangs bound": bound_tasks(world) == 8,
    })
    return out


# 5. minSubGroups family below its minimum ------------------------------------------

def _subgroup_family(store):
    """Three subgroups of 2 x 2 cores, the family needs all three; 5 nodes of
    2 cores hold two.  Both placed subgroups are reverted by the host gate.
    A plain gang behind the family then finds the room."""
    nodes(store, 5, cpu=2000)
    store.create("Queue", synth.make_queue("default"))
    gang(store, "fam", 6, cpu=2000, min_member=1, priority=10,
         policy=[{"subGroupSize": 2, "minSubGroups": 3}])
    gang(store, "plain", 1, cpu=1000, priority=1)


def _subgroup_family_cond(world):
    run = allocate_runs(world)[0]
    plan = run.plan
    sub = [c for c, cp in enumerate(plan.classes) if "#sg" in cp.job_key]
    placed = [c for c in sub if run.job_flag[plan.class_job[c]]
              and run.class_placed[c] > 0]
    gated = [r for r in world.reverts if "#sg" in r.job_key]
    return {
        "three subgroup classes, two placed on device":
            len(sub) == 3 and len(placed) == 2,
        "_gate_subgroup_families reverted the placed ones":
            len(gated) == 2
            and sum(c for r in gated for _, c in r.pieces) == 4,
        "nothing of the family bound": bound_tasks(world, "fam") == 0,
        "the plain gang bound": bound_tasks(world, "plain") == 1,
    }


# 6. spread role in a gang that reverts ---------------------------------------------

SPREAD = {"topologySpread": {"group": "web", "topologyKey": "zone",
                             "maxSkew": 1}}


def _domain_tiers():
    return [
        Tier(plugins=[PluginOption(n)
                      for n in ("priority", "gang", "conformance")]),
        Tier(plugins=[PluginOption(n) for n in (
            "overcommit", "drf", "predicates", "nodeorder", "binpack")]
            + [PluginOption("topologyspread", arguments={"exact": True})])]


def _spread_revert(store):
    """Zones a, b, c; no pod fits in c.  With maxSkew 1 a spread class places
    one pod in a and one in b and stops.  ``solo`` (one spread class of 3,
    gang 3) is discarded; ``duo`` has a spread role that places 2 and a plain
    role that is short, so the whole job reverts; ``later`` (same spread
    group, min 1) must find the counts and the room it would have found
    alone."""
    for name, zone, cpu in (("big-a", "a", 64000), ("small-b", "b", 8000),
                            ("small-c", "c", 100)):
        store.create("Node", synth.make_node(name, cpu_milli=cpu,
                                             mem=256 * GI,
                                             labels={"zone": zone}))
    store.create("Queue", synth.make_queue("default"))
    gang(store, "solo", 3, cpu=500, priority=30, role="w", affinity=SPREAD)
    roles_gang(store, "duo", [("s", 2, 500), ("z", 2, 60000)], priority=20,
               affinity_of={"s": SPREAD})
    gang(store, "later", 2, cpu=500, min_member=1, priority=10, role="w",
         affinity=SPREAD)


def _spread_revert_cond(world):
    run = allocate_runs(world)[0]
    plan = run.plan
    spread = [c for c, cp in enumerate(plan.classes) if cp.spread is not None]
    rev = [c for c in spread if not run.job_flag[plan.class_job[c]]
           and run.log_len[c] > 0]
    multi = [c for c in rev
             if plan.jobs[plan.class_job[c]].class_end
             - plan.jobs[plan.class_job[c]].class_begin > 1]
    return {
        "spread classes routed through the exact select": len(spread) == 3,
        "spread classes reverted on device after placements": len(rev) == 2,
        "one of them inside a multi-class job": len(multi) == 1,
        "nothing of the reverted gangs bound":
            bound_tasks(world, "solo") + bound_tasks(world, "duo") == 0,
        "the later job of the group bound 2": bound_tasks(world, "later") == 2,
    }


# 7. soft-shard loser ---------------------------------------------------------------

class LoserCoordinator:
    """Stands in for ``SoftShardCoordinator`` in one process: no stagger, no
    collective.  It declares lost one node that a committed plain class used
    and one that an entry in the middle of a fused run used."""

    def __init__(self, world):
        self.world = world
        self.lost = ()
        self.finalized = 0

    def stagger_bias(self, nt):
        return torch.zeros(nt.n, dtype=torch.float32,
                           device=nt.alloc_t.device)

    def find_conflicts(self, nt, used_before):
        run = allocate_runs(self.world)[-1]
        plan = run.plan
        plain = bundle = None
        for c, cp in enumerate(plan.classes):
            if not run.job_flag[plan.class_job[c]] or not run.class_placed[c]:
                continue
            ln, lc = run.entries(c)
            hit = [int(n) for n, k in zip(ln, lc) if k > 0]
            if cp.bundle is None and plain is None:
                plain = hit[0]
            elif cp.bundle is not None and len(cp.bundle) >= 3 \
                    and bundle is None:
                bundle = next(n for n in hit[len(hit) // 2:] if n != plain)
        self.lost = tuple(n for n in (plain, bundle) if n is not None)
        return frozenset(self.lost)

    def finalize(self, ssn, nt, used_before):
        self.finalized += 1


def _softshard(store):
    """``part`` has one pod bound already, so its class is planned alone
    (a plain class); six identical gangs of 3 fuse into one run.  Node room
    is 2, so the entries of the run share nodes with their neighbours."""
    nodes(store, 16, cpu=2000)
    store.create("Queue", synth.make_queue("default"))
    gang(store, "part", 4, cpu=1000, min_member=2, priority=10,
         bound_on=["node-00015"])
    for j in range(6):
        gang(store, f"fz-{j}", 3, cpu=1000, priority=1)


def _softshard_cond(world):
    coord = world.allocate.coordinator
    plain = [r for r in world.reverts if not r.bundle]
    fused = [r for r in world.reverts if r.bundle]
    return {
        "two nodes declared lost": len(set(coord.lost)) == 2,
        "a plain class was given back": len(plain) == 1,
        "pieces of a fused run were given back":
            len(fused) == 1 and len(fused[0].pieces) >= 1,
        "the other gangs of the run bound":
            3 <= bound_tasks(world, "fz-") < 18
            and bound_tasks(world, "fz-") % 3 == 0,
        "nothing of the plain class bound": bound_tasks(world, "part") == 0,
        "finalize ran": coord.finalized == 1,
    }


# 8. allocate then backfill in one session -----------------------------------------

def _backfill(store):
    """Gangs with requests for allocate (one of them short, so allocate
    leaves a give-back behind) and pods-only gangs, which backfill places on
    the state allocate left."""
    nodes(store, 6, cpu=3000)
    store.create("Queue", synth.make_queue("default"))
    for j in range(5):
        gang(store, f"al-{j}", 4, cpu=1000, priority=5)
    for j in range(3):
        gang(store, f"be-{j}", 5, cpu=0, mem=0, min_member=1, priority=1)


def _backfill_cond(world):
    bf = [r for r in world.runs if r.action == "backfill"]
    al = allocate_runs(world)
    pods = world.cache.node_tensors.dims.index["pods"]
    after_alloc = [r for r in world.reports if r.action == "allocate"][0]
    after_bf = [r for r in world.reports if r.action == "backfill"][0]
    return {
        "allocate and backfill each ran one plan": len(al) == len(bf) == 1,
        "allocate left a give-back": any(r.bundle for r in world.reverts),
        "allocate bound 4 gangs": bound_tasks(world, "al-") == 16,
        "backfill bound the pods-only tasks":
            bound_tasks(world, "be-") == 15,
        "backfill moved only the pods dim":
            after_bf.truth_used[:, pods].sum()
            == after_alloc.truth_used[:, pods].sum() + 15
            and np.array_equal(np.delete(after_bf.truth_used, pods, axis=1),
                               np.delete(after_alloc.truth_used, pods,
                                         axis=1)),
    }


# 9. preempt, then the next cycle ---------------------------------------------------

PREEMPT_ACTIONS = ["enqueue", "allocate", "preempt"]


def _preempt(store):
    nodes(store, 4, cpu=2000, mem=8 * GI)
    store.create("Queue", synth.make_queue("default"))
    gang(store, "low", 8, cpu=1000, min_member=1, priority=1)


def _preempt_between(world, cycle):
    if cycle == 0:
        # the high-priority gang arrives once the cluster is full
        gang(world.store, "high", 3, cpu=1000, priority=100)
    elif cycle == 1:
        world.nominated_before = METRICS.counter("allocate:nominated_fastpath")
        world.pipelined = sorted(
            t.node_name for t in world.cache.jobs["default/high"]
            .tasks.values() if t.status == TaskStatus.PIPELINED)
        # the evicted pods terminate
        for key in list(world.binder.evictions):
            ns, name = key.split("/", 1)
            world.store.delete("Pod", ns, name)


def _preempt_cond(world):
    high = world.cache.jobs["default/high"]
    after_preempt = [r for r in world.reports
                     if r.cycle == 1 and r.action == "preempt"][0]
    before_preempt = [r for r in world.reports
                      if r.cycle == 1 and r.action == "allocate"][0]
    return {
        "cycle 0 filled the cluster": bound_tasks(world, "low") == 8,
        "preempt evicted 3 and pipelined the gang":
            len(world.binder.evictions) == 3 and len(world.pipelined) == 3,
        "evict and pipeline left used where it was":
            np.array_equal(after_preempt.truth_used,
                           before_preempt.truth_used),
        "the next cycle took the nominated fast path":
            METRICS.counter("allocate:nominated_fastpath")
            == world.nominated_before + 1,
        "the gang is bound on its nominated nodes":
            high.occupied_count == 3
            and sorted(t.node_name for t in high.tasks.values())
            == world.pipelined,
    }


SCENARIOS: Dict[str, Scenario] = {s.name: s for s in (
    Scenario("small_gangs", _small_gangs, _small_gangs_cond, n_nodes=64),
    Scenario("two_role_short", _two_role, _two_role_cond, n_nodes=3),
    Scenario("bundle_short", _bundle_short(GI), _bundle_short_cond,
             give_back=True, n_nodes=512),
    Scenario("bundle_quota", _bundle_quota, _bundle_quota_cond,
             give_back=True, n_nodes=16),
    Scenario("subgroup_family", _subgroup_family, _subgroup_family_cond,
             give_back=True, n_nodes=5),
    Scenario("spread_revert", _spread_revert, _spread_revert_cond,
             tiers=_domain_tiers, n_nodes=3),
    Scenario("softshard_loser", _softshard, _softshard_cond,
             coordinator=True, give_back=True, n_nodes=16),
    Scenario("allocate_backfill", _backfill, _backfill_cond,
             give_back=True, n_nodes=6),
    Scenario("preempt_nominated", _preempt, _preempt_cond,
             actions=PREEMPT_ACTIONS, cycles=3, between=_preempt_between,
             queue_unchecked=("preempt",), n_nodes=4),
)}

# the byte-scale twin of bundle_short: memory 1500M, where f32 rounds
BUNDLE_SHORT_BYTES = Scenario(
    "bundle_short_bytes", _bundle_short(1500 * MB), _bundle_short_cond,
    give_back=True, n_nodes=512)

BUNDLE_SCENARIOS = ("bundle_short", "bundle_quota")
GIVE_BACK = tuple(n for n, s in SCENARIOS.items() if s.give_back)


# -- world and driver -------------------------------------------------------------

class World:
    """store -> cache -> scheduler on ``device``: ``"cpu"`` runs the plans
    through ``run_plan_torch``, ``"cuda"`` through ``run_plan_hip``."""

    def __init__(self, scenario: Scenario, device: str = "cpu"):
        self.scenario = scenario
        self.device = device
        self.store = ObjectStore()
        self.binder = FakeBinder()
        scenario.populate(self.store)
        config = default_config()
        config.actions = list(scenario.actions)
        if scenario.tiers is not None:
            config.tiers = scenario.tiers()
        if device != "cpu":
            config.use_hip = True
            config.device = device
        self.cache = SchedulerCache(store=self.store, binder=self.binder,
                                    device=device)
        self.sched = Scheduler(self.cache, config)
        self.allocate = next(a for a in self.sched._actions
                             if a.name == "allocate")
        if scenario.coordinator:
            self.allocate.coordinator = LoserCoordinator(self)
        self.runs: List[Run] = []
        self.reverts: List[Revert] = []
        self.reports: List[Report] = []
        self._action = ""

    # the runners and _revert_pieces, wrapped to record what went through
    @contextlib.contextmanager
    def _recording(self):
        saved = [(m, n, getattr(m, n))
                 for m in (alloc_mod, backfill_mod)
                 for n in ("run_plan_torch", "run_plan_hip")]
        installed = AllocateAction.__dict__["_revert_pieces"]
        revert = installed.__func__

        def runner(real, hip):
            def run(plan):
                assert hip == (self.device != "cpu"), \
                    "the plan went to the wrong runner"
                res = real(plan)
                self.runs.append(Run(
                    self._action, plan, res.job_flag.copy(),
                    res.class_placed.copy(), res.log_len.copy(),
                    res.log_nodes.copy(), res.log_counts.copy()))
                return res
            return run

        def spy(plan, cp, pieces):
            pieces = [(int(n), int(c)) for n, c in pieces]
            partial = False
            if pieces and self.runs and self.runs[-1].plan is plan:
                run = self.runs[-1]
                c = run.class_index(cp)
                if c >= 0:
                    ln, lc = run.entries(c)
                    full = {int(n): int(k) for n, k in zip(ln, lc)}
                    partial = 0 < pieces[0][1] < full.get(pieces[0][0], 0)
            self.reverts.append(Revert(cp.job_key, cp.bundle is not None,
                                       pieces, partial))
            return revert(plan, cp, pieces)

        for m, n, fn in saved:
            setattr(m, n, runner(fn, n == "run_plan_hip"))
        AllocateAction._revert_pieces = staticmethod(spy)
        try:
            yield
        finally:
            for m, n, fn in saved:
                setattr(m, n, fn)
            AllocateAction._revert_pieces = installed

    def run_session(self, cycle: int) -> List[Report]:
        """One session, one action at a time, a report after each."""
        out = []
        with self._recording():
            ssn = self.sched.open_session()
            for action in self.sched._actions:
                self._action = action.name
                action.execute(ssn)
                out.append(take_report(self, ssn, cycle, action.name))
            self.sched.close_session(ssn)
        self.reports.extend(out)
        return out

    def run(self) -> List[Report]:
        sc = self.scenario
        for cycle in range(sc.cycles):
            self.run_session(cycle)
            if sc.between is not None and cycle + 1 < sc.cycles:
                sc.between(self, cycle)
        return self.reports

    def conditions(self) -> Dict[str, bool]:
        return self.scenario.conditions(self)

    def binds(self) -> Dict[str, str]:
        return dict(self.binder.binds)


# -- mutants ------------------------------------------------------------------------

def revert_nothing(plan, cp, pieces) -> None:
    """``_revert_pieces`` that gives nothing back."""


def make_drop_partial_first(world_ref: list):
    """``_revert_pieces`` that loses only the partial first piece of a fused
    run's unclaimed tail.  ``world_ref[0]`` is the world under test (set
    after construction: the mutant has to be installed first)."""
    real = AllocateAction.__dict__["_revert_pieces"].__func__

    def mutant(plan, cp, pieces):
        world = world_ref[0]
        pieces = list(pieces)
        if cp.bundle is not None and pieces and world.runs:
            run = world.runs[-1]
            c = run.class_index(cp)
            ln, lc = run.entries(c)
            full = {int(n): int(k) for n, k in zip(ln, lc)}
            if 0 < pieces[0][1] < full.get(pieces[0][0], 0):
                pieces = pieces[1:]
        return real(plan, cp, pieces)
    return mutant


# -- the byte-scale bound -------------------------------------------------------------

def ulp_f32(x: np.ndarray) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)


def byte_bound(world: World) -> np.ndarray:
    """[N, R] bound on ``|used_t - truth|`` after the allocate of a one-cycle
    world: ``(3 k + 1) / 2 * ulp_f32(alloc)``, k = log entries of the cycle
    naming the node.  Per entry: one rounding of the fused commit
    (``used += count * req``), and a product and an add in
    ``_revert_pieces`` if the host gives (part of) it back; the ``+ 1`` is
    the f64 -> f32 rounding of the pack.  Every intermediate is at most
    ``alloc`` (capacity bounds usage), so each rounding is at most half an
    ulp of ``alloc``."""
    nt = world.cache.node_tensors
    k = np.zeros(nt.n, dtype=np.float64)
    for run in allocate_runs(world):
        for c in range(len(run.plan.classes)):
            ln, _ = run.entries(c)
            np.add.at(k, ln.astype(np.int64), 1.0)
    alloc = nt.alloc_t.detach().cpu().numpy().T          # [N, R]
    return (3.0 * k[:, None] + 1.0) * 0.5 * ulp_f32(alloc)
