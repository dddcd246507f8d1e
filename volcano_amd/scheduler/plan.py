"""Cycle plan: the host-built launch schedule for one allocate pass.

The reference's allocate action walks queues→jobs→tasks with Go callbacks
per (task, node) (`actions/allocate/allocate.go:719-866`).  Here the host
builds a *plan* — an ordered array of task-class descriptors and job gang
descriptors — and the whole cycle executes as one enqueue:

* GPU path: a single ``vamd_run_cycle`` library call replays the plan as
  back-to-back HIP kernels on one stream, zero host syncs mid-cycle
  (``ops/csrc/cycle_runner.hip``); one D2H readback returns every
  placement.
* CPU path: the same plan interpreted over the torch oracle ops
  (``ops/reference.py``) — bit-identical decisions, used by the non-GPU
  test tier and as the golden reference for the HIP kernels.
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from ..api.info import JobInfo, TaskClass
from ..ops import reference as ref
from .tensors import NodeTensors

BIG_LIMIT = 1.0e18     # "no queue limit" sentinel (finite: kernel does int cast)

# binary-compatible numpy mirrors of VamdClassDesc / VamdJobDesc
# (ops/csrc/vamd_api.h) — the descriptor marshalling fills these columns
# instead of per-field ctypes stores (which cost ~10 µs per class)
CLASS_DT = np.dtype([
    ("job_idx", "<i4"), ("queue_idx", "<i4"), ("ntasks", "<i4"),
    ("min_needed", "<i4"), ("log_off", "<i4"), ("log_cap", "<i4"),
    ("flags", "<i4"), ("bias_row", "<i4"),
    ("w_least", "<f4"), ("w_most", "<f4"), ("w_bal", "<f4"),
    ("_padf", "<f4")])
JOB_DT = np.dtype([
    ("class_begin", "<i4"), ("class_end", "<i4"),
    ("occupied", "<i4"), ("min_available", "<i4")])


@dataclass(slots=True)
class BundleEntry:
    """One gang job inside a fused bundle class (see ClassPlan.bundle)."""
    job_key: str
    tasks: list                # the job's pending TaskInfos (class order)
    ntasks: int
    min_needed: int            # gang minimum for THIS job
    job: object = None         # JobInfo ref (skips the apply-time lookup)


@dataclass(slots=True)
class SpreadGroup:
    """One domain group of a cycle (topology spread, or inter-pod
    (anti-)affinity over a topology key): the node → domain map and the
    group's member count per domain at cycle start.  The runners keep the
    live counts on the device for the whole cycle (every class of the
    group, in plan order, sees its predecessors' placements and reverts);
    nothing is read back — the next session recounts from task statuses."""
    dom_of: np.ndarray         # [N] i32, -1 = node lacks the topology label
    count: np.ndarray          # [D] i32, 1 <= D <= N
    # network-topology group (ClassPlan.hypernode): ``dom_of`` is the
    # shared leaf row ``row`` of CyclePlan.hypernode_rows, ``count`` the
    # read-only table of the rule, ``leaves`` the row's leaf count
    row: int = -1
    leaves: int = 0


@dataclass(slots=True)
class DeviceState:
    """Per-card state of the inventory at cycle start (deviceshare with
    ``exact: true``): int32 card planes ``[K, N]``, K <= 16, laid out like
    the resource planes.  ``state`` is the slice count with
    ``ref.DEV_GONE`` set for an exclusive card and for the missing cards of
    a node with fewer than K.  The runners keep the live planes for the
    whole cycle; the host pools stay the ledger across cycles."""
    mem_used: np.ndarray       # [K, N] i32
    cores_used: np.ndarray     # [K, N] i32, percent
    state: np.ndarray          # [K, N] i32
    mem_total: np.ndarray      # [N] i32, < 2^28


@dataclass(slots=True)
class ClassPlan:
    tclass: TaskClass
    job_key: str
    queue_idx: int
    req: np.ndarray            # [R] f32
    tolerated: int
    require: np.ndarray        # [W] i64
    forbid: np.ndarray         # [W] i64
    min_needed: int            # per-role minimum still missing
    w_least: float = 1.0
    w_most: float = 0.0
    w_bal: float = 0.0
    use_future: bool = False   # score against future-idle (pipelining)
    # optional per-class additive score plane [N] f32 (task-topology
    # bucket packing); overrides the plan-wide bias for this class —
    # builders that want both must pre-add plan.bias into the row
    bias: Optional[np.ndarray] = None
    log_off: int = 0
    log_cap: int = 0
    # instance count override (bundles track the sum here instead of
    # materializing a merged 100k-task list; tclass keeps ONE
    # representative task for constraint/handler access)
    ntasks_override: Optional[int] = None
    # Gang bundling: consecutive jobs with identical single-class shape are
    # fused into ONE kernel pass (ntasks = sum); the per-job gang
    # boundaries live here and are enforced at apply time (slot walk with
    # recycling).  The kernel-side fuse_min is the EASIEST entry's
    # minimum: if even that gang can't place, the bundle reverts in-kernel.
    bundle: Optional[List[BundleEntry]] = None
    # (index into CyclePlan.spread_groups, maxSkew >= 1): the class is
    # placed by the per-placement topology-spread select instead of
    # select_commit.  Never combined with ``bundle``.
    spread: Optional[Tuple[int, int]] = None
    # every (group, maxSkew) of a class under SEVERAL spread constraints
    # (zone and hostname, ...), 2 to ref.SPREAD_MAX_RULES of them over
    # distinct groups; ``spread`` is then rule 0.  Placed by the multi-rule
    # spread select, which holds every maxSkew before every placement.
    # Never combined with ``bundle``, ``affinity`` or ``hypernode``.
    spread_rules: Optional[List[Tuple[int, int]]] = None
    # one f32 weight per rule of a spread class (``spread_rules``, or
    # ``spread`` alone), 0 = hard.  A rule with a nonzero weight is soft
    # (whenUnsatisfiable: ScheduleAnyway): it never filters on counts, costs
    # its weight per member already in the node's domain before every
    # placement, and carries ref.SPREAD_SOFT_SKEW as a maxSkew that never
    # binds.  Any nonzero weight sends the class to spread_soft_select.
    spread_soft: Optional[List[float]] = None
    # (index into CyclePlan.spread_groups, mode): inter-pod affinity
    # (mode 1) or keyed anti-affinity (mode 2) enforced per placement over
    # the group's domains — domain mask + select_commit + count update.
    # Never combined with ``bundle`` or ``spread``.
    affinity: Optional[Tuple[int, int]] = None
    # index into CyclePlan.spread_groups of a network-topology group
    # (add_hypernode_group): domain mask mode 3 + select_commit, the domain
    # chosen on the device from the live cap.  Never combined with
    # ``bundle``, ``spread`` or ``affinity``.
    hypernode: Optional[int] = None
    # device request (count, memory, cores) packed per card on the device
    # (CyclePlan.add_device_request): device_cap after the score, the
    # slices taken by device_commit after the select.  Composes with every
    # domain rule; never combined with ``bundle``.
    device: Optional[Tuple[int, int, int]] = None
    # NUMA request (cpu millicores, policy: ref.NUMA_HARD /
    # ref.NUMA_BEST_EFFORT) pinned per zone on the device
    # (CyclePlan.add_numa_request): numa_cap after the score (hard only),
    # the zones taken by numa_commit after the select.  Composes with every
    # domain rule and with ``device``; never combined with ``bundle``.
    numa: Optional[Tuple[int, int]] = None
    # nodeorder ``exact: true``: the chosen node is scored again after every
    # placement (rescore_select in place of select_commit, behind the same
    # cap and mask kernels).  Composes with ``affinity``, ``hypernode``,
    # ``device`` and ``numa``; a spread class takes spread_rescore_select,
    # which holds its rules and re-scores; never combined with ``bundle``.
    rescore: bool = False

    @property
    def ntasks(self) -> int:
        return self.ntasks_override if self.ntasks_override is not None \
            else self.tclass.count

    @property
    def never_bundles(self) -> bool:
        """Carries a bias row, a domain rule, a device or a NUMA request, or
        re-scores per placement: the class is placed on its own."""
        return self.rescore or self.bias is not None \
            or self.spread is not None \
            or self.affinity is not None or self.hypernode is not None \
            or self.device is not None or self.numa is not None


@dataclass(slots=True)
class JobPlan:
    job_key: str
    class_begin: int
    class_end: int
    occupied: int
    min_available: int


@dataclass
class ClassResult:
    placements: List[Tuple[int, int]]   # (node_id, count)
    placed: int


class CycleResult:
    """Array-backed cycle outcome (one readback): per-class undo logs,
    placed counts, per-job commit flags.  The apply path consumes the
    numpy arrays directly; the dict/object views materialize lazily for
    cold consumers (subgroup gating, tests)."""

    def __init__(self, plan, log_nodes, log_counts, log_len, class_placed,
                 job_placed, job_flag, dev_assign=None, numa_assign=None):
        self.plan = plan
        self.dev_assign = dev_assign       # [L, K] i32, or None
        self.numa_assign = numa_assign     # [L, Z] i32, or None
        self.log_nodes = log_nodes
        self.log_counts = log_counts
        self.log_len = log_len
        self.class_placed = class_placed
        self.job_placed_arr = job_placed
        self.job_flag = job_flag
        self._committed = None
        self._class_results = None

    @property
    def job_committed(self) -> Dict[str, bool]:
        if self._committed is None:
            self._committed = {jp.job_key: bool(self.job_flag[j])
                               for j, jp in enumerate(self.plan.jobs)}
        return self._committed

    @property
    def job_placed(self) -> Dict[str, int]:
        return {jp.job_key: int(self.job_placed_arr[j])
                for j, jp in enumerate(self.plan.jobs)}

    def class_entries(self, c: int):
        """(nodes, counts) numpy views of class c's undo log."""
        cp = self.plan.classes[c]
        n = int(self.log_len[c])
        sl = slice(cp.log_off, cp.log_off + n)
        return self.log_nodes[sl], self.log_counts[sl]

    def class_cards(self, c: int) -> List[List[int]]:
        """Card indices of every placed task of device class c, one list
        per task, in log order (entry by entry, ``count`` slices each)."""
        cp = self.plan.classes[c]
        if cp.device is None or self.dev_assign is None:
            return []
        _, lc = self.class_entries(c)
        out: List[List[int]] = []
        for e, cnt in enumerate(lc.tolist()):
            if cnt > 0:
                out.extend(ref.device_cards(self.dev_assign[cp.log_off + e],
                                            cnt, cp.device[0]))
        return out

    def class_zones(self, c: int) -> List[Optional[int]]:
        """The NUMA zone of every placed task of NUMA class c (None: the
        pod is bound unpinned — best-effort only), in log order."""
        cp = self.plan.classes[c]
        if cp.numa is None or self.numa_assign is None:
            return []
        _, lc = self.class_entries(c)
        out: List[Optional[int]] = []
        for e, cnt in enumerate(lc.tolist()):
            if cnt > 0:
                out.extend(ref.numa_zones(self.numa_assign[cp.log_off + e],
                                          cnt))
        return out

    @property
    def class_results(self) -> List[ClassResult]:
        if self._class_results is None:
            out = []
            for c in range(len(self.plan.classes)):
                ln, lc = self.class_entries(c)
                entries = [(int(n), int(k)) for n, k in zip(ln, lc)
                           if k > 0]
                out.append(ClassResult(entries, int(self.class_placed[c])))
            self._class_results = out
        return self._class_results


class CyclePlan:
    """Ordered classes + gang jobs + packed per-class constraint tensors."""

    def __init__(self, nt: NodeTensors, queue_limit: torch.Tensor,
                 queue_alloc: torch.Tensor):
        self.nt = nt
        self.classes: List[ClassPlan] = []
        self.jobs: List[JobPlan] = []
        self.queue_limit = queue_limit          # [Q, R] f32 (host)
        self.queue_alloc = queue_alloc          # [Q, R] f32 (host)
        self.bias: Optional[torch.Tensor] = None
        self.dim_w = torch.ones(nt.r, dtype=torch.float32)
        self.log_total = 0
        self.spread_groups: List[SpreadGroup] = []
        # live per-domain counts of the last run (device tensors, one per
        # group) — left for inspection, never copied to the host here
        self.spread_counts = None
        # leaf_of rows ([N] i32, leaf count) shared by network-topology
        # groups, and the groups already made per (row, table)
        self.hypernode_rows: List[Tuple[np.ndarray, int]] = []
        self._hypernode_groups: Dict[Tuple[int, bytes], int] = {}
        # card planes at cycle start, and the live planes of the last run
        # (tensors on the runner's side, left for inspection)
        self.device_state: Optional[DeviceState] = None
        self.device_planes = None
        # zone plane [Z, N] i32 at cycle start, and the live plane of the
        # last run (a tensor on the runner's side, left for inspection)
        self.numa_state: Optional[np.ndarray] = None
        self.numa_plane = None

    def set_numa_state(self, zone_free) -> None:
        """The inventory's free millicores per NUMA zone ([Z, N] int32,
        0 for the missing zones of a smaller node)."""
        zone_free = np.ascontiguousarray(zone_free, dtype=np.int32)
        if zone_free.ndim != 2 or zone_free.shape[1] != self.nt.n or \
                not 1 <= zone_free.shape[0] <= ref.NUMA_MAX_ZONES:
            raise ValueError("numa state: zone_free is [Z, N] with "
                             f"1 <= Z <= {ref.NUMA_MAX_ZONES}")
        if zone_free.max(initial=0) >= ref.NUMA_FREE_LIMIT or \
                zone_free.min(initial=0) < 0:
            raise ValueError("numa state: zone_free outside [0, 2^28)")
        self.numa_state = zone_free

    def add_numa_request(self, cp: ClassPlan, cpu: int, policy: int) -> None:
        """Pin cp's instances per NUMA zone: ``cpu`` millicores each from
        one zone; ``policy`` ref.NUMA_HARD clamps the capacity,
        ref.NUMA_BEST_EFFORT pins what fits."""
        if self.numa_state is None:
            raise ValueError("numa request without numa state")
        if cp.bundle is not None:
            raise ValueError("numa classes never bundle")
        cp.numa = ref.check_numa_request(cpu, policy)

    def set_device_state(self, mem_used, cores_used, state,
                         mem_total) -> None:
        """The inventory's card planes ([K, N] / [N] int32)."""
        planes = [np.ascontiguousarray(a, dtype=np.int32)
                  for a in (mem_used, cores_used, state)]
        mem_total = np.ascontiguousarray(mem_total, dtype=np.int32)
        K = planes[0].shape[0] if planes[0].ndim == 2 else 0
        if not 1 <= K <= ref.DEV_MAX_CARDS or \
                any(a.shape != (K, self.nt.n) for a in planes) or \
                mem_total.shape != (self.nt.n,):
            raise ValueError("device state: card planes are [K, N] with "
                             f"1 <= K <= {ref.DEV_MAX_CARDS}, mem_total [N]")
        if mem_total.max(initial=0) >= ref.DEV_MEM_LIMIT or \
                mem_total.min(initial=0) < 0:
            raise ValueError("device state: mem_total outside [0, 2^28)")
        ref.check_card_planes(*planes)
        self.device_state = DeviceState(*planes, mem_total)

    def add_device_request(self, cp: ClassPlan, count: int, memory: int,
                           cores: int) -> None:
        """Pack cp's instances per card: ``count`` slices of (memory,
        cores) each; memory == cores == 0 asks for whole cards."""
        if self.device_state is None:
            raise ValueError("device request without device state")
        if cp.bundle is not None:
            raise ValueError("device classes never bundle")
        cp.device = ref.check_device_request((count, memory, cores))

    def add_hypernode_row(self, leaf_of, n_leaves: int) -> int:
        """Register a node → leaf map (leaves numbered depth-first over
        the HyperNode tree); every group built on it shares the upload."""
        leaf_of = np.ascontiguousarray(leaf_of, dtype=np.int32)
        if leaf_of.shape != (self.nt.n,):
            raise ValueError("hypernode row: leaf_of needs one entry per "
                             "node")
        if not 1 <= int(n_leaves) <= max(self.nt.n, 1):
            raise ValueError("hypernode row: leaf count outside [1, N]")
        if leaf_of.max(initial=-1) >= n_leaves or \
                leaf_of.min(initial=0) < -1:
            raise ValueError("hypernode row: leaf id out of range")
        self.hypernode_rows.append((leaf_of, int(n_leaves)))
        return len(self.hypernode_rows) - 1

    def add_hypernode_group(self, row_id: int, table) -> int:
        """One network-topology rule (``ref.hypernode_table``) over leaf
        row ``row_id``.  Identical (T, need, pin, soft, ranges) share one
        group, hence one table slice."""
        if not 0 <= row_id < len(self.hypernode_rows):
            raise ValueError(f"hypernode group: unknown row {row_id}")
        table = np.ascontiguousarray(table, dtype=np.int32)
        leaf_of, leaves = self.hypernode_rows[row_id]
        key = (row_id, table.tobytes())
        g = self._hypernode_groups.get(key)
        if g is None:
            ref.check_hypernode_table(table, leaves)
            self.spread_groups.append(
                SpreadGroup(leaf_of, table, row=row_id, leaves=leaves))
            g = self._hypernode_groups[key] = len(self.spread_groups) - 1
        return g

    def add_spread_group(self, dom_of, count) -> int:
        dom_of = np.ascontiguousarray(dom_of, dtype=np.int32)
        count = np.ascontiguousarray(count, dtype=np.int32)
        if dom_of.shape != (self.nt.n,):
            raise ValueError("spread group: dom_of needs one entry per node")
        if not 1 <= count.shape[0] <= max(self.nt.n, 1):
            raise ValueError("spread group: domain count outside [1, N]")
        if dom_of.max(initial=-1) >= count.shape[0] or \
                dom_of.min(initial=0) < -1:
            raise ValueError("spread group: domain id out of range")
        self.spread_groups.append(SpreadGroup(dom_of, count))
        return len(self.spread_groups) - 1

    def add_job(self, job: JobInfo, classes: List[ClassPlan]) -> None:
        if not classes:
            return
        begin = len(self.classes)
        self.classes.extend(classes)
        self.jobs.append(JobPlan(
            job_key=job.key, class_begin=begin, class_end=len(self.classes),
            occupied=job.occupied_count, min_available=job.min_available))

    def add_gang(self, cp: ClassPlan) -> None:
        """Append cp as a single-class gang of its own (a bundle, a fused
        run, a subgroup): the gang holds when ``cp.min_needed`` place."""
        self.jobs.append(JobPlan(
            job_key=cp.job_key, class_begin=len(self.classes),
            class_end=len(self.classes) + 1, occupied=0,
            min_available=cp.min_needed))
        self.classes.append(cp)

    def check_spread_rules(self, c: int, cp: ClassPlan) -> None:
        """``cp.spread_rules`` of class ``c`` against the plan's groups (part
        of ``finalize``; whoever sets the rules on a finalized plan runs it
        itself)."""
        if cp.spread_rules is None:
            return
        rules = [tuple(r) for r in cp.spread_rules]
        gs = [g for g, _ in rules]
        if not 1 <= len(rules) <= ref.SPREAD_MAX_RULES or \
                cp.spread is None or tuple(cp.spread) != rules[0]:
            raise ValueError(
                f"class {c}: 1 to {ref.SPREAD_MAX_RULES} spread rules, the "
                "first of them in ``spread``")
        if any(not 0 <= g < len(self.spread_groups) for g in gs):
            raise ValueError(f"class {c}: unknown spread group")
        if len(set(gs)) != len(gs):
            raise ValueError(f"class {c}: two spread rules over one group")
        if any(skew < 1 for _, skew in rules):
            raise ValueError(f"class {c}: maxSkew must be >= 1")
        if any(self.spread_groups[g].row >= 0 for g in gs):
            raise ValueError(f"class {c}: a spread rule names a hypernode "
                             "group")
        if sum(self.spread_groups[g].count.shape[0] for g in gs) \
                > ref.SPREAD_MULTI_LDS_DOMAINS:
            raise ValueError(
                f"class {c}: its spread rules have more than "
                f"{ref.SPREAD_MULTI_LDS_DOMAINS} domains in all")
        if cp.bundle is not None or cp.affinity is not None \
                or cp.hypernode is not None:
            raise ValueError(f"class {c}: several spread rules never "
                             "combine with bundle, affinity or hypernode")

    def check_spread_soft(self, c: int, cp: ClassPlan) -> None:
        """``cp.spread_soft`` of class ``c`` against its rules (part of
        ``finalize``)."""
        if cp.spread_soft is None:
            return
        rules = cp.spread_rules or ([cp.spread] if cp.spread else [])
        tws = np.asarray(cp.spread_soft, dtype=np.float32)
        if tws.shape != (len(rules),) or not rules \
                or not np.isfinite(tws).all():
            raise ValueError(f"class {c}: one finite weight per spread rule")
        if sum(self.spread_groups[g].count.shape[0]
               for (g, _), tw in zip(rules, tws) if tw != 0) \
                > ref.SPREAD_SOFT_LDS_DOMAINS:
            raise ValueError(
                f"class {c}: its soft spread rules have more than "
                f"{ref.SPREAD_SOFT_LDS_DOMAINS} domains in all")

    def finalize(self) -> None:
        """Assign undo-log slots (one contiguous region per class),
        normalize constraint widths (the label-bit registry may have
        grown while classes were built), and stage the per-class job
        index + request matrix both runners and the apply path share."""
        # per-class bias rows REPLACE the plan bias in the kernel — fold
        # the plan-wide plane (score_bias / soft-shard stagger) into them
        # so biased classes don't lose it.  Shared rows fold once.
        if self.bias is not None:
            pb = self.bias.cpu().numpy().astype(np.float32)
            originals = [cp.bias for cp in self.classes
                         if cp.bias is not None]     # pin ids during fold
            folded: Dict[int, np.ndarray] = {}
            for cp in self.classes:
                if cp.bias is not None:
                    nb = folded.get(id(cp.bias))
                    if nb is None:
                        nb = folded[id(cp.bias)] = \
                            (cp.bias + pb).astype(np.float32)
                    cp.bias = nb
            del originals
        self.nt.ensure_plane_width()
        W = self.nt.planes_t.shape[0] if self.nt.planes_t is not None \
            else max(self.nt.labels.words, 1)
        off = 0
        n = self.nt.n
        C = len(self.classes)
        self.req_np = np.empty((C, self.nt.r), dtype=np.float32)
        for c, cp in enumerate(self.classes):
            cp.log_off = off
            cp.log_cap = max(1, min(cp.ntasks, n))
            off += cp.log_cap
            if len(cp.require) < W:
                cp.require = np.pad(cp.require, (0, W - len(cp.require)))
            if len(cp.forbid) < W:
                cp.forbid = np.pad(cp.forbid, (0, W - len(cp.forbid)))
            self.req_np[c] = cp.req
            if cp.spread is not None:
                g, skew = cp.spread
                if not 0 <= g < len(self.spread_groups):
                    raise ValueError(f"class {c}: unknown spread group {g}")
                if skew < 1:
                    raise ValueError(f"class {c}: maxSkew must be >= 1")
                if cp.bundle is not None:
                    raise ValueError(f"class {c}: spread classes never "
                                     "bundle")
            self.check_spread_rules(c, cp)
            self.check_spread_soft(c, cp)
            if cp.affinity is not None:
                g, mode = cp.affinity
                if not 0 <= g < len(self.spread_groups):
                    raise ValueError(f"class {c}: unknown affinity group {g}")
                if mode not in (ref.AFFINITY, ref.ANTI_AFFINITY):
                    raise ValueError(f"class {c}: affinity mode must be 1 "
                                     "(affinity) or 2 (anti-affinity)")
                if cp.bundle is not None:
                    raise ValueError(f"class {c}: affinity classes never "
                                     "bundle")
                if cp.spread is not None:
                    raise ValueError(f"class {c}: one domain rule per class "
                                     "(spread and affinity both set)")
            if cp.hypernode is not None:
                g = cp.hypernode
                if not 0 <= g < len(self.spread_groups) or \
                        self.spread_groups[g].row < 0:
                    raise ValueError(f"class {c}: unknown hypernode group "
                                     f"{g}")
                if cp.bundle is not None:
                    raise ValueError(f"class {c}: hypernode classes never "
                                     "bundle")
                if cp.spread is not None or cp.affinity is not None:
                    raise ValueError(f"class {c}: one domain rule per class")
            if cp.device is not None and (cp.bundle is not None or
                                          self.device_state is None):
                raise ValueError(f"class {c}: a device class needs device "
                                 "state and never bundles")
            if cp.numa is not None and (cp.bundle is not None or
                                        self.numa_state is None):
                raise ValueError(f"class {c}: a numa class needs numa "
                                 "state and never bundles")
            if cp.rescore and cp.bundle is not None:
                raise ValueError(f"class {c}: re-scoring classes never "
                                 "bundle")
            for rule in (cp.spread, cp.affinity):
                if rule is not None and self.spread_groups[rule[0]].row >= 0:
                    raise ValueError(f"class {c}: group {rule[0]} is a "
                                     "hypernode group")
        self.log_total = off
        # a spread class re-scores inside a select of its own and has its own
        # column: class_rescore stays 0 for it
        self.class_rescore = np.array(
            [1 if cp.rescore and cp.spread is None else 0
             for cp in self.classes], dtype=np.int32)
        self.class_spread_rescore = np.array(
            [1 if cp.rescore and cp.spread is not None else 0
             for cp in self.classes], dtype=np.int32)
        # one weight per rule of the spread classes; a row with a nonzero
        # weight takes spread_soft_select
        self.class_spread_soft = np.zeros(
            (len(self.classes), ref.SPREAD_MAX_RULES), dtype=np.float32)
        for c, cp in enumerate(self.classes):
            if cp.spread_soft is not None:
                self.class_spread_soft[c, :len(cp.spread_soft)] = \
                    cp.spread_soft
        lens = np.fromiter((jp.class_end - jp.class_begin
                            for jp in self.jobs), dtype=np.int64,
                           count=len(self.jobs))
        self.class_job = np.repeat(
            np.arange(len(self.jobs), dtype=np.int32), lens)

    @property
    def n_classes(self) -> int:
        return len(self.classes)


def run_plan_torch(plan: CyclePlan) -> CycleResult:
    """Interpret the plan over the torch oracle ops — mirrors
    ``cycle_runner.hip`` statement for statement (CPU test tier)."""
    nt = plan.nt
    N, R = nt.n, nt.r
    dev = nt.alloc_t.device
    C = plan.n_classes
    if C == 0:
        return CycleResult([], {}, {})

    alloc = nt.alloc_t.t()          # [N, R] views over the [R, N] planes
    used = nt.used_t.t()
    extra_full = nt.extra_t.t()
    zeros_extra = torch.zeros_like(extra_full)
    planes = nt.planes_t.t()        # [N, W]

    dim_w = plan.dim_w.to(dev)
    score = torch.empty(N, dtype=torch.float32, device=dev)
    cap = torch.empty(N, dtype=torch.int32, device=dev)
    log_nodes = torch.zeros(plan.log_total, dtype=torch.int32, device=dev)
    log_counts = torch.zeros(plan.log_total, dtype=torch.int32, device=dev)
    log_len = torch.zeros(C, dtype=torch.int32, device=dev)
    class_placed = torch.zeros(C, dtype=torch.int32, device=dev)
    job_placed = torch.zeros(len(plan.jobs), dtype=torch.int32, device=dev)
    job_flag = torch.ones(len(plan.jobs), dtype=torch.uint8, device=dev)
    class_min = torch.tensor([cp.min_needed for cp in plan.classes],
                             dtype=torch.int32, device=dev)
    sp_dom = [torch.from_numpy(g.dom_of).to(dev) for g in plan.spread_groups]
    sp_cnt = [torch.from_numpy(g.count.copy()).to(dev)
              for g in plan.spread_groups]
    plan.spread_counts = sp_cnt
    # card planes and assignment rows live on the host here: the device
    # oracles are the per-pod GPUDevicePool loop
    cards = dev_assign = None
    if any(cp.device is not None for cp in plan.classes):
        ds = plan.device_state
        cards = [torch.from_numpy(a.copy()) for a in
                 (ds.mem_used, ds.cores_used, ds.state, ds.mem_total)]
        dev_assign = torch.zeros((plan.log_total, cards[0].shape[0]),
                                 dtype=torch.int32)
        plan.device_planes = dict(zip(
            ("mem_used", "cores_used", "state", "mem_total"), cards))
    # so do the zone plane and its rows: the oracle is the per-pod
    # best_zone loop
    zones = numa_assign = None
    if any(cp.numa is not None for cp in plan.classes):
        zones = torch.from_numpy(plan.numa_state.copy())
        numa_assign = torch.zeros((plan.log_total, zones.shape[0]),
                                  dtype=torch.int32)
        plan.numa_plane = zones

    def revert(c, cp, flag, req, sl):
        if cp.numa is not None:
            ref.numa_revert(flag, log_nodes[sl], log_len[c], zones,
                            numa_assign[sl], cp.numa[0])
        if cp.device is not None:
            ref.device_revert(flag, log_nodes[sl], log_len[c], *cards,
                              dev_assign[sl], cp.device)
        if cp.spread_rules is not None and len(cp.spread_rules) >= 2:
            ref.spread_multi_revert(
                flag, log_nodes[sl], log_counts[sl], log_len[c], req, used,
                plan.queue_alloc[cp.queue_idx], class_placed[c],
                job_placed[j],
                [(sp_dom[g], sp_cnt[g], k) for g, k in cp.spread_rules])
        elif cp.spread is not None or cp.affinity is not None:
            g = (cp.spread or cp.affinity)[0]
            ref.spread_revert(flag, log_nodes[sl], log_counts[sl],
                              log_len[c], req, used,
                              plan.queue_alloc[cp.queue_idx],
                              class_placed[c], job_placed[j],
                              sp_dom[g], sp_cnt[g])
        else:
            ref.cond_revert(flag, log_nodes[sl], log_counts[sl],
                            log_len[c], req, used,
                            plan.queue_alloc[cp.queue_idx],
                            class_placed[c], job_placed[j])

    for j, jp in enumerate(plan.jobs):
        nc = jp.class_end - jp.class_begin
        single = nc == 1
        for c in range(jp.class_begin, jp.class_end):
            cp = plan.classes[c]
            req = torch.from_numpy(cp.req).to(dev)
            require = torch.from_numpy(cp.require).to(dev)
            forbid = torch.from_numpy(cp.forbid).to(dev)
            extra = extra_full if cp.use_future else zeros_extra
            b = plan.bias if cp.bias is None \
                else torch.from_numpy(cp.bias).to(dev)
            ref.score_cap(alloc, used, extra, nt.ready.bool(), nt.taint_mask,
                          planes, req, cp.tolerated, require, forbid,
                          cp.w_least, cp.w_most, cp.w_bal, dim_w, b,
                          score, cap)
            if cp.device is not None:
                ref.device_cap(score, cap, *cards, cp.device)
            if cp.numa is not None and cp.numa[1] == ref.NUMA_HARD:
                ref.numa_cap(score, cap, zones, cp.numa[0])
            sl = slice(cp.log_off, cp.log_off + cp.log_cap)
            def select():
                # the static fill, or the per-placement re-score behind the
                # same score, cap and mask
                if not plan.class_rescore[c]:
                    return ref.select_commit(
                        score, cap, req, cp.ntasks, used,
                        plan.queue_alloc[cp.queue_idx],
                        plan.queue_limit[cp.queue_idx],
                        log_nodes[sl], log_counts[sl], log_len[c],
                        class_placed[c], job_placed[j])
                return ref.rescore_select_commit(
                    alloc, used, extra, nt.ready.bool(), nt.taint_mask,
                    planes, req, cp.tolerated, require, forbid, cp.w_least,
                    cp.w_most, cp.w_bal, dim_w, b, score, cap, cp.ntasks,
                    plan.queue_alloc[cp.queue_idx],
                    plan.queue_limit[cp.queue_idx],
                    log_nodes[sl], log_counts[sl], log_len[c],
                    class_placed[c], job_placed[j])

            if single:
                # a discarded single-class gang leaves no trace (the HIP
                # selects commit from the log only when the gang holds):
                # u + c*r - c*r is not u in f32 once usage comes in bytes
                used_before = used.clone()
                qa_before = plan.queue_alloc[cp.queue_idx].clone()
            if plan.class_spread_soft[c].any():
                rules = cp.spread_rules or [cp.spread]
                ref.spread_soft_select_commit(
                    alloc, used, extra, nt.ready.bool(), nt.taint_mask,
                    planes, req, cp.tolerated, require, forbid, cp.w_least,
                    cp.w_most, cp.w_bal, dim_w, b, score, cap, cp.ntasks,
                    plan.queue_alloc[cp.queue_idx],
                    plan.queue_limit[cp.queue_idx],
                    log_nodes[sl], log_counts[sl], log_len[c],
                    class_placed[c], job_placed[j],
                    [(sp_dom[g], sp_cnt[g], k, tw) for (g, k), tw in
                     zip(rules, plan.class_spread_soft[c])],
                    bool(plan.class_spread_rescore[c]))
            elif plan.class_spread_rescore[c]:
                ref.spread_rescore_select_commit(
                    alloc, used, extra, nt.ready.bool(), nt.taint_mask,
                    planes, req, cp.tolerated, require, forbid, cp.w_least,
                    cp.w_most, cp.w_bal, dim_w, b, score, cap, cp.ntasks,
                    plan.queue_alloc[cp.queue_idx],
                    plan.queue_limit[cp.queue_idx],
                    log_nodes[sl], log_counts[sl], log_len[c],
                    class_placed[c], job_placed[j],
                    [(sp_dom[g], sp_cnt[g], k)
                     for g, k in cp.spread_rules or [cp.spread]])
            elif cp.spread_rules is not None and len(cp.spread_rules) >= 2:
                ref.spread_multi_select_commit(
                    score, cap, req, cp.ntasks, used,
                    plan.queue_alloc[cp.queue_idx],
                    plan.queue_limit[cp.queue_idx],
                    log_nodes[sl], log_counts[sl], log_len[c],
                    class_placed[c], job_placed[j],
                    [(sp_dom[g], sp_cnt[g], k) for g, k in cp.spread_rules])
            elif cp.spread is not None:
                g, skew = cp.spread
                ref.spread_select_commit(
                    score, cap, req, cp.ntasks, used,
                    plan.queue_alloc[cp.queue_idx],
                    plan.queue_limit[cp.queue_idx],
                    log_nodes[sl], log_counts[sl], log_len[c],
                    class_placed[c], job_placed[j],
                    sp_dom[g], sp_cnt[g], skew)
            elif cp.hypernode is not None:
                g = cp.hypernode
                ref.hypernode_mask(score, cap, sp_dom[g], sp_cnt[g],
                                   plan.spread_groups[g].leaves)
                select()
            elif cp.affinity is not None and plan.class_rescore[c]:
                # the device's own composition: mask, select, count update
                g, mode = cp.affinity
                ref.domain_mask(score, cap, sp_dom[g], sp_cnt[g], mode)
                select()
                n = int(log_len[c])
                sp_cnt[g].index_add_(
                    0, sp_dom[g][log_nodes[sl][:n].long()].long(),
                    log_counts[sl][:n])
            elif cp.affinity is not None:
                g, mode = cp.affinity
                ref.affinity_select_commit(
                    score, cap, req, cp.ntasks, used,
                    plan.queue_alloc[cp.queue_idx],
                    plan.queue_limit[cp.queue_idx],
                    log_nodes[sl], log_counts[sl], log_len[c],
                    class_placed[c], job_placed[j],
                    sp_dom[g], sp_cnt[g], mode)
            else:
                select()
            if single:
                need = max(jp.min_available - jp.occupied, cp.min_needed, 0)
                flag = (class_placed[c] >= need).to(torch.uint8)
                job_flag[j] = flag
                if int(flag) == 0:
                    revert(c, cp, flag, req, sl)
                    idx = log_nodes[sl][:int(log_len[c])].long()
                    used[idx] = used_before[idx]
                    plan.queue_alloc[cp.queue_idx].copy_(qa_before)
            # the (zeroed) log of a discarded single-class gang takes nothing
            if cp.device is not None:
                ref.device_commit(log_nodes[sl], log_counts[sl], log_len[c],
                                  *cards, dev_assign[sl], cp.device)
            if cp.numa is not None:
                ref.numa_commit(log_nodes[sl], log_counts[sl], log_len[c],
                                zones, numa_assign[sl], cp.numa[0])
        if not single:
            ref.finalize_job(job_placed[j], jp.occupied, jp.min_available,
                             class_placed[jp.class_begin:jp.class_end],
                             class_min[jp.class_begin:jp.class_end],
                             job_flag[j])
            for c in range(jp.class_begin, jp.class_end):
                cp = plan.classes[c]
                req = torch.from_numpy(cp.req).to(dev)
                sl = slice(cp.log_off, cp.log_off + cp.log_cap)
                revert(c, cp, job_flag[j], req, sl)

    return CycleResult(plan, log_nodes.cpu().numpy(),
                      log_counts.cpu().numpy(), log_len.cpu().numpy(),
                      class_placed.cpu().numpy(), job_placed.cpu().numpy(),
                      job_flag.cpu().numpy(),
                      None if dev_assign is None else dev_assign.numpy(),
                      None if numa_assign is None else numa_assign.numpy())


def run_plan_hip(plan: CyclePlan) -> CycleResult:
    """One library call → whole cycle on the GPU (no host syncs mid-cycle)."""
    from ..ops import hip

    nt = plan.nt
    N, R = nt.n, nt.r
    W = nt.planes_t.shape[0]
    dev = nt.alloc_t.device
    C = plan.n_classes
    if C == 0:
        return CycleResult([], {}, {})
    if R > 64:
        # revert/commit kernels map one wavefront (64 lanes) per log
        # entry — more resource dims than lanes would silently skip dims
        raise RuntimeError(
            f"HIP decision plane supports up to 64 resource dims, got {R} "
            "(synthetic paa:/hp: dims count); split the inventory or use "
            "the torch oracle path")

    # ---- descriptor marshalling: ONE pass over the classes filling
    # numpy staging buffers (ctypes per-field struct stores measured
    # ~100 ms/cycle on 10k-class mixed plans — the numpy columns are
    # binary-compatible with VamdClassDesc/VamdJobDesc).
    J = len(plan.jobs)
    cds = np.empty(C, dtype=CLASS_DT)
    jds = np.empty(J, dtype=JOB_DT)
    for j, jp in enumerate(plan.jobs):
        jds[j] = (jp.class_begin, jp.class_end, jp.occupied,
                  jp.min_available)
    job_idx = plan.class_job

    req_np = plan.req_np
    require_np = np.empty((C, W), dtype=np.int64)
    forbid_np = np.empty((C, W), dtype=np.int64)
    tol_np = np.empty(C, dtype=np.int64)
    bias_rows_list: List[np.ndarray] = []
    bias_row_of: Dict[int, int] = {}      # id(array) -> row index
    for c, cp in enumerate(plan.classes):
        if cp.bias is None:
            brow = -1
        else:
            brow = bias_row_of.get(id(cp.bias))
            if brow is None:
                brow = bias_row_of[id(cp.bias)] = len(bias_rows_list)
                bias_rows_list.append(cp.bias)
        nt_override = cp.ntasks_override
        cds[c] = (job_idx[c], cp.queue_idx,
                  nt_override if nt_override is not None
                  else len(cp.tclass.tasks),
                  cp.min_needed, cp.log_off, cp.log_cap,
                  1 if cp.use_future else 0, brow,
                  cp.w_least, cp.w_most, cp.w_bal, 0.0)
        require_np[c] = cp.require
        forbid_np[c] = cp.forbid
        tol_np[c] = cp.tolerated

    class_req = torch.from_numpy(req_np).to(dev)                    # [C,R]
    # class_tol stays HOST-side: cycle_runner dereferences it per class on
    # the CPU and passes the value into the launch (vamd_api.h)
    class_tol = torch.from_numpy(tol_np)
    class_require = torch.from_numpy(require_np).to(dev)            # [C,W]
    class_forbid = torch.from_numpy(forbid_np).to(dev)
    class_min = torch.from_numpy(
        np.ascontiguousarray(cds["min_needed"], dtype=np.int32)).to(dev)
    dim_w = plan.dim_w.to(dev, torch.float32)
    q_alloc = plan.queue_alloc.to(dev).contiguous()
    q_limit = plan.queue_limit.to(dev).contiguous()
    bias = plan.bias.to(dev) if plan.bias is not None else None
    bias_rows = torch.from_numpy(
        np.stack(bias_rows_list).astype(np.float32)).to(dev).contiguous() \
        if bias_rows_list else None                                # [B,N]

    score = torch.empty(N, dtype=torch.float32, device=dev)
    cap = torch.empty(N, dtype=torch.int32, device=dev)
    log_nodes = torch.zeros(plan.log_total, dtype=torch.int32, device=dev)
    log_counts = torch.zeros(plan.log_total, dtype=torch.int32, device=dev)
    log_len = torch.zeros(C, dtype=torch.int32, device=dev)
    class_placed = torch.zeros(C, dtype=torch.int32, device=dev)
    job_placed = torch.zeros(len(plan.jobs), dtype=torch.int32, device=dev)
    job_flag = torch.ones(len(plan.jobs), dtype=torch.uint8, device=dev)
    # radix scratch for the bulk select path (keys/ids ping-pong)
    sort_scratch = torch.empty(4 * N, dtype=torch.int32, device=dev) \
        if C and int(cds["ntasks"].max()) >= 512 and N >= 512 else None

    # domain-rule classes (topology spread, inter-pod affinity): group
    # tables go to the device once, the per-class (group, maxSkew, mode)
    # columns stay host-side for the runner.  The mode column exists only
    # when the plan has affinity classes — otherwise the call is the one a
    # spread-only plan always made.
    spread = None
    any_hn = any(cp.hypernode is not None for cp in plan.classes)
    any_aff = any(cp.affinity is not None for cp in plan.classes)
    if any_hn or any_aff or \
            any(cp.spread is not None for cp in plan.classes):
        groups = plan.spread_groups
        cg = np.full(C, -1, dtype=np.int32)
        cs = np.ones(C, dtype=np.int32)
        cm = np.zeros(C, dtype=np.int32)
        for c, cp in enumerate(plan.classes):
            if cp.spread is not None:
                cg[c], cs[c] = cp.spread
            elif cp.affinity is not None:
                cg[c], cm[c] = cp.affinity
            elif cp.hypernode is not None:
                cg[c], cm[c] = cp.hypernode, ref.HYPERNODE
        # a hypernode group's slice of `count` is its table and its D the
        # leaf count of its row
        lens = np.array([g.count.shape[0] for g in groups], dtype=np.int32)
        doms = np.array([g.leaves if g.row >= 0 else g.count.shape[0]
                         for g in groups], dtype=np.int32)
        offs = (np.cumsum(lens) - lens).astype(np.int32)
        count = torch.from_numpy(
            np.concatenate([g.count for g in groups]).astype(np.int32)
        ).to(dev)
        # dom_of rows: one per ordinary group, ONE per leaf map however
        # many hypernode groups read it (group_row names the row)
        rows: List[np.ndarray] = []
        row_of_leafmap: Dict[int, int] = {}
        grow = np.empty(len(groups), dtype=np.int32)
        for gi, g in enumerate(groups):
            if g.row >= 0:
                r = row_of_leafmap.get(g.row)
                if r is None:
                    r = row_of_leafmap[g.row] = len(rows)
                    rows.append(g.dom_of)
                grow[gi] = r
            else:
                grow[gi] = len(rows)
                rows.append(g.dom_of)
        spread = dict(
            class_group=cg, class_skew=cs,
            dom_of=torch.from_numpy(
                np.stack(rows).astype(np.int32)
            ).to(dev).contiguous(),
            count=count, count_off=offs, domains=doms,
            scratch=hip.spread_scratch(N, dev))
        if any_aff or any_hn:
            spread["class_mode"] = cm
        if row_of_leafmap:
            spread["group_row"] = grow
        # classes under several spread rules: n, then the (group, maxSkew)
        # pairs; the column exists only when the plan has such a class
        if any(cp.spread_rules is not None and len(cp.spread_rules) >= 2
               for cp in plan.classes):
            cr = np.zeros((C, 9), dtype=np.int32)
            for c, cp in enumerate(plan.classes):
                if cp.spread_rules is not None and len(cp.spread_rules) >= 2:
                    cr[c, 0] = len(cp.spread_rules)
                    cr[c, 1:1 + 2 * len(cp.spread_rules)] = \
                        np.asarray(cp.spread_rules, dtype=np.int32).ravel()
            spread["class_rules"] = cr
        # spread classes that re-score per placement: the flag column stays
        # host-side for the runner and exists only when the plan has one
        if plan.class_spread_rescore.any():
            spread["class_rescore"] = plan.class_spread_rescore
        # so do the weights of the classes with a soft rule
        if plan.class_spread_soft.any():
            spread["class_soft"] = plan.class_spread_soft
        plan.spread_counts = [count[int(o):int(o) + int(d)]
                              for o, d in zip(offs, lens)]

    # device-request classes: the card planes go up once, the per-class
    # request column stays host-side for the runner, and the assignment
    # rows (parallel to the log) come back with the log
    devices = None
    if any(cp.device is not None for cp in plan.classes):
        ds = plan.device_state
        creq = np.zeros((C, 4), dtype=np.int32)
        for c, cp in enumerate(plan.classes):
            if cp.device is not None:
                creq[c, :3] = cp.device
        devices = dict(
            mem_used=torch.from_numpy(ds.mem_used).to(dev),
            cores_used=torch.from_numpy(ds.cores_used).to(dev),
            state=torch.from_numpy(ds.state).to(dev),
            mem_total=torch.from_numpy(ds.mem_total).to(dev),
            class_req=creq,
            assign=torch.zeros((plan.log_total, ds.mem_used.shape[0]),
                               dtype=torch.int32, device=dev))
        plan.device_planes = {k: devices[k] for k in (
            "mem_used", "cores_used", "state", "mem_total")}

    # NUMA-request classes, the same way: one plane up, one request column
    # host-side, one set of rows back
    numa = None
    if any(cp.numa is not None for cp in plan.classes):
        nreq = np.zeros((C, 2), dtype=np.int32)
        for c, cp in enumerate(plan.classes):
            if cp.numa is not None:
                nreq[c] = cp.numa
        numa = dict(
            zone_free=torch.from_numpy(plan.numa_state).to(dev),
            class_req=nreq,
            assign=torch.zeros((plan.log_total, plan.numa_state.shape[0]),
                               dtype=torch.int32, device=dev))
        plan.numa_plane = numa["zone_free"]

    # re-scoring classes: the flag column stays host-side for the runner;
    # the block exists only when the plan has such a class
    rescore = None
    if plan.class_rescore.any():
        rescore = dict(
            class_rescore=plan.class_rescore,
            slot=torch.empty(max(N, 1), dtype=torch.int32, device=dev))

    hip.run_cycle(
        ctypes.c_void_p(cds.ctypes.data), C,
        ctypes.c_void_p(jds.ctypes.data), len(plan.jobs),
        nt.alloc_t, nt.used_t, nt.extra_t, nt.ready, nt.taint_mask,
        nt.planes_t, bias, bias_rows, class_req, class_tol, class_require,
        class_forbid, class_min, dim_w, q_alloc, q_limit, score, cap,
        log_nodes, log_counts, log_len, class_placed, job_placed, job_flag,
        sort_scratch, spread=spread, devices=devices, numa=numa,
        rescore=rescore)

    res = CycleResult(plan, log_nodes.cpu().numpy(),
                      log_counts.cpu().numpy(), log_len.cpu().numpy(),
                      class_placed.cpu().numpy(), job_placed.cpu().numpy(),
                      job_flag.cpu().numpy(),
                      None if devices is None
                      else devices["assign"].cpu().numpy(),
                      None if numa is None
                      else numa["assign"].cpu().numpy())
    # the cycle mutated device queue_alloc; reflect back to the host copy
    plan.queue_alloc.copy_(q_alloc.cpu())
    return res


