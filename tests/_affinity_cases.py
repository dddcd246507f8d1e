"""Inputs and an independent model for the inter-pod (anti-)affinity select.

``model`` is the per-instance definition of the rule in plain Python (no
torch, no shared code with ``reference.affinity_select_commit``).  Scores
are a few multiples of 0.25 (exact in f32, large tie groups), requests and
usage small integers, so every f32 operation is exact and "equal" means
bit-equal.  Kernel-level cases feed ``score``/``cap`` directly.  Plain
module: no fixtures, no collection hooks.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

import numpy as np
import torch

from volcano_amd.ops import reference as ref

NEG_INF = float("-inf")
BIG = 1.0e18
AFFINITY, ANTI = 1, 2


@dataclass
class AffinityCase:
    name: str
    score: np.ndarray        # [N] f32 (-inf = infeasible)
    cap: np.ndarray          # [N] i32
    req: np.ndarray          # [R] f32
    ntasks: int
    used: np.ndarray         # [N, R] f32
    queue_alloc: np.ndarray  # [R] f32
    queue_limit: np.ndarray  # [R] f32
    dom_of: np.ndarray       # [N] i32
    dom_count: np.ndarray    # [D] i32
    mode: int
    fuse_min: int = -1       # >= 0: single-class gang minimum (kernel side)

    @property
    def N(self):
        return len(self.score)

    @property
    def D(self):
        return len(self.dom_count)

    @property
    def K(self):
        return max(1, min(self.ntasks, self.N))


def quota_of(case) -> int:
    """Instances the queue still admits (integer inputs: exact)."""
    q = 2 ** 30
    for r in range(len(case.req)):
        if case.req[r] > 0:
            head = float(case.queue_limit[r]) - float(case.queue_alloc[r])
            q = min(q, max(0, int(np.floor(head / float(case.req[r])))))
    return q


def model(score, cap, dom_of, count, mode, budget):
    """Independent per-instance model -> (placement sequence, counts)."""
    count = list(count)
    left = {n: cap[n] for n in range(len(cap))
            if score[n] > NEG_INF and dom_of[n] >= 0 and cap[n] > 0}
    seq = []
    for _ in range(budget):
        if mode == AFFINITY:
            open_doms = {d for d, c in enumerate(count) if c > 0}
            if not open_doms:               # empty group: anyone anchors
                open_doms = set(range(len(count)))
        else:
            open_doms = {d for d, c in enumerate(count) if c == 0}
        ok = sorted(n for n in left if dom_of[n] in open_doms)
        if not ok:
            break
        top = max(score[n] for n in ok)
        n = next(n for n in ok if score[n] == top)
        left[n] -= 1
        if left[n] == 0:
            del left[n]
        count[dom_of[n]] += 1
        seq.append(n)
    return seq, count


def model_of(case: AffinityCase):
    return model(case.score.tolist(), case.cap.tolist(),
                 case.dom_of.tolist(), case.dom_count.tolist(), case.mode,
                 min(case.ntasks, quota_of(case)))


def log_of(seq: List[int]):
    """(nodes, counts): one entry per node in order of first placement."""
    nodes, counts = [], {}
    for n in seq:
        if n not in counts:
            nodes.append(n)
            counts[n] = 0
        counts[n] += 1
    return nodes, [counts[n] for n in nodes]


# --------------------------------------------------------------------------
# kernel-level cases
# --------------------------------------------------------------------------

def base_case(name, N, D, R, seed, mode, *, ntasks=None, count=None,
              unlabeled=0.1, infeasible=0.15, cap_hi=4, cap_lo=0,
              identity=False, quota=None, fuse_min=-1,
              scores=None) -> AffinityCase:
    """``scores``: a function ``(N, rng) -> float32[N]`` that replaces the
    four-valued draw (the infeasible share is still set to -inf here)."""
    rng = np.random.RandomState(seed)
    D = min(D, N)
    if identity:
        dom_of = np.arange(N, dtype=np.int32)
    else:
        # every domain owns at least one node when N allows it
        dom_of = np.concatenate([np.arange(D), rng.randint(0, D, size=N - D)])
        dom_of = dom_of[rng.permutation(N)].astype(np.int32)
        if N > 1:
            dom_of[rng.rand(N) < unlabeled] = -1
    score = (rng.randint(0, 4, size=N) * 0.25).astype(np.float32)
    if scores is not None:
        score = np.array(scores(N, rng), dtype=np.float32)
        assert score.shape == (N,)
    if N > 1:
        score[rng.rand(N) < infeasible] = NEG_INF
    cap = rng.randint(cap_lo, cap_hi + 1, size=N).astype(np.int32)
    if N == 1:
        cap[0] = max(int(cap[0]), 2)
    if count is None:
        count = np.zeros(D, dtype=np.int32)
    count = np.asarray(count, dtype=np.int32)
    assert count.shape == (D,)
    req = np.zeros(R, dtype=np.float32)
    req[0] = 1.0
    for r in range(1, min(R, 4)):
        req[r] = float(rng.randint(0, 3))
    used = rng.randint(0, 8, size=(N, R)).astype(np.float32)
    qa = rng.randint(0, 5, size=R).astype(np.float32)
    ql = np.full(R, BIG, dtype=np.float32)
    if ntasks is None:
        ntasks = 12
    if quota is not None:
        ql[0] = qa[0] + float(quota)
    return AffinityCase(name, score, cap, req, int(ntasks), used, qa, ql,
                        dom_of, count, mode, fuse_min)


def _labelled(case, d=None):
    m = case.dom_of >= 0 if d is None else case.dom_of == d
    return np.flatnonzero(m)


def a_anchor_best():
    c = base_case("anchor-best", 63, 3, 4, 1, AFFINITY, ntasks=9)
    n = int(_labelled(c, 2)[-1])
    c.score[n] = 1.0
    c.cap[n] = 2
    return c


def a_anchor_tie():
    """Top score on two nodes of different domains: the lower index
    anchors."""
    c = base_case("anchor-tie", 65, 3, 1, 2, AFFINITY, ntasks=9)
    lo, hi = int(_labelled(c, 2)[0]), int(_labelled(c, 0)[-1])
    assert lo < hi
    c.score[[lo, hi]] = 1.0
    c.cap[[lo, hi]] = 1
    return c


def a_zero_tie():
    """-0.0 at the lower index ties with +0.0: the lower index anchors."""
    c = base_case("zero-tie", 65, 3, 4, 3, AFFINITY, ntasks=6)
    c.score[c.score > NEG_INF] -= 1.0          # all others below zero
    lo, hi = int(_labelled(c, 1)[0]), int(_labelled(c, 0)[-1])
    assert lo < hi
    c.score[lo], c.score[hi] = -0.0, 0.0
    c.cap[[lo, hi]] = 1
    return c


def a_best_unlabelled():
    c = base_case("best-unlabelled", 65, 3, 1, 4, AFFINITY, ntasks=7)
    n = int(np.flatnonzero(c.dom_of < 0)[0])
    c.score[n] = 2.0
    c.cap[n] = 50
    return c


def a_two_of_three():
    return base_case("two-of-three", 65, 3, 4, 5, AFFINITY, ntasks=30,
                     count=[2, 0, 1])


def a_dead_domains():
    """Members only where nothing is feasible: no second anchor."""
    c = base_case("dead-domains", 65, 3, 1, 6, AFFINITY, ntasks=5,
                  count=[0, 3, 0])
    c.score[c.dom_of == 1] = NEG_INF
    return c


def a_budget_zero():
    return base_case("budget-zero", 63, 3, 4, 7, AFFINITY, ntasks=5,
                     quota=0)


def a_identity_cap3():
    c = base_case("identity-cap3", 1025, 1025, 1, 8, AFFINITY, ntasks=5,
                  identity=True)
    c.score[700] = 1.0
    c.cap[700] = 3
    return c


def a_fuse_min_revert():
    c = base_case("fuse-min-revert", 65, 3, 4, 9, AFFINITY, ntasks=400,
                  fuse_min=400)
    return c


def a_single_node():
    return base_case("single-node", 1, 1, 1, 10, AFFINITY, ntasks=3)


def a_bulk_empty():
    return base_case("bulk-empty", 1500, 7, 4, 11, AFFINITY, ntasks=600)


def a_bulk_hosting():
    return base_case("bulk-hosting", 1500, 7, 1, 12, AFFINITY, ntasks=600,
                     count=[0, 2, 0, 0, 1, 0, 0])


AFFINITY_CASES: Dict[str, Callable[[], AffinityCase]] = {
    f.__name__[2:].replace("_", "-"): f for f in (
        a_anchor_best, a_anchor_tie, a_zero_tie, a_best_unlabelled,
        a_two_of_three, a_dead_domains, a_budget_zero, a_identity_cap3,
        a_fuse_min_revert, a_single_node, a_bulk_empty, a_bulk_hosting)}


def b_one_per_open():
    return base_case("one-per-open", 63, 3, 4, 21, ANTI, ntasks=3)


def b_occupied_closed():
    return base_case("occupied-closed", 65, 3, 1, 22, ANTI, ntasks=3,
                     count=[1, 0, 0])


def b_head_tie():
    """A domain's top score on two of its nodes: the lower index is its
    head."""
    c = base_case("head-tie", 65, 3, 4, 23, ANTI, ntasks=3)
    ids = _labelled(c, 1)
    c.score[[ids[1], ids[-1]]] = 1.0
    c.cap[[ids[1], ids[-1]]] = 2
    return c


def b_zero_tie():
    c = base_case("zero-tie", 65, 3, 1, 24, ANTI, ntasks=3)
    c.score[c.score > NEG_INF] -= 1.0
    ids = _labelled(c, 2)
    c.score[ids[0]], c.score[ids[-1]] = -0.0, 0.0
    c.cap[[ids[0], ids[-1]]] = 1
    return c


def b_more_than_open():
    return base_case("more-than-open", 65, 3, 4, 25, ANTI, ntasks=40)


def b_caps_clipped():
    return base_case("caps-clipped", 63, 3, 1, 26, ANTI, ntasks=20,
                     cap_lo=2, cap_hi=5)


def b_identity():
    return base_case("identity", 1025, 1025, 4, 27, ANTI, ntasks=300,
                     identity=True)


def b_budget_clamp():
    return base_case("budget-clamp", 65, 3, 4, 28, ANTI, ntasks=3, quota=2)


def b_fuse_min_revert():
    return base_case("fuse-min-revert", 65, 3, 1, 29, ANTI, ntasks=8,
                     fuse_min=4)


def b_single_node():
    return base_case("single-node", 1, 1, 4, 30, ANTI, ntasks=3)


def b_bulk():
    return base_case("bulk", 1500, 7, 4, 31, ANTI, ntasks=600,
                     count=[0, 0, 4, 0, 0, 1, 0])


def b_bulk_identity():
    c = base_case("bulk-identity", 1500, 1500, 1, 32, ANTI, ntasks=600,
                  identity=True)
    c.dom_count[::3] = 1
    return c


ANTI_CASES: Dict[str, Callable[[], AffinityCase]] = {
    f.__name__[2:].replace("_", "-"): f for f in (
        b_one_per_open, b_occupied_closed, b_head_tie, b_zero_tie,
        b_more_than_open, b_caps_clipped, b_identity, b_budget_clamp,
        b_fuse_min_revert, b_single_node, b_bulk, b_bulk_identity)}


# --------------------------------------------------------------------------
# oracle runners
# --------------------------------------------------------------------------

def _buffers(case):
    t = torch.from_numpy
    return dict(
        used=t(case.used.copy()), qa=t(case.queue_alloc.copy()),
        req=t(case.req.copy()),
        ln=torch.zeros(case.K, dtype=torch.int32),
        lc=torch.zeros(case.K, dtype=torch.int32),
        ll=torch.zeros((), dtype=torch.int32),
        placed=torch.zeros((), dtype=torch.int32),
        jp=torch.full((), 7, dtype=torch.int32))


def run_oracle(case: AffinityCase, *, revert: Optional[bool] = None):
    """reference.affinity_select_commit on fresh copies.  ``revert``: apply
    spread_revert afterwards (None: decide from case.fuse_min, as the
    select kernels do in place)."""
    t = torch.from_numpy
    b = _buffers(case)
    cnt = t(case.dom_count.copy())
    dom = t(case.dom_of.copy())
    ref.affinity_select_commit(
        t(case.score.copy()), t(case.cap.copy()), b["req"], case.ntasks,
        b["used"], b["qa"], t(case.queue_limit.copy()), b["ln"], b["lc"],
        b["ll"], b["placed"], b["jp"], dom, cnt, case.mode)
    before = dict(log_nodes=b["ln"].numpy().copy(),
                  log_counts=b["lc"].numpy().copy(),
                  placed=int(b["placed"]), dom_count=cnt.numpy().copy())
    if revert is None:
        revert = case.fuse_min >= 0 and int(b["placed"]) < case.fuse_min
    if revert:
        ref.spread_revert(torch.zeros((), dtype=torch.uint8), b["ln"],
                          b["lc"], b["ll"], b["req"], b["used"], b["qa"],
                          b["placed"], b["jp"], dom, cnt)
    return dict(log_nodes=b["ln"].numpy(), log_counts=b["lc"].numpy(),
                log_len=int(b["ll"]), placed=int(b["placed"]),
                job_placed=int(b["jp"]), used=b["used"].numpy(),
                queue_alloc=b["qa"].numpy(), dom_count=cnt.numpy(),
                reverted=bool(revert), before=before)


def run_unconstrained(case: AffinityCase, *, clip=False):
    """reference.select_commit on the same inputs, no domain rule
    (``clip``: caps clipped to 1) -> (log nodes, log counts, placed)."""
    t = torch.from_numpy
    b = _buffers(case)
    cap = np.minimum(case.cap, 1) if clip else case.cap
    ref.select_commit(t(case.score.copy()), t(cap.copy()), b["req"],
                      case.ntasks, b["used"], b["qa"],
                      t(case.queue_limit.copy()), b["ln"], b["lc"], b["ll"],
                      b["placed"], b["jp"])
    n = int(b["ll"])
    return (b["ln"].numpy()[:n].tolist(), b["lc"].numpy()[:n].tolist(),
            int(b["placed"]))


# --------------------------------------------------------------------------
# plan-level case: affinity, anti-affinity, spread and plain classes
# --------------------------------------------------------------------------

@dataclass
class AffinityPlanCase:
    base: object                   # _kernel_cases.PlanCase
    spread: dict                   # class index -> (group, max_skew)
    affinity: dict                 # class index -> (group, mode)
    groups: list                   # [(dom_of i32 [N], count i32 [D])]
    roles: dict                    # name -> class index


def affinity_plan_case(N=1500, R=5, W=1, seed=33, inexact=False,
                       bias_shift=0.0) -> AffinityPlanCase:
    """``inexact``: the inexact node state and bias rows, ``w_bal`` 1 for
    every class; ``bias_shift`` is added to the plan-wide bias.

    Group 0: zones (3 domains, empty at the start), shared by affinity
    classes.  Group 1: zones of a spread rule.  Group 2: racks of an anti
    rule (7 domains, two occupied).  Group 3: per-node affinity (identity).

    Job order: an affinity job of group 0 that anchors, then misses its
    gang minimum in the select and reverts · an affinity job of group 0
    (anchors again, from restored counts) · 34 small plain jobs (a chain
    run) · a two-role gang, role 1 affinity of group 0, role 2 missing its
    minimum (multi-class revert) · an affinity job of group 0 (follows the
    anchor, sees the gang's counts given back) · an anti job of group 2 · a spread job of
    group 1 · a second anti job of group 2 (sees the closed domains) · a
    bulk-sized affinity job of group 0 (N >= 512 only) · a per-node
    affinity job of group 3 · 6 plain jobs."""
    import _kernel_cases as kc
    rng = np.random.RandomState(seed)
    st = kc.dyadic_state(N, R, W, seed, inexact=inexact)
    if bias_shift:
        st["bias"] = st["bias"] + np.float32(bias_shift)
    classes, jobs, spread, affinity, roles = [], [], {}, {}, {}

    def add_job(cls, occupied, min_avail):
        b = len(classes)
        classes.extend(cls)
        jobs.append((b, len(classes), occupied, min_avail))

    def small_jobs(count):
        for j in range(count):
            n = int(rng.randint(1, 13))
            need = n + 1 if j % 11 == 3 else max(1, n - 1)
            add_job([kc._class(rng, R, W, n, 2 if j % 5 == 4 else j % 2,
                               bias_row=j % 2 if j % 3 == 0 else None,
                               plain=True)], 0, need)

    def mark(name, table, value):
        roles[name] = len(classes)
        table[len(classes)] = value

    mark("aff_revert", affinity, (0, AFFINITY))
    add_job([kc._class(rng, R, W, 6, 0, plain=True)], 0, 100 * N)
    mark("aff_anchor", affinity, (0, AFFINITY))
    add_job([kc._class(rng, R, W, 9, 0, plain=True)], 0, 2)
    small_jobs(34)
    mark("gang_aff", affinity, (0, AFFINITY))
    add_job([kc._class(rng, R, W, 7, 0, min_needed=1, plain=True),
             kc._class(rng, R, W, 3, 1, min_needed=4, plain=True)], 0, 5)
    mark("aff_follow", affinity, (0, AFFINITY))
    add_job([kc._class(rng, R, W, 4, 1, plain=True)], 0, 1)
    mark("anti", affinity, (2, ANTI))
    add_job([kc._class(rng, R, W, 3, 1, plain=True)], 0, 1)
    mark("spread", spread, (1, 1))
    add_job([kc._class(rng, R, W, 10, 0, plain=True)], 0, 2)
    mark("anti_later", affinity, (2, ANTI))
    add_job([kc._class(rng, R, W, 20, 0, plain=True)], 0, 1)
    if N >= 512:
        mark("aff_bulk", affinity, (0, AFFINITY))
        add_job([kc._class(rng, R, W, 600, 1, plain=True)], 0, 10)
    mark("host", affinity, (3, AFFINITY))
    add_job([kc._class(rng, R, W, 5, 0, plain=True)], 0, 1)
    small_jobs(6)

    dom0 = rng.randint(0, 3, size=N).astype(np.int32)
    dom0[rng.rand(N) < 0.1] = -1
    dom2 = rng.randint(0, 7, size=N).astype(np.int32)
    dom2[rng.rand(N) < 0.05] = -1
    groups = [(dom0, np.zeros(3, dtype=np.int32)),
              (dom0.copy(), np.array([1, 0, 0], dtype=np.int32)),
              (dom2, np.array([0, 2, 0, 0, 1, 0, 0], dtype=np.int32)),
              (np.arange(N, dtype=np.int32), np.zeros(N, dtype=np.int32))]
    ql, qa = kc._queues(rng, R, limit_dim0=30)
    base = kc.PlanCase("affinity", N, R, W, st, classes, jobs, ql, qa,
                       kc._bias_rows(rng, N, 2, inexact=inexact),
                       w_bal=1.0 if inexact else 0.0)
    return AffinityPlanCase(base, spread, affinity, groups, roles)


def build_affinity_plan(case: AffinityPlanCase, device, *, rules=True,
                        w_bal: float = 0.0):
    """``rules=False``: the same classes with no domain rule at all."""
    import _kernel_cases as kc
    plan = kc.build_plan(case.base, device, w_bal)
    if not rules:
        return plan
    for dom_of, count in case.groups:
        plan.add_spread_group(dom_of.copy(), count.copy())
    for c, sp in case.spread.items():
        plan.classes[c].spread = sp
    for c, af in case.affinity.items():
        plan.classes[c].affinity = af
    return plan


def plan_snapshot(plan, res) -> dict:
    import _kernel_cases as kc
    snap = kc.snapshot(plan, res)
    snap["spread_counts"] = [t.cpu().numpy().copy()
                             for t in (plan.spread_counts or [])]
    return snap


def compare_plans(want: dict, got: dict) -> None:
    import _kernel_cases as kc
    kc.compare_results(want, got)
    assert len(want["spread_counts"]) == len(got["spread_counts"])
    for g, (a, b) in enumerate(zip(want["spread_counts"],
                                   got["spread_counts"])):
        assert np.array_equal(a, b), f"group {g}: final dom_count differs"


def run_plan_oracle(case: AffinityPlanCase, *, rules=True):
    """run_plan_torch on the CPU -> (snapshot, records of every oracle
    affinity select: group, mode, counts before, placed)."""
    from volcano_amd.scheduler import plan as planmod
    plan = build_affinity_plan(case, "cpu", rules=rules)
    records = []
    real = ref.affinity_select_commit

    def spy(score, cap, req, ntasks, used, qa, ql, ln, lc, ll, placed, jp,
            dom_of, dom_count, mode):
        rec = dict(count=dom_count.tolist(), mode=mode, ntasks=int(ntasks))
        real(score, cap, req, ntasks, used, qa, ql, ln, lc, ll, placed, jp,
             dom_of, dom_count, mode)
        rec["placed"] = int(placed)
        rec["after"] = dom_count.tolist()
        records.append(rec)

    planmod.ref.affinity_select_commit = spy
    try:
        res = planmod.run_plan_torch(plan)
    finally:
        planmod.ref.affinity_select_commit = real
    return plan_snapshot(plan, res), records
