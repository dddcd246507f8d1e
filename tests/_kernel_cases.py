"""Shared inputs for the kernel edge tests and the plan-path harness.

Oracle (``volcano_amd/ops/reference.py``) and kernels are both f32, but the
device compiler contracts ``a*b+c`` into FMA, so on arbitrary floats the two
scores differ in the last bits and a near-tie may order differently without
any bug.  ``dyadic_state`` generates inputs on which EVERY f32 operation of
the score is exact (with or without FMA, in any summation order):

* ``alloc`` is a power of two, ``used``/``req``/``extra`` are small
  integers -> ``(used + req) / alloc`` is a multiple of 2^-6 in [0, 1];
* ``dim_w`` is in {1, 2} with a power-of-two sum -> the weighted sums have
  a handful of mantissa bits and the division by the sum is a shift;
* ``w_least``/``w_most`` are in {0, 0.5, 1, 2}, ``w_bal`` is 0;
* the bias is a multiple of 2^-6.

Scores are then bit-identical on both sides, and because nodes are drawn
from a few node *types* (as real inventories are) large tie groups appear
naturally.  This is a plain module (no fixtures, no collection hooks).

Production runs where every one of those operations rounds, so the same
generators have an ``inexact=True`` mode (``inexact_plan_cases``): ``alloc``
is the dyadic value minus 1 or 3, ``dim_w`` is in {1, 2, 3} with a sum that
is no power of two, every bias is scaled by 0.3 and ``w_bal`` is 1.  Node
types, ``used``/``req``/``extra`` (small integers) and the feasibility
inputs stay, so twin groups survive and usage arithmetic stays exact.  No
bit-equality with the f32 oracle is claimed there; instead
``validate_plan`` replays any runner's snapshot in float64 and accepts an
order only within ``KERNEL_ERR`` (measured below against the float64
formula, never against a kernel), and the GPU paths are compared with each
other bit for bit.  ``byte_plan_cases`` put decimal byte-scale memory
(``1500M``) into one dim, where ``u + c*r - c*r`` is not ``u`` in f32.
"""

from __future__ import annotations

import contextlib
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np
import torch

from volcano_amd.ops import reference as ref
from volcano_amd.scheduler import plan as planmod
from volcano_amd.scheduler.plan import ClassPlan, CyclePlan, JobPlan

EPS = ref.EPS
BIG_CAP = ref.BIG_CAP
NEG_INF = float("-inf")
BIT62 = np.int64(1) << np.int64(62)
BIT63 = np.int64(np.iinfo(np.int64).min)          # bit 63 as a signed word
TOPK = 16            # CH_TOPK of the chain path
CHAIN_THREADS = 256  # CH_THREADS: touched lists longer than this loop twice


def dim_weights(R: int, rng: np.random.RandomState) -> np.ndarray:
    """{1, 2}-valued weights whose sum is the next power of two >= R."""
    P = 1
    while P < R:
        P *= 2
    w = np.ones(R, dtype=np.float32)
    w[rng.permutation(R)[:P - R]] = 2.0
    assert float(w.sum()) == float(P)
    return w


def inexact_dim_weights(R: int, rng: np.random.RandomState) -> np.ndarray:
    """{1, 2, 3}-valued weights whose sum is no power of two."""
    w = rng.randint(1, 4, size=R).astype(np.float32)
    while float(w.sum()) in {float(2 ** k) for k in range(12)}:
        w[0] = w[0] % 3 + 1
    return w


INEXACT_BIAS = np.float32(0.3)


def dyadic_state(N: int, R: int, W: int, seed: int, *, n_types: int = 12,
                 cap_one: bool = False, not_ready: float = 0.05,
                 hot: int = 0, inexact: bool = False
                 ) -> Dict[str, torch.Tensor]:
    """Node state + one request on which the f32 score is exact.

    ``inexact`` keeps every draw of the exact state and then takes 1 or 3
    off each node type's ``alloc`` per dim, draws ``dim_w`` from {1, 2, 3}
    and scales the bias by 0.3: every fraction, weighted sum and bias add
    of the score rounds, node types and integer usage stay.

    ``cap_one`` leaves exactly one unit of dim 0 free on every node (the
    requests of the plan builder always ask one unit of dim 0), ``hot``
    makes the first ``hot`` nodes small and feasible for every plain class,
    so a bias can make all classes prefer them and use them up."""
    rng = np.random.RandomState(seed)
    T = max(1, min(n_types, N))
    t_alloc = rng.choice([16.0, 32.0, 64.0], size=(T, R)).astype(np.float32)
    t_used = np.floor(t_alloc * rng.choice([0.0, 0.25, 0.5, 0.75],
                                           size=(T, R))).astype(np.float32)
    t_extra = rng.randint(0, 3, size=(T, R)).astype(np.float32)
    kind = rng.randint(0, T, size=N)
    rng_x = np.random.RandomState(seed + 7919)     # inexact-only draws
    if inexact:
        t_alloc = t_alloc - rng_x.choice([1.0, 3.0], size=(T, R)).astype(
            np.float32)
    alloc = t_alloc[kind]
    used = t_used[kind].copy()
    extra = t_extra[kind]
    # a few nodes carry individual integer usage so not everything ties
    odd = rng.rand(N) < 0.2
    used[odd] = np.minimum(used[odd] + rng.randint(0, 4, size=(int(odd.sum()), R)),
                           alloc[odd]).astype(np.float32)
    if cap_one:
        alloc[:, 0] = 16.0
        used[:, 0] = 15.0
        extra = extra.copy()
        extra[:, 0] = 0.0
    ready = rng.rand(N) >= not_ready
    taint_bits = np.array([1, 2, BIT62, BIT63], dtype=np.int64)
    taints = np.zeros(N, dtype=np.int64)
    for b in taint_bits:
        taints |= np.where(rng.rand(N) < 0.08, b, np.int64(0))
    plane_bits = np.array([1, 4, 8, BIT62, BIT63], dtype=np.int64)
    planes = np.zeros((N, W), dtype=np.int64)
    for b in plane_bits:
        planes |= np.where(rng.rand(N, W) < 0.5, b, np.int64(0))
    if hot:
        # room for one or two tasks each, feasible for every plain class
        ready[:hot] = True
        taints[:hot] = 0
        used[:hot, 1:4] = 0.0
        used[:hot, 0] = alloc[:hot, 0] - rng.randint(1, 3, size=hot)
        extra = extra.copy()
        extra[:hot, 0] = 0.0
    req = np.zeros(R, dtype=np.float32)
    req[0] = 1.0
    for r in range(1, min(R, 4)):
        req[r] = float(rng.randint(0, 4))
    bias = (rng.randint(-2, 3, size=N) * (16 / 64.0)).astype(np.float32)
    dim_w = dim_weights(R, rng)
    if inexact:
        bias = bias * INEXACT_BIAS
        dim_w = inexact_dim_weights(R, rng_x)
    return dict(
        alloc=torch.from_numpy(alloc.copy()), used=torch.from_numpy(used),
        extra=torch.from_numpy(np.ascontiguousarray(extra)),
        ready=torch.from_numpy(ready), taints=torch.from_numpy(taints),
        planes=torch.from_numpy(planes), req=torch.from_numpy(req),
        dim_w=torch.from_numpy(dim_w),
        bias=torch.from_numpy(bias))


def oracle_score_cap(st, *, req=None, tolerated=0, require=None, forbid=None,
                     w_least=1.0, w_most=0.0, w_bal=0.0, bias=None,
                     extra=True):
    """reference.score_cap on a state dict -> (score f32 [N], cap i32 [N])."""
    N = st["alloc"].shape[0]
    W = st["planes"].shape[1]
    zw = torch.zeros(W, dtype=torch.int64)
    score = torch.empty(N)
    cap = torch.empty(N, dtype=torch.int32)
    ref.score_cap(st["alloc"], st["used"],
                  st["extra"] if extra else torch.zeros_like(st["extra"]),
                  st["ready"], st["taints"], st["planes"],
                  st["req"] if req is None else req, tolerated,
                  zw if require is None else require,
                  zw if forbid is None else forbid,
                  w_least, w_most, w_bal, st["dim_w"], bias, score, cap)
    return score, cap


def score_f64(st, *, req=None, w_least=1.0, w_most=0.0, w_bal=0.0, bias=None):
    """The score formula of reference.score_cap evaluated in float64 on the
    f32 inputs (no feasibility masking) -> float64 [N]."""
    alloc = st["alloc"].double().numpy()
    used = st["used"].double().numpy()
    rq = (st["req"] if req is None else req).double().numpy()
    dw = st["dim_w"].double().numpy()
    eps = float(np.float32(EPS))
    frac = np.minimum((used + rq) / np.maximum(alloc, eps), 1.0)
    wsum = max(dw.sum(), eps)
    least = ((1.0 - frac) * dw).sum(axis=1) / wsum
    most = (frac * dw).sum(axis=1) / wsum
    mean = frac.mean(axis=1, keepdims=True)
    bal = 1.0 - np.sqrt(((frac - mean) ** 2).mean(axis=1))
    # the weights reach both implementations as f32
    s = (float(np.float32(w_least)) * least + float(np.float32(w_most)) * most
         + float(np.float32(w_bal)) * bal)
    if bias is not None:
        s = s + bias.double().numpy()
    return s


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit-for-bit equality of two f32 tensors (distinguishes +-0)."""
    return torch.equal(a.contiguous().view(torch.int32),
                       b.contiguous().view(torch.int32))


# --------------------------------------------------------------------------
# plan-level cases
# --------------------------------------------------------------------------

@dataclass
class PlanCase:
    name: str
    N: int
    R: int
    W: int
    state: Dict[str, torch.Tensor]
    classes: List[dict]                    # one dict per class (see _class)
    jobs: List[tuple]                      # (begin, end, occupied, min_avail)
    queue_limit: np.ndarray                # [3, R] f32
    queue_alloc: np.ndarray                # [3, R] f32
    bias_rows: List[np.ndarray] = field(default_factory=list)
    chain: bool = False
    w_bal: float = 0.0                     # of every class (build_plan)
    byte_dim: Optional[int] = None         # dim in decimal bytes, or None


class _Labels:
    def __init__(self, words):
        self.words = words


class StubNodes:
    """The slice of NodeTensors that run_plan_torch / run_plan_hip read."""

    def __init__(self, st, device):
        self.n, self.r = st["alloc"].shape
        self.alloc_t = st["alloc"].t().contiguous().to(device)
        self.used_t = st["used"].t().contiguous().to(device)
        self.extra_t = st["extra"].t().contiguous().to(device)
        self.ready = st["ready"].to(torch.uint8).to(device)
        self.taint_mask = st["taints"].clone().to(device)
        self.planes_t = st["planes"].t().contiguous().to(device)
        self.labels = _Labels(st["planes"].shape[1])

    def ensure_plane_width(self):
        pass


def _class(rng, R, W, ntasks, queue_idx, *, min_needed=0, bias_row=None,
           plain=False):
    req = np.zeros(R, dtype=np.float32)
    req[0] = 1.0
    for r in range(1, min(R, 4)):
        req[r] = float(rng.randint(0, 3))
    tol = np.int64(0)
    for b in (np.int64(1), np.int64(2), BIT62, BIT63):
        if plain or rng.rand() < 0.7:
            tol |= b
    require = np.zeros(W, dtype=np.int64)
    forbid = np.zeros(W, dtype=np.int64)
    if not plain:
        w = rng.randint(0, W)
        if rng.rand() < 0.4:
            require[w] = rng.choice(np.array([1, 4, BIT63], dtype=np.int64))
        if rng.rand() < 0.3:
            forbid[rng.randint(0, W)] = rng.choice(
                np.array([8, BIT62], dtype=np.int64))
    w_least, w_most = [(1.0, 0.0), (0.0, 1.0), (0.5, 2.0), (2.0, 0.5)][
        rng.randint(0, 4)]
    return dict(req=req, tolerated=int(tol), require=require, forbid=forbid,
                ntasks=int(ntasks), queue_idx=int(queue_idx),
                min_needed=int(min_needed), w_least=w_least, w_most=w_most,
                use_future=bool(rng.rand() < 0.5), bias_row=bias_row)


def _queues(rng, R, limit_dim0):
    """Three queues, non-zero integer allocations, queue 2 bound on dim 0."""
    ql = np.full((3, R), planmod.BIG_LIMIT, dtype=np.float32)
    qa = rng.randint(0, 5, size=(3, R)).astype(np.float32)
    ql[2, 0] = qa[2, 0] + float(limit_dim0)
    return ql, qa


def _bias_rows(rng, N, n_rows, hot=0, inexact=False):
    rows = []
    for _ in range(n_rows):
        row = (rng.randint(-1, 2, size=N) * (8 / 64.0)).astype(np.float32)
        if inexact:
            row = row * INEXACT_BIAS
        if hot:
            row[:hot] += 8.0
        rows.append(row)
    return rows


def mixed_case(name, N, R, W, seed, *, n_jobs=12, bulk=None, n_classes=None,
               inexact=False):
    """Single- and multi-class gangs over three queues.  ``bulk`` adds one
    600-task class: "single" as its own job, "multi" as the first class of
    a two-class gang whose second class cannot meet its role minimum."""
    rng = np.random.RandomState(seed)
    st = dyadic_state(N, R, W, seed, inexact=inexact)
    rows = _bias_rows(rng, N, 2, inexact=inexact)
    classes, jobs = [], []

    def add_job(cls, occupied, min_avail):
        b = len(classes)
        classes.extend(cls)
        jobs.append((b, len(classes), occupied, min_avail))

    if bulk == "single":
        add_job([_class(rng, R, W, 600, 0, plain=True)], 0, 300)
    elif bulk == "multi":
        a = _class(rng, R, W, 600, 0, plain=True)
        b = _class(rng, R, W, 3, 1, min_needed=4, plain=True)
        add_job([a, b], 0, 100)
    j = 0
    while (len(jobs) < n_jobs if n_classes is None
           else len(classes) < n_classes):
        kind = j % 4
        q = j % 3
        row = (j % 2) if j % 3 == 0 else None
        if kind in (0, 1):                      # single-class gang
            n = int(rng.randint(1, 40))
            # every third one asks more than can ever be placed
            need = n + 1 if j % 6 == 1 else max(1, n - int(rng.randint(0, 3)))
            add_job([_class(rng, R, W, n, q, bias_row=row)],
                    int(rng.randint(0, 2)), need)
        elif kind == 2:                         # two roles, usually ready
            n1, n2 = int(rng.randint(1, 20)), int(rng.randint(1, 20))
            add_job([_class(rng, R, W, n1, q, min_needed=1, bias_row=row),
                     _class(rng, R, W, n2, (q + 1) % 3, min_needed=0)],
                    1, max(1, (n1 + n2) // 2))
        else:                                   # one role one short
            n1, n2 = int(rng.randint(2, 10)), int(rng.randint(2, 10))
            short = j % 8 == 3
            add_job([_class(rng, R, W, n1, q, min_needed=n1, plain=True),
                     _class(rng, R, W, n2, q,
                            min_needed=n2 + 1 if short else n2, plain=True),
                     _class(rng, R, W, 2, q, min_needed=0)],
                    0, n1)
        j += 1
    if n_classes is not None:
        del classes[n_classes:]
        b, e, o, m = jobs[-1]
        jobs[-1] = (b, min(e, n_classes), o, m)
    ql, qa = _queues(rng, R, limit_dim0=25)
    return PlanCase(name, N, R, W, st, classes, jobs, ql, qa, rows,
                    w_bal=1.0 if inexact else 0.0)


def chain_case(name, N, R, W, seed, shape, *, inexact=False):
    """Runs of single-class small jobs (the chain path's diet).

    "ragged": 70 jobs of 1..12 tasks; "wide": 300 one-task jobs (``inexact``: every fourth asks three) on nodes
    with room for exactly one; "hot": 70 jobs that all prefer the same 16
    nodes, so the candidate lists of later classes are used up."""
    rng = np.random.RandomState(seed)
    hot = TOPK if shape == "hot" else 0
    st = dyadic_state(N, R, W, seed, cap_one=(shape == "wide"), hot=hot,
                      not_ready=0.02 if shape == "wide" else 0.05,
                      inexact=inexact)
    rows = _bias_rows(rng, N, 2, hot=hot, inexact=inexact)
    classes, jobs = [], []
    n_jobs = 300 if shape == "wide" else 70
    for j in range(n_jobs):
        q = 2 if j % 5 == 4 else j % 2
        if shape == "wide":
            # the inexact twin needs neighbours in a log: some jobs take
            # three nodes (every node has room for exactly one task)
            n = 3 if inexact and j % 4 == 2 else 1
            need = 2 if j % 37 == 5 else 1
        else:
            n = int(rng.randint(1, 13)) if shape == "ragged" \
                else int(rng.randint(3, 8))
            need = n + 1 if j % 11 == 3 else max(1, n - 1)
        if shape == "hot":
            row = None if j % 7 == 6 else j % 2
        else:
            row = j % 2 if j % 3 == 0 else None
        c = _class(rng, R, W, n, q, bias_row=row,
                   plain=(shape != "ragged"))
        b = len(classes)
        classes.append(c)
        jobs.append((b, b + 1, 0, need))
    ql, qa = _queues(rng, R, limit_dim0=30)
    if shape == "hot":
        st["bias"][:hot] += 4.0
    return PlanCase(name, N, R, W, st, classes, jobs, ql, qa, rows,
                    chain=True, w_bal=1.0 if inexact else 0.0)


def build_plan(case: PlanCase, device, w_bal: float = 0.0) -> CyclePlan:
    """A fresh CyclePlan (fresh node state) straight from the arrays.
    Every class gets ``w_bal``, or the case's own when that is set."""
    w_bal = case.w_bal if case.w_bal != 0.0 else w_bal
    nt = StubNodes(case.state, device)
    plan = CyclePlan(nt, torch.from_numpy(case.queue_limit.copy()),
                     torch.from_numpy(case.queue_alloc.copy()))
    plan.dim_w = case.state["dim_w"].clone()
    plan.bias = case.state["bias"].clone()
    rows = [r.copy() for r in case.bias_rows]       # shared by object id
    for j, (b, e, occ, mn) in enumerate(case.jobs):
        for c in range(b, e):
            d = case.classes[c]
            plan.classes.append(ClassPlan(
                tclass=None, job_key=f"j{j}", queue_idx=d["queue_idx"],
                req=d["req"].copy(), tolerated=d["tolerated"],
                require=d["require"].copy(), forbid=d["forbid"].copy(),
                min_needed=d["min_needed"], w_least=d["w_least"],
                w_most=d["w_most"], w_bal=w_bal, use_future=d["use_future"],
                bias=None if d["bias_row"] is None else rows[d["bias_row"]],
                ntasks_override=d["ntasks"]))
        plan.jobs.append(JobPlan(f"j{j}", b, e, occ, mn))
    plan.finalize()
    return plan


def snapshot(plan: CyclePlan, res) -> dict:
    """Everything a cycle decides, as host arrays."""
    return dict(
        log_nodes=np.asarray(res.log_nodes), log_counts=np.asarray(res.log_counts),
        log_len=np.asarray(res.log_len), class_placed=np.asarray(res.class_placed),
        job_placed=np.asarray(res.job_placed_arr), job_flag=np.asarray(res.job_flag),
        used=plan.nt.used_t.t().cpu().numpy().copy(),
        queue_alloc=plan.queue_alloc.cpu().numpy().copy(),
        log_off=np.array([cp.log_off for cp in plan.classes]),
        jobs=[(jp.class_begin, jp.class_end) for jp in plan.jobs])


def compare_results(want: dict, got: dict) -> None:
    """``want`` is the oracle's snapshot.  Raises AssertionError on the
    first difference; logs are compared entry for entry, in order."""
    assert np.array_equal(want["log_len"], got["log_len"]), "log_len differs"
    for c, (off, n) in enumerate(zip(want["log_off"], want["log_len"])):
        sl = slice(int(off), int(off) + int(n))
        assert np.array_equal(want["log_nodes"][sl], got["log_nodes"][sl]), \
            f"class {c}: log_nodes {want['log_nodes'][sl]} vs {got['log_nodes'][sl]}"
        assert np.array_equal(want["log_counts"][sl], got["log_counts"][sl]), \
            f"class {c}: log_counts {want['log_counts'][sl]} vs {got['log_counts'][sl]}"
    assert np.array_equal(want["class_placed"], got["class_placed"]), \
        "class_placed differs"
    assert np.array_equal(want["job_placed"], got["job_placed"]), \
        "job_placed differs"
    assert np.array_equal(want["used"], got["used"]), "final used differs"
    assert np.array_equal(want["queue_alloc"], got["queue_alloc"]), \
        "final queue_alloc differs"
    for j, (b, e) in enumerate(want["jobs"]):
        if e - b > 1:
            assert want["job_flag"][j] == got["job_flag"][j], \
                f"job {j}: flag differs"
        elif want["job_flag"][j] == 0:
            # the fused single-class paths revert in the select kernel and
            # never write the job flag: the visible outcome is placed == 0
            assert got["class_placed"][b] == 0, \
                f"job {j}: reverted single-class job kept placements"


@contextlib.contextmanager
def _recording(records: list):
    """Record the inputs of every oracle select_commit of a plan run."""
    real = ref.select_commit

    def spy(score, cap, req, ntasks, used, queue_alloc, queue_limit, *rest):
        pos = req > EPS
        per = torch.where(pos, (queue_limit - queue_alloc + EPS)
                          / torch.clamp(req, min=EPS),
                          torch.full_like(req, float(BIG_CAP)))
        quota = int(per.amin().clamp(min=0, max=float(BIG_CAP)).floor())
        feas = score > NEG_INF
        records.append(dict(
            score=score.clone(), cap=cap.clone(), quota=quota,
            ntasks=int(ntasks), room=int(cap[feas].to(torch.int64).sum()),
            used=used.clone()))
        return real(score, cap, req, ntasks, used, queue_alloc, queue_limit,
                    *rest)

    planmod.ref.select_commit = spy
    try:
        yield
    finally:
        planmod.ref.select_commit = real


def run_oracle(case: PlanCase):
    """run_plan_torch on CPU -> (snapshot, per-class records, plan)."""
    plan = build_plan(case, "cpu")
    records: list = []
    with _recording(records):
        res = planmod.run_plan_torch(plan)
    return snapshot(plan, res), records, plan


def plan_conditions(case: PlanCase, snap: dict, records: list,
                    chunk: Optional[int] = None) -> Dict[str, bool]:
    """What the oracle's run of a case exercises (non-vacuity)."""
    out = dict(reverts=bool((snap["job_flag"] == 0).any()),
               commits=bool(((snap["job_flag"] == 1)
                             & (snap["job_placed"] > 0)).any()),
               quota_cut=False, index_tie=False)
    for c, rec in enumerate(records):
        if rec["quota"] < min(rec["ntasks"], rec["room"]):
            out["quota_cut"] = True
        off, n = int(snap["log_off"][c]), int(snap["log_len"][c])
        picked = set(snap["log_nodes"][off:off + n].tolist())
        if not picked:
            continue
        score = rec["score"]
        # a picked score shared by >= 3 feasible nodes: the index alone
        # decides which of them is taken, or in which order they are logged
        for node in picked:
            group = torch.nonzero(score == score[node]).flatten().tolist()
            if len(group) >= 3 and (sum(g in picked for g in group) >= 2
                                    or any(g not in picked for g in group)):
                out["index_tie"] = True
                break
    if chunk is not None:
        out.update(_chain_conditions(case, snap, records, chunk))
    return out


def _chain_conditions(case, snap, records, chunk):
    """Replay of the chain path's bookkeeping on the oracle's decisions:
    per chunk, scores are a snapshot taken at the chunk's first class and
    every node an earlier class of the chunk logged is "touched"."""
    assert all(e - b == 1 for b, e, _, _ in case.jobs)
    st = case.state
    exhausted = False
    most_touched = 0
    C = len(case.classes)
    for c0 in range(0, C, chunk):
        at_start = dict(st, used=records[c0]["used"])
        touched: set = set()
        for c in range(c0, min(c0 + chunk, C)):
            d = case.classes[c]
            if d["bias_row"] is None:
                bias = st["bias"]
            else:
                bias = torch.from_numpy(case.bias_rows[d["bias_row"]]) \
                    + st["bias"]
            score, _ = oracle_score_cap(
                at_start, req=torch.from_numpy(d["req"]),
                tolerated=d["tolerated"],
                require=torch.from_numpy(d["require"]),
                forbid=torch.from_numpy(d["forbid"]), w_least=d["w_least"],
                w_most=d["w_most"], w_bal=case.w_bal, bias=bias,
                extra=d["use_future"])
            order = torch.argsort(score, descending=True, stable=True)[:TOPK]
            budget = min(records[c]["ntasks"], records[c]["quota"])
            if (len(order) == TOPK and bool((score[order] > NEG_INF).all())
                    and budget > 0
                    and all(int(i) in touched for i in order)):
                exhausted = True
            off, n = int(snap["log_off"][c]), int(snap["log_len"][c])
            touched.update(snap["log_nodes"][off:off + n].tolist())
        most_touched = max(most_touched, len(touched))
    return dict(topk_exhausted=exhausted,
                wide_touched=most_touched > CHAIN_THREADS)


# name -> (builder, conditions every run must meet, chunk sizes for the
# chain replay).  Seeds were chosen on the CPU so the oracle alone meets
# the conditions; tests/test_kernel_cases.py re-checks them every run.
BASE = ("reverts", "commits", "quota_cut", "index_tie")
SHAPES = ((5, 1), (64, 4))          # (R, W) of every plan


def plan_cases() -> Dict[str, tuple]:
    cases = {}
    for R, W in SHAPES:
        tag = f"R{R}W{W}"
        cases[f"fused-{tag}"] = (
            lambda R=R, W=W: mixed_case("fused", 1000, R, W, 11), BASE, ())
        cases[f"split-{tag}"] = (
            lambda R=R, W=W: mixed_case("split", 4097, R, W, 12), BASE, ())
        cases[f"bulk-single-{tag}"] = (
            lambda R=R, W=W: mixed_case("bulk1", 1000, R, W, 13,
                                        bulk="single"), BASE, ())
        cases[f"bulk-multi-{tag}"] = (
            lambda R=R, W=W: mixed_case("bulk2", 4097, R, W, 14,
                                        bulk="multi"), BASE, ())
        cases[f"mega-{tag}"] = (
            lambda R=R, W=W: mixed_case("mega", 1000, R, W, 15,
                                        n_classes=40), BASE, ())
        cases[f"chain-ragged-{tag}"] = (
            lambda R=R, W=W: chain_case("ragged", 1000, R, W, 16, "ragged"),
            BASE, ())
        cases[f"chain-wide-{tag}"] = (
            lambda R=R, W=W: chain_case("wide", 600, R, W, 17, "wide"),
            BASE, ((512, "wide_touched"),))
        cases[f"chain-hot-{tag}"] = (
            lambda R=R, W=W: chain_case("hot", 1000, R, W, 18, "hot"),
            BASE, ((8, "topk_exhausted"), (512, "topk_exhausted")))
    return cases


# --------------------------------------------------------------------------
# score_cap shapes shared by the CPU exactness check and the GPU edge test
# --------------------------------------------------------------------------
SCORE_NS = (1, 63, 64, 65, 255, 257)
SCORE_RW = ((1, 1), (16, 4), (17, 1), (64, 4))
SCORE_WEIGHTS = ((1.0, 0.0), (0.5, 2.0))      # (w_least, w_most)
GRID_WRAP = (4096 * 256 + 77, 2, 1)           # one node past 4096 x 256
W_BAL = 0.25
# Largest |f32 oracle - float64 formula| over every (N, R, W) above with
# w_bal = W_BAL, seeds 0..2, bias on and off, both weight pairs, measured
# on the CPU: 1.33e-7 (scores are below 4, one f32 ulp there is 2.4e-7).
# tests/test_kernel_cases.py re-measures it on every run.
BAL_ERR_F32 = 1.4e-7


# --------------------------------------------------------------------------
# the inexact family: plan cases, error bounds, float64 validator
# --------------------------------------------------------------------------

def inexact_plan_cases() -> Dict[str, tuple]:
    """An inexact twin (``w_bal`` = 1) of every plan shape, same layout as
    ``plan_cases``; the mega and the chain shapes at N = 1000 (per-class
    path is the fused kernel) and N = 4097 (score + select)."""
    cases = {}
    for R, W in SHAPES:
        tag = f"R{R}W{W}"
        cases[f"fused-{tag}"] = (
            lambda R=R, W=W: mixed_case("fused", 1000, R, W, 21,
                                        inexact=True), BASE, ())
        cases[f"split-{tag}"] = (
            lambda R=R, W=W: mixed_case("split", 4097, R, W, 22,
                                        inexact=True), BASE, ())
        cases[f"bulk-single-{tag}"] = (
            lambda R=R, W=W: mixed_case("bulk1", 1000, R, W, 23,
                                        bulk="single", inexact=True),
            BASE, ())
        cases[f"bulk-multi-{tag}"] = (
            lambda R=R, W=W: mixed_case("bulk2", 4097, R, W, 24,
                                        bulk="multi", inexact=True),
            BASE, ())
        for N in (1000, 4097):
            cases[f"mega-N{N}-{tag}"] = (
                lambda R=R, W=W, N=N: mixed_case(
                    "mega", N, R, W, 25, n_classes=40, inexact=True),
                BASE, ())
            cases[f"chain-ragged-N{N}-{tag}"] = (
                lambda R=R, W=W, N=N: chain_case(
                    "ragged", N, R, W, 26, "ragged", inexact=True),
                BASE, ())
            cases[f"chain-hot-N{N}-{tag}"] = (
                lambda R=R, W=W, N=N: chain_case(
                    "hot", N, R, W, 28, "hot", inexact=True),
                BASE, ((8, "topk_exhausted"), (512, "topk_exhausted")))
        for N in (600, 4097):
            cases[f"chain-wide-N{N}-{tag}"] = (
                lambda R=R, W=W, N=N: chain_case(
                    "wide", N, R, W, 27, "wide", inexact=True),
                BASE, ((512, "wide_touched"),))
    return cases


def class_bias(case: PlanCase, c: int) -> torch.Tensor:
    """The bias plane class ``c`` is scored with (CyclePlan.finalize folds
    the plan-wide plane into a class's own row with one f32 add)."""
    row = case.classes[c]["bias_row"]
    if row is None:
        return case.state["bias"]
    return torch.from_numpy(case.bias_rows[row]) + case.state["bias"]


def kernel_replay_f32(st, *, req=None, w_least=1.0, w_most=0.0, w_bal=0.0,
                      bias=None, fused=False) -> np.ndarray:
    """The score of ``node_score_one`` in the kernel's own operation order,
    in numpy f32: serial sums over R, a second pass over R for the
    variance, ``w_least*least/wsum + w_most*most/wsum + w_bal*bal``, then
    the bias.  ``fused`` turns every ``a*b + c`` of that text into one
    rounding (the product is exact in float64, so the float64 sum rounded
    to f32 is the fused result up to a double rounding); without it every
    operation rounds on its own.  No feasibility masking -> f32 [N]."""
    f32 = np.float32
    alloc = st["alloc"].numpy()
    used = st["used"].numpy()
    rq = (st["req"] if req is None else req).numpy()
    dw = st["dim_w"].numpy()
    N, R = alloc.shape
    eps = f32(EPS)

    def mad(a, b, c):
        if fused:
            return (a.astype(np.float64) * np.float64(b)
                    + c.astype(np.float64)).astype(f32)
        return (a * b).astype(f32) + c

    wsum = f32(0)
    for r in range(R):
        wsum = f32(wsum + dw[r])
    wsum = max(wsum, eps)
    one = f32(1)
    least = np.zeros(N, f32)
    most = np.zeros(N, f32)
    mean = np.zeros(N, f32)
    fr = []
    for r in range(R):
        f = np.minimum((used[:, r] + rq[r]) / np.maximum(alloc[:, r], eps),
                       one)
        fr.append(f)
        least = mad(one - f, dw[r], least)
        most = mad(f, dw[r], most)
        mean = mean + f
    mean = mean / f32(R)
    s = (f32(w_least) * least) / wsum + (f32(w_most) * most) / wsum
    if w_bal != 0.0:
        var = np.zeros(N, f32)
        for f in fr:
            d = f - mean
            var = mad(d, d, var)
        bal = one - np.sqrt(var / f32(R))
        s = mad(bal, f32(w_bal), s)
    if bias is not None:
        s = s + bias.numpy()
    assert s.dtype == f32
    return s


# Worst |score - float64 formula| over every feasible node of every class
# of every inexact plan case, against the usage the class really saw,
# measured on the CPU and re-measured by tests/test_inexact_cases.py on
# every run (scores reach 14.6 on the "hot" shapes, where one f32 ulp is
# 9.5e-7):
#   f32 torch oracle                        7.07e-7
#   kernel op order, no a*b+c fused         7.07e-7
#   kernel op order, every a*b+c fused      6.85e-7
# (the oracle sums over R column by column, as the kernel does, so the
# unfused replay reproduces it)
SCORE_ERR_F32 = 7.1e-7
REPLAY_ERR_UNFUSED = 7.1e-7
REPLAY_ERR_FUSED = 6.9e-7
# What a kernel's score may differ from the float64 formula.  The margin
# of 2 is there because the device compiler may fuse ANY subset of the
# a*b+c sites, per inlining context; the two replays only measure the two
# ends.  Never derived from a kernel's output.
KERNEL_ERR = 2 * max(SCORE_ERR_F32, REPLAY_ERR_UNFUSED, REPLAY_ERR_FUSED)
# The same three figures on test_ops_gpu.rand_state(4096, 6), the inputs of
# test_score_cap_matches_oracle (scores below 2.1): the largest is 3.17e-7
RAND_KERNEL_ERR = 2 * 3.2e-7
RAND_SCORE_SHAPES = ((177, 8), (10000, 8), (2000, 20), (1000, 61))
RAND_SCORE_SEEDS = (0, 1, 2)


def rand_score_case(rand_state, N, R, seed):
    """Inputs of test_ops_gpu.test_score_cap_matches_oracle (``rand_state``
    is that module's generator) -> (state, score weights, class masks)."""
    st = rand_state(N=N, R=R, seed=seed)
    g = torch.Generator().manual_seed(seed + 4242)
    st["dim_w"] = torch.rand(R, generator=g) + 0.5
    return (st, dict(w_least=1.0, w_most=0.7, w_bal=0.3),
            dict(tolerated=0b01,
                 require=torch.tensor([0b1010, 0], dtype=torch.int64),
                 forbid=torch.tensor([0b0100, 0], dtype=torch.int64)))


class PlanInvalid(AssertionError):
    pass


def _static_ok(st, d) -> np.ndarray:
    """ready, taints and label planes of one class, in Python integers'
    two's complement via numpy int64 (bit tests only)."""
    taints = st["taints"].numpy()
    planes = st["planes"].numpy()
    ok = st["ready"].numpy().astype(bool)
    ok = ok & ((taints & ~np.int64(d["tolerated"])) == 0)
    ok = ok & ((planes & d["require"]) == d["require"]).all(axis=1)
    ok = ok & ((planes & d["forbid"]) == 0).all(axis=1)
    return ok


def _caps(avail, req):
    eps = float(np.float32(EPS))
    pos = req > eps
    per = np.where(pos, np.floor((avail + eps) / np.maximum(req, eps)),
                   float(BIG_CAP))
    return np.clip(per.min(axis=-1), 0, float(BIG_CAP)).astype(np.int64)


def validate_plan(case: PlanCase, snap: dict, tol: Optional[float] = None
                  ) -> Dict[str, int]:
    """Replay the snapshot of ANY runner in float64 and raise PlanInvalid
    on the first violation.  The f32 oracle is never called: usage, quota,
    feasibility and capacity are recomputed exactly (integers on these
    inputs), scores with ``score_f64``.  Class by class, in plan order:

    * every logged node is feasible, its count is min(cap, budget left);
    * consecutive entries: f64(e) >= f64(e+1) - tol, and a *tied* pair
      (identical alloc row, usage row, extra row under use_future, and bias
      value -> equal scores on any correct implementation) ascends in
      node index, no tolerance;
    * no feasible node is left out while budget remains; once the budget
      ran out none of them scores above the last entry + tol, and a twin
      of a logged node has a higher index than every logged twin;
    * counters and flags follow from the counts and the gang minimums, a
      discarded class has zeroed counts, final usage and queue allocation
      equal the replay exactly.

    ``tol`` defaults to 2 * KERNEL_ERR (both scores of a pair may be off).
    Returns how many consecutive pairs were tied / forced (gap > tol) /
    ambiguous (neither)."""
    tol = 2 * KERNEL_ERR if tol is None else tol
    st = case.state
    alloc = st["alloc"].double().numpy()
    extra = st["extra"].double().numpy()
    used = st["used"].double().numpy().copy()
    qa = case.queue_alloc.astype(np.float64)
    ql = case.queue_limit.astype(np.float64)
    stats = dict(tied=0, forced=0, ambiguous=0)

    def bad(msg):
        raise PlanInvalid(f"{case.name}: {msg}")

    for j, (b, e, occupied, min_avail) in enumerate(case.jobs):
        saved = (used.copy(), qa.copy())
        totals, expect, ok = [], [], True
        for c in range(b, e):
            d = case.classes[c]
            req = d["req"].astype(np.float64)
            off, n = int(snap["log_off"][c]), int(snap["log_len"][c])
            nodes = snap["log_nodes"][off:off + n].astype(np.int64)
            counts = snap["log_counts"][off:off + n].astype(np.int64)
            avail = alloc - used + (extra if d["use_future"] else 0.0)
            eps = float(np.float32(EPS))
            cap = _caps(avail, req)
            feas = _static_ok(st, d) & (avail + eps >= req).all(axis=1) \
                & (cap > 0)
            quota = int(_caps(ql[d["queue_idx"]] - qa[d["queue_idx"]], req))
            budget = min(d["ntasks"], quota)
            bias = class_bias(case, c)
            used32 = used.astype(np.float32)
            assert np.array_equal(used32.astype(np.float64), used)
            s64 = score_f64(dict(st, used=torch.from_numpy(used32)),
                            req=torch.from_numpy(d["req"]),
                            w_least=d["w_least"], w_most=d["w_most"],
                            w_bal=case.w_bal, bias=bias)
            key = [st["alloc"].numpy(), used32, bias.numpy()[:, None]]
            if d["use_future"]:
                key.append(st["extra"].numpy())
            key = np.concatenate(key, axis=1)

            def twins(a, b_):
                return bool(np.array_equal(key[a], key[b_]))

            if len(set(nodes.tolist())) != n:
                bad(f"class {c}: a node is logged twice")
            left, want = budget, []
            for k, node in enumerate(nodes.tolist()):
                if not 0 <= node < case.N or not feas[node]:
                    bad(f"class {c}: entry {k} logs infeasible node {node}")
                if left <= 0:
                    bad(f"class {c}: entry {k} logged past the budget")
                want.append(min(int(cap[node]), left))
                left -= want[-1]
            total = budget - left
            for k in range(n - 1):
                x, y = int(nodes[k]), int(nodes[k + 1])
                gap = s64[x] - s64[y]
                if twins(x, y):
                    stats["tied"] += 1
                    if x > y:
                        bad(f"class {c}: tied nodes {x}, {y} not in index "
                            f"order at entries {k}, {k + 1}")
                elif gap > tol:
                    stats["forced"] += 1
                else:
                    stats["ambiguous"] += 1
                    if gap < -tol:
                        bad(f"class {c}: entry {k + 1} (node {y}) beats "
                            f"entry {k} (node {x}) by {-gap:.3e}")
            unlogged = feas.copy()
            unlogged[nodes] = False
            if left > 0 and unlogged.any():
                bad(f"class {c}: budget left ({left}) but feasible node "
                    f"{int(np.flatnonzero(unlogged)[0])} is not logged")
            if n and unlogged.any():
                last = s64[int(nodes[-1])]
                over = np.flatnonzero(unlogged & (s64 > last + tol))
                if over.size:
                    bad(f"class {c}: unlogged node {int(over[0])} beats the "
                        f"last entry by {s64[over[0]] - last:.3e}")
                near = np.flatnonzero(unlogged & (s64 >= last - tol))
                logged_near = [int(x) for x in nodes.tolist()
                               if s64[x] <= last + tol]
                for u in near.tolist():
                    for x in logged_near:
                        if x > u and s64[x] == s64[u] and twins(x, u):
                            bad(f"class {c}: node {u} skipped for its "
                                f"higher-index twin {x}")
            totals.append(total)
            expect.append((c, nodes, counts, np.array(want, dtype=np.int64),
                           req, d))
            # stage: the job's later classes see this usage
            np.add.at(used, nodes, np.array(want, dtype=np.float64)[:, None]
                      * req[None, :])
            qa[d["queue_idx"]] += total * req
        if e - b == 1:
            d = case.classes[b]
            ok = totals[0] >= max(min_avail - occupied, d["min_needed"], 0)
            if snap["job_flag"][j] == 0 and ok:
                bad(f"job {j}: flag 0 on a gang that reached its minimum")
        else:
            ok = sum(totals) + occupied >= min_avail and all(
                t >= case.classes[c]["min_needed"]
                for t, c in zip(totals, range(b, e)))
            if int(snap["job_flag"][j]) != int(ok):
                bad(f"job {j}: flag {snap['job_flag'][j]}, gang ready = {ok}")
        for (c, nodes, counts, want, req, d), total in zip(expect, totals):
            if not np.array_equal(counts, want if ok else 0 * want):
                bad(f"class {c}: counts {counts.tolist()}, expected "
                    f"{(want if ok else 0 * want).tolist()}")
            if int(snap["class_placed"][c]) != (total if ok else 0):
                bad(f"class {c}: class_placed {snap['class_placed'][c]}, "
                    f"expected {total if ok else 0}")
        if int(snap["job_placed"][j]) != (sum(totals) if ok else 0):
            bad(f"job {j}: job_placed {snap['job_placed'][j]}")
        if not ok:
            used, qa = saved                      # discarded: no trace
    if not np.array_equal(snap["used"].astype(np.float64), used):
        i = np.argwhere(snap["used"].astype(np.float64) != used)[0]
        bad(f"final used differs at node {i[0]} dim {i[1]}")
    if not np.array_equal(snap["queue_alloc"].astype(np.float64), qa):
        bad("final queue_alloc differs")
    return stats


# --------------------------------------------------------------------------
# decimal byte-scale usage: a discarded single-class gang leaves no trace
# --------------------------------------------------------------------------
BYTE_REQS = (2.5e8, 7.0e8, 1.1e9, 1.5e9)       # "250M" ... "1500M"
BYTE_ALLOC = 270186586112.0                     # 263856432Ki
BYTE_DIM = 1                                    # of the plan cases


def residue_f32(u, count, req, fused):
    """``u + count*req - count*req`` in f32, elementwise: with the product
    rounded on its own, or folded into each add (one rounding per step,
    through float64 where the product is exact)."""
    u = np.asarray(u, dtype=np.float32)
    c = np.asarray(count).astype(np.float32)
    r = np.asarray(req, dtype=np.float32)
    if fused:
        p = c.astype(np.float64) * r.astype(np.float64)
        up = (u.astype(np.float64) + p).astype(np.float32)
        return (up.astype(np.float64) - p).astype(np.float32)
    p = (c * r).astype(np.float32)
    return ((u + p).astype(np.float32) - p).astype(np.float32)


def ulp_f32(x):
    """Spacing of f32 at |x| (the gap to the next float up)."""
    x = np.abs(np.asarray(x, dtype=np.float32))
    return np.nextafter(x, np.float32(np.inf)) - x


def byte_select_inputs(N: int, R: int, seed: int) -> dict:
    """Scores, capacities and byte-scale state for one select: dim 0 is
    memory in bytes (requests from BYTE_REQS, usage sums of them), the
    other dims small integers.  ``fuse_fail`` is one above what a class of
    ``ntasks`` can place, so the gang is discarded."""
    rng = np.random.RandomState(seed)
    req = rng.randint(0, 4, size=R).astype(np.float32)
    req[0] = np.float32(BYTE_REQS[seed % 4])
    used = rng.randint(0, 50, size=(N, R)).astype(np.float32)
    used[:, 0] = (rng.randint(0, 40, size=N) * np.float32(7.0e8)
                  + rng.randint(0, 40, size=N) * np.float32(1.5e9))
    qa = rng.randint(1, 20, size=R).astype(np.float32)
    qa[0] = np.float32(37 * 7.0e8 + 11 * 1.5e9)
    score = (rng.randint(0, 64, size=N) / np.float32(7.0)).astype(np.float32)
    score[rng.rand(N) < 0.1] = NEG_INF
    cap = rng.randint(1, 9, size=N).astype(np.int32)
    cap[score == NEG_INF] = 0
    return dict(score=torch.from_numpy(score), cap=torch.from_numpy(cap),
                req=torch.from_numpy(req), used=torch.from_numpy(used),
                qa=torch.from_numpy(qa), room=int(cap.sum()))


def byte_state(N: int, R: int, seed: int) -> Dict[str, torch.Tensor]:
    """An inexact state whose dim 0 is memory in bytes: alloc around
    BYTE_ALLOC, usage sums of BYTE_REQS, request 1500M."""
    st = dyadic_state(N, R, 1, seed, inexact=True)
    rng = np.random.RandomState(seed + 1)
    st["alloc"][:, 0] = torch.from_numpy(
        (BYTE_ALLOC - rng.randint(0, 4, size=N) * 2.0 ** 30)
        .astype(np.float32))
    st["used"][:, 0] = torch.from_numpy(
        (rng.randint(0, 40, size=N) * np.float32(7.0e8)
         + rng.randint(0, 40, size=N) * np.float32(1.5e9)))
    st["extra"][:, 0] = 0.0
    st["req"][0] = BYTE_REQS[3]
    return st


def _byte_scaled(case: PlanCase, dim: int = BYTE_DIM) -> PlanCase:
    """``case`` with ``dim`` turned into memory in bytes.  Every new value
    is a function of the small integer it replaces, so twins stay twins;
    the dim never binds (capacity > 100 everywhere), it only moves scores
    and makes every usage update round."""
    st = {k: v.clone() for k, v in case.state.items()}
    f32 = np.float32
    a, u, x = (st[k].numpy() for k in ("alloc", "used", "extra"))
    k = u[:, dim].copy()
    a[:, dim] = (BYTE_ALLOC - a[:, dim].astype(np.float64) * 2.0 ** 24
                 ).astype(f32)
    # sums that straddle 2^36: one more task often crosses the binade
    u[:, dim] = ((40 + k % 6) * f32(1.5e9) + (k % 5) * f32(7.0e8)
                 + (k % 3) * f32(2.5e8)).astype(f32)
    x[:, dim] = x[:, dim] * f32(2.5e8)
    classes = []
    for c, d in enumerate(case.classes):
        d = dict(d, req=d["req"].copy())
        d["req"][dim] = f32(BYTE_REQS[(int(d["req"][dim]) + c) % 4])
        classes.append(d)
    qa = case.queue_alloc.copy()
    qa[:, dim] = qa[:, dim] * f32(1.1e9)
    st["req"][dim] = BYTE_REQS[0]
    return PlanCase(case.name + "-bytes", case.N, case.R, case.W, st,
                    classes, list(case.jobs), case.queue_limit.copy(), qa,
                    case.bias_rows, chain=case.chain, w_bal=case.w_bal,
                    byte_dim=dim)


def byte_plan_cases() -> Dict[str, tuple]:
    """One inexact plan per single-class path with byte-scale memory in
    BYTE_DIM.  Usage is no longer integer there, so these cases do not go
    through validate_plan: they are compared path against path, and
    against the same plan without its discarded jobs."""
    R, W = SHAPES[0]
    return {
        "fused-bytes": (lambda: _byte_scaled(mixed_case(
            "fused", 1000, R, W, 35, inexact=True)), BASE, ()),
        "mega-bytes": (lambda: _byte_scaled(mixed_case(
            "mega", 1000, R, W, 25, n_classes=40, inexact=True)), BASE, ()),
        "chain-bytes": (lambda: _byte_scaled(chain_case(
            "ragged", 1000, R, W, 26, "ragged", inexact=True)), BASE, ()),
    }


def discarded_single_jobs(case: PlanCase, snap: dict) -> List[int]:
    """Single-class jobs that logged nodes and were discarded."""
    return [j for j, (b, e, _, _) in enumerate(case.jobs)
            if e - b == 1 and snap["log_len"][b] > 0
            and snap["class_placed"][b] == 0]


def without_jobs(case: PlanCase, drop) -> PlanCase:
    """The same plan with the jobs in ``drop`` taken out."""
    classes, jobs = [], []
    for j, (b, e, occ, mn) in enumerate(case.jobs):
        if j in drop:
            continue
        jobs.append((len(classes), len(classes) + e - b, occ, mn))
        classes.extend(case.classes[b:e])
    return PlanCase(case.name + "-pruned", case.N, case.R, case.W,
                    case.state, classes, jobs, case.queue_limit,
                    case.queue_alloc, case.bias_rows, chain=case.chain,
                    w_bal=case.w_bal, byte_dim=case.byte_dim)


def same_trace(full: dict, pruned: dict, case: PlanCase, drop) -> None:
    """``pruned`` ran ``without_jobs(case, drop)``: every surviving class
    must have logged the same entries, and final usage and queue
    allocation must be bit-equal — the dropped jobs left no trace."""
    keep = [j for j in range(len(case.jobs)) if j not in drop]
    pc = 0
    for j in keep:
        b, e, _, _ = case.jobs[j]
        for c in range(b, e):
            for key in ("log_nodes", "log_counts"):
                a = full[key][int(full["log_off"][c]):][:int(full["log_len"][c])]
                p = pruned[key][int(pruned["log_off"][pc]):][
                    :int(pruned["log_len"][pc])]
                assert np.array_equal(a, p), \
                    f"class {c}: {key} {a} vs {p} without the discarded jobs"
            assert full["class_placed"][c] == pruned["class_placed"][pc]
            pc += 1
    for key in ("used", "queue_alloc"):
        assert same_bits(torch.from_numpy(full[key]),
                         torch.from_numpy(pruned[key])), \
            f"final {key}: a discarded single-class job left a trace"


# (N, R, seed): seeds chosen on the CPU so that both rounding forms leave a
# residue at both class sizes (tests/test_inexact_cases.py re-checks)
BYTE_SELECT_SHAPES = ((100, 1, 1), (100, 6, 1), (1025, 1, 2), (1025, 6, 1))
BYTE_SELECT_TASKS = (60, 600)            # serial select, sort-based select


def select_log(inp: dict, ntasks: int):
    """What reference.select_commit logs for ``byte_select_inputs`` with no
    queue limit -> (nodes, counts, placed)."""
    N, R = inp["used"].shape
    K = max(1, min(ntasks, N))
    ln = torch.zeros(K, dtype=torch.int32)
    lc = torch.zeros(K, dtype=torch.int32)
    ll, pl, jp = (torch.zeros((), dtype=torch.int32) for _ in range(3))
    ref.select_commit(inp["score"].clone(), inp["cap"], inp["req"], ntasks,
                      inp["used"].clone(), inp["qa"].clone(),
                      torch.full((R,), 1.0e18), ln, lc, ll, pl, jp)
    m = int(ll)
    return ln[:m].numpy(), lc[:m].numpy(), int(pl)


def select_residues(used, req, nodes, counts):
    """How many (node, dim) elements ``used`` would NOT get back from f32
    add-then-subtract of the logged placements -> (unfused, fused)."""
    u = used.numpy()[nodes]
    out = []
    for fused in (False, True):
        back = residue_f32(u, counts[:, None], req.numpy()[None, :], fused)
        out.append(int((back != u).sum()))
    return tuple(out)
