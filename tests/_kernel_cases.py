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


def dyadic_state(N: int, R: int, W: int, seed: int, *, n_types: int = 12,
                 cap_one: bool = False, not_ready: float = 0.05,
                 hot: int = 0) -> Dict[str, torch.Tensor]:
    """Node state + one request on which the f32 score is exact.

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
    return dict(
        alloc=torch.from_numpy(alloc.copy()), used=torch.from_numpy(used),
        extra=torch.from_numpy(np.ascontiguousarray(extra)),
        ready=torch.from_numpy(ready), taints=torch.from_numpy(taints),
        planes=torch.from_numpy(planes), req=torch.from_numpy(req),
        dim_w=torch.from_numpy(dim_weights(R, rng)),
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


def _bias_rows(rng, N, n_rows, hot=0):
    rows = []
    for _ in range(n_rows):
        row = (rng.randint(-1, 2, size=N) * (8 / 64.0)).astype(np.float32)
        if hot:
            row[:hot] += 8.0
        rows.append(row)
    return rows


def mixed_case(name, N, R, W, seed, *, n_jobs=12, bulk=None, n_classes=None):
    """Single- and multi-class gangs over three queues.  ``bulk`` adds one
    600-task class: "single" as its own job, "multi" as the first class of
    a two-class gang whose second class cannot meet its role minimum."""
    rng = np.random.RandomState(seed)
    st = dyadic_state(N, R, W, seed)
    rows = _bias_rows(rng, N, 2)
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
    return PlanCase(name, N, R, W, st, classes, jobs, ql, qa, rows)


def chain_case(name, N, R, W, seed, shape):
    """Runs of single-class small jobs (the chain path's diet).

    "ragged": 70 jobs of 1..12 tasks; "wide": 300 one-task jobs on nodes
    with room for exactly one; "hot": 70 jobs that all prefer the same 16
    nodes, so the candidate lists of later classes are used up."""
    rng = np.random.RandomState(seed)
    hot = TOPK if shape == "hot" else 0
    st = dyadic_state(N, R, W, seed, cap_one=(shape == "wide"), hot=hot,
                      not_ready=0.02 if shape == "wide" else 0.05)
    rows = _bias_rows(rng, N, 2, hot=hot)
    classes, jobs = [], []
    n_jobs = 300 if shape == "wide" else 70
    for j in range(n_jobs):
        q = 2 if j % 5 == 4 else j % 2
        if shape == "wide":
            n = 1
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
                    chain=True)


def build_plan(case: PlanCase, device) -> CyclePlan:
    """A fresh CyclePlan (fresh node state) straight from the arrays."""
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
                w_most=d["w_most"], w_bal=0.0, use_future=d["use_future"],
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
                w_most=d["w_most"], bias=bias, extra=d["use_future"])
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
