"""Pure-PyTorch reference implementations of the scheduler kernels.

These define the *semantics* the HIP kernels (``csrc/scheduler_kernels.hip``)
must reproduce exactly on the decision level (same placements, same ready
flags).  They run on CPU for the non-GPU test tier and are the golden
oracle for the GPU numerics tests.

Design rule — **sync-free hot loop**: every op is buffer-style (writes into
caller-provided device tensors, returns nothing host-visible).  The per-job
gang decision (commit vs revert) is made *on device* so a whole scheduling
cycle is one enqueue of kernels on one HIP stream with a single D2H readback
at the end.  The reference (Go) makes the same decisions with per-task
host code — the order-equivalent semantics are documented per op.

Kernel inventory (SURVEY.md §2.9 K1–K6 mapping):

* ``score_cap``      — K1+K2 fused: feasibility + capacity + score per node.
* ``select_commit``  — K2 select + K4 gang placement with undo log.
* ``finalize_job``   — K4 gang readiness decision (device flag).
* ``cond_revert``    — K4 rollback of one class, gated on the job flag.
* ``spread_select_commit`` / ``spread_revert`` — K2 select under a
  topology-spread bound checked before every placement, and its rollback.
* ``affinity_select_commit`` — K2 select under an inter-pod (anti-)affinity
  domain rule checked before every placement (reverts: ``spread_revert``).
* ``drf_share``      — K3 dominant share per job.
* ``waterfill``      — K3 proportion/capacity deserved water-filling.

Decision determinism: score ties break toward the lower node index
(everywhere — CPU reference, HIP kernels, torch fallbacks).
"""

from __future__ import annotations

from typing import Optional

import torch

NEG_INF = float("-inf")
EPS = 1e-4          # resource-fit slack, mirrors api/resource.MIN_RESOURCE scale
BIG_CAP = 2 ** 30   # "unbounded" capacity sentinel


def _row_sum(x: torch.Tensor) -> torch.Tensor:
    """Sum over the resource dim, one column after the other (the kernel's
    order).  ``x.sum(dim=1)`` vectorizes across rows and rounds a row
    differently depending on where in the tensor it sits, so two nodes
    with identical inputs could get different scores and a tie would no
    longer go to the lower index; elementwise adds cannot do that."""
    acc = torch.zeros(x.shape[0], dtype=x.dtype, device=x.device)
    for r in range(x.shape[1]):
        acc = acc + x[:, r]
    return acc


def score_cap(
    alloc: torch.Tensor,        # [N, R] f32 allocatable
    used: torch.Tensor,         # [N, R] f32 currently used (incl. staged)
    extra: torch.Tensor,        # [N, R] f32 future credit (releasing − pipelined); zeros for idle-only
    ready: torch.Tensor,        # [N] bool node schedulable
    taints: torch.Tensor,       # [N] i64 taint bitmask
    planes: torch.Tensor,       # [N, W] i64 label planes
    req: torch.Tensor,          # [R] f32 per-task request
    tolerated: int,             # i64 taint bits this class tolerates
    require: torch.Tensor,      # [W] i64 plane bits that must all be set
    forbid: torch.Tensor,       # [W] i64 plane bits that must all be clear
    w_least: float,             # leastrequested weight (nodeorder)
    w_most: float,              # mostrequested / binpack weight
    w_bal: float,               # balancedallocation weight
    dim_w: torch.Tensor,        # [R] f32 per-resource weights (binpack.weight.<res>)
    bias: Optional[torch.Tensor],  # [N] f32 additive score bias (or None)
    score_out: torch.Tensor,    # [N] f32 out: -inf for infeasible
    cap_out: torch.Tensor,      # [N] i32 out: instances that fit
) -> None:
    avail = alloc - used + extra                              # [N, R]

    fits = (avail + EPS >= req).all(dim=1)
    taint_ok = (taints & ~torch.tensor(tolerated, dtype=torch.int64, device=taints.device)) == 0
    aff_ok = ((planes & require) == require).all(dim=1)
    anti_ok = ((planes & forbid) == 0).all(dim=1)
    feasible = ready & fits & taint_ok & aff_ok & anti_ok

    pos = req > EPS
    per_dim = torch.where(pos, (avail + EPS) / torch.clamp(req, min=EPS),
                          torch.full_like(avail, float(BIG_CAP)))
    cap = per_dim.amin(dim=1).clamp(min=0, max=float(BIG_CAP)).floor().to(torch.int32)
    cap_out.copy_(torch.where(feasible, cap, torch.zeros_like(cap)))

    denom = torch.clamp(alloc, min=EPS)
    frac = torch.clamp((used + req) / denom, max=1.0)         # [N, R]
    wsum = torch.clamp(dim_w.sum(), min=EPS)
    R = alloc.shape[1]
    least = _row_sum((1.0 - frac) * dim_w) / wsum
    most = _row_sum(frac * dim_w) / wsum
    mean = (_row_sum(frac) / R).unsqueeze(1)
    bal = 1.0 - torch.sqrt(_row_sum((frac - mean) ** 2) / R)
    score = w_least * least + w_most * most + w_bal * bal
    if bias is not None:
        score = score + bias
    score_out.copy_(torch.where(feasible & (cap_out > 0), score,
                                torch.full_like(score, NEG_INF)))


def select_commit(
    score: torch.Tensor,        # [N] f32 from score_cap
    cap: torch.Tensor,          # [N] i32
    req: torch.Tensor,          # [R] f32
    ntasks: int,                # class size (instances to place)
    used: torch.Tensor,         # [N, R] f32 — updated in place (staged)
    queue_alloc: torch.Tensor,  # [R] f32 — this queue's allocated row, in place
    queue_limit: torch.Tensor,  # [R] f32 — queue bound (+inf = none)
    log_nodes: torch.Tensor,    # [K] i32 — this class's undo-log slot (K ≥ min(ntasks, N))
    log_counts: torch.Tensor,   # [K] i32
    log_len: torch.Tensor,      # [] i32 — entries written
    placed: torch.Tensor,       # [] i32 — this class's placed count
    job_placed: torch.Tensor,   # [] i32 — accumulator across the job's classes
) -> None:
    """Greedy best-score fill for one task class.

    Sequential-equivalent semantics: repeatedly take the feasible node with
    the highest score (ties → lowest index), place as many instances as its
    capacity and the queue quota allow, move on.  The score is *not*
    recomputed between placements within one class — all instances of a
    class are identical, so the node order is static and the fill equals
    "sort by score desc, take cap each".  (The reference scores per task and
    samples 5 % of nodes — predicate_helper.go:45, scheduler_helper.go:56;
    we score ALL nodes, which strictly improves placement quality.)
    """
    N = score.shape[0]
    log_nodes.zero_()
    log_counts.zero_()

    # queue quota → instance budget under the queue limit
    headroom = queue_limit - queue_alloc                      # [R]
    pos = req > EPS
    per_dim = torch.where(pos, (headroom + EPS) / torch.clamp(req, min=EPS),
                          torch.full_like(headroom, float(BIG_CAP)))
    quota = per_dim.amin().clamp(min=0, max=float(BIG_CAP)).floor()
    budget = torch.minimum(torch.tensor(float(ntasks), device=score.device), quota)

    if N == 0:
        log_len.zero_(); placed.zero_()
        return
    order = torch.argsort(score, descending=True, stable=True)
    sorted_cap = torch.where(score[order] > NEG_INF, cap[order],
                             torch.zeros_like(cap)).to(torch.int64)
    csum = torch.cumsum(sorted_cap, dim=0)
    take = torch.clamp(sorted_cap - torch.clamp(csum - budget.to(torch.int64), min=0), min=0)
    total = torch.minimum(csum[-1], budget.to(torch.int64))

    k = log_nodes.shape[0]
    # compact the first k nonzero entries into the log slot
    # (torch.nonzero syncs on GPU — acceptable: the GPU path runs the HIP
    #  kernel, which compacts in-kernel; this reference is the CPU oracle)
    idx = torch.nonzero(take > 0, as_tuple=False).flatten()[:k]
    cnt = take[idx].to(torch.int32)
    m = int(idx.shape[0])
    log_nodes[:m] = order[idx].to(torch.int32)
    log_counts[:m] = cnt
    log_len.fill_(m)

    used.index_add_(0, order[idx].to(torch.long),
                    cnt.to(torch.float32).unsqueeze(1) * req.unsqueeze(0))
    queue_alloc += total.to(torch.float32) * req
    placed.copy_(total.to(torch.int32))
    job_placed.add_(total.to(torch.int32))


def finalize_job(
    job_placed: torch.Tensor,   # [] i32 placed across the job's classes
    occupied: int,              # tasks already holding resources (host-known at cycle start)
    min_available: int,         # gang minimum
    class_placed: torch.Tensor,  # [nc] i32 per-class placed counts
    class_min: torch.Tensor,     # [nc] i32 per-class minimums (role mins)
    flag: torch.Tensor,         # [] u8 out: 1 = commit, 0 = revert
) -> None:
    """Gang readiness (session_plugins.go:483 JobReady AND-aggregation)."""
    ok = (job_placed + occupied >= min_available)
    ok = ok & (class_placed >= class_min).all()
    flag.copy_(ok.to(torch.uint8))


def cond_revert(
    flag: torch.Tensor,         # [] u8 — 1 = keep, 0 = revert
    log_nodes: torch.Tensor,    # [K] i32
    log_counts: torch.Tensor,   # [K] i32 — zeroed on revert
    log_len: torch.Tensor,      # [] i32
    req: torch.Tensor,          # [R] f32
    used: torch.Tensor,         # [N, R] f32 in place
    queue_alloc: torch.Tensor,  # [R] f32 in place
    placed: torch.Tensor,       # [] i32 — zeroed on revert
    job_placed: torch.Tensor,   # [] i32 — decremented on revert
) -> None:
    """Undo one class's staged placement iff the gang failed
    (statement.go:375 Discard, reverse-order undo)."""
    do = (flag == 0).to(torch.float32)                        # 0.0 keep / 1.0 revert
    cnt = log_counts.to(torch.float32) * do
    arange = torch.arange(log_counts.shape[0], device=log_counts.device)
    valid = arange < log_len.to(arange.dtype)
    cnt = cnt * valid.to(torch.float32)
    used.index_add_(0, log_nodes.to(torch.long),
                    -cnt.unsqueeze(1) * req.unsqueeze(0))
    queue_alloc -= cnt.sum() * req
    job_placed.add_((-placed * (flag == 0).to(torch.int32)))
    placed.mul_((flag != 0).to(torch.int32))
    log_counts.mul_((flag != 0).to(torch.int32))


def spread_select_commit(
    score: torch.Tensor,        # [N] f32 from score_cap
    cap: torch.Tensor,          # [N] i32
    req: torch.Tensor,          # [R] f32
    ntasks: int,
    used: torch.Tensor,         # [N, R] f32 — updated in place (staged)
    queue_alloc: torch.Tensor,  # [R] f32 in place
    queue_limit: torch.Tensor,  # [R] f32
    log_nodes: torch.Tensor,    # [K] i32 (K ≥ min(ntasks, N))
    log_counts: torch.Tensor,   # [K] i32
    log_len: torch.Tensor,      # [] i32
    placed: torch.Tensor,       # [] i32
    job_placed: torch.Tensor,   # [] i32
    dom_of: torch.Tensor,       # [N] i32 node → spread domain (-1: unlabeled)
    dom_count: torch.Tensor,    # [D] i32 group members per domain, in place
    max_skew: int,              # ≥ 1
) -> None:
    """Per-placement topology-spread fill for one task class (k8s
    podtopologyspread DoNotSchedule, evaluated before EVERY instance).

    A plain sequential loop on purpose — this is the source of truth the
    HIP ``spread_select_kernel`` must reproduce bit for bit.  Scores are
    static within the class (as in ``select_commit``); what changes after
    each placement is eligibility: a node may take an instance only while
    ``dom_count[its domain] + 1 - min(dom_count) <= max_skew``.  The
    minimum ranges over ALL domains, also those without a feasible node.
    Counts only change on placement, so a state with no eligible node is
    final and the loop stops there.

    The log carries one (node, count) entry per node in order of first
    placement; ``used`` takes one ``float(count) * req`` per entry.
    """
    if max_skew < 1:
        raise ValueError("max_skew must be >= 1")
    N = score.shape[0]
    log_nodes.zero_()
    log_counts.zero_()

    headroom = queue_limit - queue_alloc
    pos = req > EPS
    per_dim = torch.where(pos, (headroom + EPS) / torch.clamp(req, min=EPS),
                          torch.full_like(headroom, float(BIG_CAP)))
    quota = int(per_dim.amin().clamp(min=0, max=float(BIG_CAP)).floor())
    budget = min(int(ntasks), quota)

    sc = score.tolist()
    dom = dom_of.tolist()
    cnt = dom_count.tolist()
    rem = [int(c) if (s > NEG_INF and d >= 0) else 0
           for s, c, d in zip(sc, cap.tolist(), dom)]
    slot = {}                   # node → log entry
    nodes: list = []
    counts: list = []
    total = 0
    while total < budget:
        m = min(cnt)
        best = -1
        for n in range(N):
            if rem[n] > 0 and cnt[dom[n]] + 1 - m <= max_skew \
                    and (best < 0 or sc[n] > sc[best]):
                best = n
        if best < 0:
            break
        rem[best] -= 1
        cnt[dom[best]] += 1
        total += 1
        e = slot.get(best)
        if e is None:
            slot[best] = len(nodes)
            nodes.append(best)
            counts.append(1)
        else:
            counts[e] += 1

    m = len(nodes)
    assert m <= log_nodes.shape[0], "undo-log slot too small"
    dev = score.device
    idx = torch.tensor(nodes, dtype=torch.long, device=dev)
    c32 = torch.tensor(counts, dtype=torch.int32, device=dev)
    log_nodes[:m] = idx.to(torch.int32)
    log_counts[:m] = c32
    log_len.fill_(m)
    dom_count.copy_(torch.tensor(cnt, dtype=torch.int32, device=dev))
    used.index_add_(0, idx, c32.to(torch.float32).unsqueeze(1)
                    * req.unsqueeze(0))
    queue_alloc += torch.tensor(float(total), device=dev) * req
    placed.fill_(total)
    job_placed.add_(total)


def spread_revert(
    flag: torch.Tensor, log_nodes: torch.Tensor, log_counts: torch.Tensor,
    log_len: torch.Tensor, req: torch.Tensor, used: torch.Tensor,
    queue_alloc: torch.Tensor, placed: torch.Tensor,
    job_placed: torch.Tensor,
    dom_of: torch.Tensor,       # [N] i32
    dom_count: torch.Tensor,    # [D] i32 in place
) -> None:
    """``cond_revert`` for a spread class: additionally gives the logged
    placements back to the group's per-domain counts."""
    if int(flag) == 0:
        n = int(log_len)
        nodes = log_nodes[:n].to(torch.long)
        doms = dom_of[nodes].to(torch.long)
        dom_count.index_add_(0, doms, -log_counts[:n])
    cond_revert(flag, log_nodes, log_counts, log_len, req, used,
                queue_alloc, placed, job_placed)


AFFINITY = 1                    # domain-rule modes of affinity_select_commit
ANTI_AFFINITY = 2


def affinity_select_commit(
    score: torch.Tensor,        # [N] f32 from score_cap
    cap: torch.Tensor,          # [N] i32
    req: torch.Tensor,          # [R] f32
    ntasks: int,
    used: torch.Tensor,         # [N, R] f32 — updated in place (staged)
    queue_alloc: torch.Tensor,  # [R] f32 in place
    queue_limit: torch.Tensor,  # [R] f32
    log_nodes: torch.Tensor,    # [K] i32 (K ≥ min(ntasks, N))
    log_counts: torch.Tensor,   # [K] i32
    log_len: torch.Tensor,      # [] i32
    placed: torch.Tensor,       # [] i32
    job_placed: torch.Tensor,   # [] i32
    dom_of: torch.Tensor,       # [N] i32 node → domain (-1: unlabeled)
    dom_count: torch.Tensor,    # [D] i32 group members per domain, in place
    mode: int,                  # AFFINITY or ANTI_AFFINITY
) -> None:
    """Per-placement inter-pod (anti-)affinity fill for one task class (k8s
    interpodaffinity filter, evaluated before EVERY instance).

    A plain sequential loop on purpose — the source of truth for the HIP
    composition ``domain_mask`` → ``select_commit`` → ``domain_count_add``.
    Scores are static within the class; what moves is eligibility:

    * ``AFFINITY``: while no domain holds a member, every feasible labelled
      node is eligible and the first placement anchors its domain;
      afterwards only nodes of domains with ``count > 0``.
    * ``ANTI_AFFINITY``: only nodes of domains with ``count == 0``; a
      placement closes its domain.

    Unlabelled nodes (``dom_of < 0``) never take an instance.  Log, ``used``
    and the counters follow ``spread_select_commit``.
    """
    if mode not in (AFFINITY, ANTI_AFFINITY):
        raise ValueError("mode must be AFFINITY (1) or ANTI_AFFINITY (2)")
    N = score.shape[0]
    log_nodes.zero_()
    log_counts.zero_()

    headroom = queue_limit - queue_alloc
    pos = req > EPS
    per_dim = torch.where(pos, (headroom + EPS) / torch.clamp(req, min=EPS),
                          torch.full_like(headroom, float(BIG_CAP)))
    quota = int(per_dim.amin().clamp(min=0, max=float(BIG_CAP)).floor())
    budget = min(int(ntasks), quota)

    sc = score.tolist()
    dom = dom_of.tolist()
    cnt = dom_count.tolist()
    rem = [int(c) if (s > NEG_INF and d >= 0) else 0
           for s, c, d in zip(sc, cap.tolist(), dom)]
    hosting = sum(1 for c in cnt if c > 0)
    slot = {}                   # node → log entry
    nodes: list = []
    counts: list = []
    total = 0
    while total < budget:
        best = -1
        for n in range(N):
            if rem[n] <= 0:
                continue
            c = cnt[dom[n]]
            if mode == AFFINITY:
                ok = hosting == 0 or c > 0
            else:
                ok = c == 0
            if ok and (best < 0 or sc[n] > sc[best]):
                best = n
        if best < 0:
            break
        rem[best] -= 1
        if cnt[dom[best]] == 0:
            hosting += 1
        cnt[dom[best]] += 1
        total += 1
        e = slot.get(best)
        if e is None:
            slot[best] = len(nodes)
            nodes.append(best)
            counts.append(1)
        else:
            counts[e] += 1

    m = len(nodes)
    assert m <= log_nodes.shape[0], "undo-log slot too small"
    dev = score.device
    idx = torch.tensor(nodes, dtype=torch.long, device=dev)
    c32 = torch.tensor(counts, dtype=torch.int32, device=dev)
    log_nodes[:m] = idx.to(torch.int32)
    log_counts[:m] = c32
    log_len.fill_(m)
    dom_count.copy_(torch.tensor(cnt, dtype=torch.int32, device=dev))
    used.index_add_(0, idx, c32.to(torch.float32).unsqueeze(1)
                    * req.unsqueeze(0))
    queue_alloc += torch.tensor(float(total), device=dev) * req
    placed.fill_(total)
    job_placed.add_(total)


def drf_share(job_alloc: torch.Tensor, total: torch.Tensor) -> torch.Tensor:
    """Dominant share per job: max_r alloc/total (drf.go calculateShare).

    job_alloc [J, R], total [R] → [J] f64."""
    t = torch.clamp(total.to(torch.float64), min=1.0)
    return (job_alloc.to(torch.float64) / t).amax(dim=1)


def waterfill(
    weight: torch.Tensor,       # [Q] f32 queue weights
    request: torch.Tensor,      # [Q, R] f32 total demand per queue
    guarantee: torch.Tensor,    # [Q, R] f32 floor
    capability: torch.Tensor,   # [Q, R] f32 ceiling (+inf = none)
    total: torch.Tensor,        # [R] f32 cluster total
    iters: int = 16,
) -> torch.Tensor:
    """Proportion-plugin deserved computation (proportion.go:90-260).

    Iterative weighted water-filling: each round splits the remaining pool
    by weight among unsatisfied queues, capping at min(max(request,
    guarantee), capability); guarantees are granted first.  float64
    accumulators for reproducibility (SURVEY §7 hard-parts note)."""
    w = weight.to(torch.float64)
    demand = torch.minimum(request.to(torch.float64), capability.to(torch.float64))
    demand = torch.maximum(demand, guarantee.to(torch.float64))
    deserved = torch.minimum(guarantee.to(torch.float64),
                             capability.to(torch.float64)).clone()
    remaining = torch.clamp(total.to(torch.float64) - deserved.sum(dim=0), min=0.0)

    for _ in range(iters):
        unsat = deserved + 1e-9 < demand                      # [Q, R]
        wsum = (w.unsqueeze(1) * unsat).sum(dim=0)            # [R]
        give = torch.where(wsum > 0, remaining / torch.clamp(wsum, min=1e-12),
                           torch.zeros_like(remaining))
        inc = torch.minimum(w.unsqueeze(1) * give.unsqueeze(0) * unsat,
                            demand - deserved)
        inc = torch.clamp(inc, min=0.0)
        deserved = deserved + inc
        remaining = torch.clamp(remaining - inc.sum(dim=0), min=0.0)
    return deserved.to(torch.float32)
