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
* ``rescore_select_commit`` — K2 select that re-scores the chosen node after
  every placement (reverts: ``cond_revert``).
* ``hypernode_mask`` — network-topology domain choice from the live cap:
  a mask before ``select_commit`` (reverts: ``cond_revert``).
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
    ``rescore_select_commit`` is the exact variant that does re-score the
    chosen node after every placement (nodeorder ``exact: true``).
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


SPREAD_MAX_RULES = 4            # rules of one spread_multi_select_commit
# largest sum of D over them on the device (``SM_LDS_DOMAINS`` of
# scheduler_kernels.hip: 32 KB of eligibility bits; checked on load)
SPREAD_MULTI_LDS_DOMAINS = 1 << 18


def spread_multi_select_commit(
    score: torch.Tensor, cap: torch.Tensor, req: torch.Tensor, ntasks: int,
    used: torch.Tensor, queue_alloc: torch.Tensor, queue_limit: torch.Tensor,
    log_nodes: torch.Tensor, log_counts: torch.Tensor, log_len: torch.Tensor,
    placed: torch.Tensor, job_placed: torch.Tensor,
    rules,                      # 1..4 x (dom_of [N] i32, dom_count [D_r] i32
                                #         in place, max_skew >= 1)
) -> None:
    """``spread_select_commit`` under several topology-spread constraints
    at once (zone AND hostname): node ``n`` may take an instance only
    while, for EVERY rule ``r``, ``dom_r[n] >= 0`` and
    ``cnt_r[dom_r[n]] + 1 - min(cnt_r) <= skew_r`` — each minimum over all
    ``D_r`` domains of its rule.  A placement joins the node's domain in
    every rule.  Everything else (queue budget, log, ``used``, the stop at
    the first state without an eligible node) is ``spread_select_commit``,
    which this equals with one rule.

    A plain sequential loop — the source of truth of the HIP
    ``spread_multi_select_kernel``."""
    rules = list(rules)
    if not 1 <= len(rules) <= SPREAD_MAX_RULES:
        raise ValueError(f"1 to {SPREAD_MAX_RULES} spread rules per class")
    if any(int(skew) < 1 for _, _, skew in rules):
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
    doms = [d.tolist() for d, _, _ in rules]
    cnts = [c.tolist() for _, c, _ in rules]
    skews = [int(s) for _, _, s in rules]
    rem = [int(c) if s > NEG_INF and all(d[n] >= 0 for d in doms) else 0
           for n, (s, c) in enumerate(zip(sc, cap.tolist()))]
    slot = {}                   # node → log entry
    nodes: list = []
    counts: list = []
    total = 0
    while total < budget:
        lows = [min(c) for c in cnts]
        best = -1
        for n in range(N):
            if rem[n] > 0 and (best < 0 or sc[n] > sc[best]) and all(
                    c[d[n]] + 1 - m <= k
                    for c, d, m, k in zip(cnts, doms, lows, skews)):
                best = n
        if best < 0:
            break
        rem[best] -= 1
        for c, d in zip(cnts, doms):
            c[d[best]] += 1
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
    for (_, dom_count, _), c in zip(rules, cnts):
        dom_count.copy_(torch.tensor(c, dtype=torch.int32, device=dev))
    used.index_add_(0, idx, c32.to(torch.float32).unsqueeze(1)
                    * req.unsqueeze(0))
    queue_alloc += torch.tensor(float(total), device=dev) * req
    placed.fill_(total)
    job_placed.add_(total)


def spread_multi_revert(
    flag: torch.Tensor, log_nodes: torch.Tensor, log_counts: torch.Tensor,
    log_len: torch.Tensor, req: torch.Tensor, used: torch.Tensor,
    queue_alloc: torch.Tensor, placed: torch.Tensor,
    job_placed: torch.Tensor,
    rules,                      # as in spread_multi_select_commit
) -> None:
    """``cond_revert`` for a class with several spread rules: the logged
    placements go back to the counts of every rule first."""
    if int(flag) == 0:
        n = int(log_len)
        nodes = log_nodes[:n].to(torch.long)
        for dom_of, dom_count, _ in rules:
            dom_count.index_add_(0, dom_of[nodes].to(torch.long),
                                 -log_counts[:n])
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


def fma_f32(k: int, req: torch.Tensor, acc: torch.Tensor) -> torch.Tensor:
    """``fma(float(k), req, acc)`` in f32 with ONE rounding, elementwise —
    what ``acc_add`` of the kernels computes.  ``k * req`` is exact in f64;
    the f64 sum is rounded to odd (TwoSum gives its error), after which the
    rounding to f32 is the rounding of the exact value."""
    import numpy as np
    a = acc.detach().cpu().double().numpy()
    p = float(k) * req.detach().cpu().double().numpy()
    s = a + p
    bb = s - a
    err = (a - (s - bb)) + (p - bb)             # exact: a + p == s + err
    toward = np.nextafter(s, np.where(err > 0, np.inf, -np.inf))
    is_odd = (s.view(np.int64) & 1) == 1
    s = np.where((err == 0) | is_odd | ~np.isfinite(s), s, toward)
    return torch.from_numpy(s.astype(np.float32)).to(acc.device)


def rescore_select_commit(
    alloc: torch.Tensor,        # [N, R] f32 — the inputs of score_cap ...
    used: torch.Tensor,         # [N, R] f32 — updated in place (staged)
    extra: torch.Tensor,        # [N, R] f32
    ready: torch.Tensor, taints: torch.Tensor, planes: torch.Tensor,
    req: torch.Tensor, tolerated: int, require: torch.Tensor,
    forbid: torch.Tensor, w_least: float, w_most: float, w_bal: float,
    dim_w: torch.Tensor, bias: Optional[torch.Tensor],
    score: torch.Tensor,        # [N] f32 from score_cap (and any mask)
    cap: torch.Tensor,          # [N] i32 likewise
    ntasks: int,
    queue_alloc: torch.Tensor,  # [R] f32 in place
    queue_limit: torch.Tensor,  # [R] f32
    log_nodes: torch.Tensor,    # [K] i32 (K ≥ min(ntasks, N))
    log_counts: torch.Tensor,   # [K] i32
    log_len: torch.Tensor,      # [] i32
    placed: torch.Tensor,       # [] i32
    job_placed: torch.Tensor,   # [] i32
    fuse_min: int = -1,         # ≥ 0: single-class gang minimum
    score_fn=None,              # (node, k) -> float, replaces the formula
) -> None:
    """``select_commit`` with the chosen node re-scored after EVERY
    placement (the per-task scoring of the reference's nodeorder).

    A plain sequential loop on purpose — the source of truth the HIP
    ``rescore_select_kernel`` must reproduce bit for bit.  It runs where
    ``select_commit`` would, on ``score`` / ``cap`` as ``score_cap`` and any
    cap or mask kernel left them.  ``rem[n] = cap[n]`` where
    ``score[n] > -inf``, else 0.  Each step takes the node with the highest
    score among those with ``rem > 0`` (ties to the lower index), places
    ONE instance and re-scores that node alone: ``-inf`` once ``rem`` is 0,
    else the ``score_cap`` formula (same operations, bias included) on
    ``used_k = fma(float(k), req, used0)`` for its ``k`` staged instances —
    the value the commit writes for a count of ``k``, one rounding — and
    ``-inf`` when the formula's own fit test fails there.  The loop stops
    at the budget ``min(ntasks, queue quota)``, when a new node would need
    a log entry past ``K``, or when no node is left.

    Log, ``used`` and counters follow ``spread_select_commit``: one
    ``(node, count)`` entry per node in order of first placement, one
    ``float(count) * req`` per entry.  A gang that misses ``fuse_min``
    commits nothing and keeps its nodes with zeroed counts.
    """
    N = score.shape[0]
    K = log_nodes.shape[0]
    log_nodes.zero_()
    log_counts.zero_()

    headroom = queue_limit - queue_alloc
    pos = req > EPS
    per_dim = torch.where(pos, (headroom + EPS) / torch.clamp(req, min=EPS),
                          torch.full_like(headroom, float(BIG_CAP)))
    quota = int(per_dim.amin().clamp(min=0, max=float(BIG_CAP)).floor())
    budget = min(int(ntasks), quota)

    one_s = torch.empty(1, dtype=torch.float32, device=score.device)
    one_c = torch.empty(1, dtype=torch.int32, device=score.device)

    def formula(n: int, k: int) -> float:
        # Readiness, taints and label planes do not move with usage and
        # are already in ``score``: only the fit test is asked again.
        row = slice(n, n + 1)
        used_k = fma_f32(k, req, used[row])
        score_cap(alloc[row], used_k, extra[row], torch.ones_like(ready[row]),
                  torch.zeros_like(taints[row]), planes[row], req, 0,
                  torch.zeros_like(require), torch.zeros_like(forbid),
                  w_least, w_most, w_bal, dim_w,
                  None if bias is None else bias[row], one_s, one_c)
        return float(one_s)

    rescore = formula if score_fn is None else score_fn
    import heapq
    rem = [int(c) if s > NEG_INF else 0
           for s, c in zip(score.tolist(), cap.tolist())]
    # every node that can still take an instance, once, under its live
    # score: the smallest (-score, index) is the highest score, ties to the
    # lower index (-0.0 and 0.0 compare equal)
    heap = [(-s, n) for n, s in enumerate(score.tolist()) if rem[n] > 0]
    heapq.heapify(heap)
    slot = {}                   # node → log entry
    nodes: list = []
    counts: list = []
    total = 0
    while total < budget and heap:
        best = heap[0][1]
        e = slot.get(best)
        if e is None:
            if len(nodes) >= K:
                break
            e = slot[best] = len(nodes)
            nodes.append(best)
            counts.append(0)
        heapq.heappop(heap)
        counts[e] += 1
        rem[best] -= 1
        total += 1
        s = rescore(best, counts[e]) if rem[best] > 0 else NEG_INF
        if s > NEG_INF:
            heapq.heappush(heap, (-s, best))

    m = len(nodes)
    dev = score.device
    idx = torch.tensor(nodes, dtype=torch.long, device=dev)
    c32 = torch.tensor(counts, dtype=torch.int32, device=dev)
    log_nodes[:m] = idx.to(torch.int32)
    log_len.fill_(m)
    if fuse_min >= 0 and total < fuse_min:
        placed.fill_(0)
        return
    log_counts[:m] = c32
    used.index_add_(0, idx, c32.to(torch.float32).unsqueeze(1)
                    * req.unsqueeze(0))
    queue_alloc += torch.tensor(float(total), device=dev) * req
    placed.fill_(total)
    job_placed.add_(total)


def spread_rescore_select_commit(
    alloc: torch.Tensor, used: torch.Tensor, extra: torch.Tensor,
    ready: torch.Tensor, taints: torch.Tensor, planes: torch.Tensor,
    req: torch.Tensor, tolerated: int, require: torch.Tensor,
    forbid: torch.Tensor, w_least: float, w_most: float, w_bal: float,
    dim_w: torch.Tensor, bias: Optional[torch.Tensor],
    score: torch.Tensor, cap: torch.Tensor, ntasks: int,
    queue_alloc: torch.Tensor, queue_limit: torch.Tensor,
    log_nodes: torch.Tensor, log_counts: torch.Tensor, log_len: torch.Tensor,
    placed: torch.Tensor, job_placed: torch.Tensor,
    rules,                      # as in spread_multi_select_commit
    fuse_min: int = -1, score_fn=None,
) -> None:
    """``rescore_select_commit`` under the 1 to 4 spread rules of
    ``spread_multi_select_commit`` (topologyspread and nodeorder both exact):
    replicas spread over the domains AND take the best node by its live
    score inside them.

    A plain sequential loop — the source of truth of the HIP
    ``spread_rescore_select_kernel``.  Per instance: among the nodes with
    ``score > -inf`` whose domain is open under EVERY rule
    (``cnt_r[d] + 1 - min(cnt_r) <= skew_r``, the minimum over all ``D_r``
    domains) the best score wins, ties to the lower index; it takes ONE
    instance; its domain's count rises under every rule; and it alone is
    scored again as ``rescore_select_commit`` does it (``score_fn`` hook
    included): the formula on ``fma_f32(k, req, used)`` for its ``k`` staged
    instances, ``-inf`` once its capacity is used up or the fit test fails.
    The loop stops at the budget, at a new node past the log's ``K`` entries,
    or at the first state without an eligible node.

    One ``(node, count)`` log entry per node in order of first placement, one
    ``count * req`` per entry into ``used`` after the loop.  A gang that
    misses ``fuse_min`` gives every count back and writes nothing else: the
    log keeps its nodes with zeroed counts."""
    rules = list(rules)
    if not 1 <= len(rules) <= SPREAD_MAX_RULES:
        raise ValueError(f"1 to {SPREAD_MAX_RULES} spread rules per class")
    if any(int(skew) < 1 for _, _, skew in rules):
        raise ValueError("max_skew must be >= 1")
    N = score.shape[0]
    K = log_nodes.shape[0]
    log_nodes.zero_()
    log_counts.zero_()

    headroom = queue_limit - queue_alloc
    pos = req > EPS
    per_dim = torch.where(pos, (headroom + EPS) / torch.clamp(req, min=EPS),
                          torch.full_like(headroom, float(BIG_CAP)))
    quota = int(per_dim.amin().clamp(min=0, max=float(BIG_CAP)).floor())
    budget = min(int(ntasks), quota)

    one_s = torch.empty(1, dtype=torch.float32, device=score.device)
    one_c = torch.empty(1, dtype=torch.int32, device=score.device)

    def formula(n: int, k: int) -> float:
        row = slice(n, n + 1)
        score_cap(alloc[row], fma_f32(k, req, used[row]), extra[row],
                  torch.ones_like(ready[row]), torch.zeros_like(taints[row]),
                  planes[row], req, 0, torch.zeros_like(require),
                  torch.zeros_like(forbid), w_least, w_most, w_bal, dim_w,
                  None if bias is None else bias[row], one_s, one_c)
        return float(one_s)

    rescore = formula if score_fn is None else score_fn
    sc = score.tolist()
    doms = [d.tolist() for d, _, _ in rules]
    cnts = [c.tolist() for _, c, _ in rules]
    before = [list(c) for c in cnts]
    skews = [int(s) for _, _, s in rules]
    rem = [int(c) if s > NEG_INF and all(d[n] >= 0 for d in doms) else 0
           for n, (s, c) in enumerate(zip(sc, cap.tolist()))]
    slot = {}                   # node → log entry
    nodes: list = []
    counts: list = []
    total = 0
    while total < budget:
        lows = [min(c) for c in cnts]
        best = -1
        for n in range(N):
            if rem[n] > 0 and (best < 0 or sc[n] > sc[best]) and all(
                    c[d[n]] + 1 - m <= k
                    for c, d, m, k in zip(cnts, doms, lows, skews)):
                best = n
        if best < 0:
            break
        e = slot.get(best)
        if e is None:
            if len(nodes) >= K:
                break
            e = slot[best] = len(nodes)
            nodes.append(best)
            counts.append(0)
        counts[e] += 1
        rem[best] -= 1
        total += 1
        for c, d in zip(cnts, doms):
            c[d[best]] += 1
        s = rescore(best, counts[e]) if rem[best] > 0 else NEG_INF
        sc[best] = s
        if not s > NEG_INF:
            rem[best] = 0

    m = len(nodes)
    dev = score.device
    idx = torch.tensor(nodes, dtype=torch.long, device=dev)
    c32 = torch.tensor(counts, dtype=torch.int32, device=dev)
    log_nodes[:m] = idx.to(torch.int32)
    log_len.fill_(m)
    discard = fuse_min >= 0 and total < fuse_min
    for (_, dom_count, _), c in zip(rules, before if discard else cnts):
        dom_count.copy_(torch.tensor(c, dtype=torch.int32, device=dev))
    if discard:
        placed.fill_(0)
        return
    log_counts[:m] = c32
    used.index_add_(0, idx, c32.to(torch.float32).unsqueeze(1)
                    * req.unsqueeze(0))
    queue_alloc += torch.tensor(float(total), device=dev) * req
    placed.fill_(total)
    job_placed.add_(total)


# largest sum of D over the SOFT rules of one spread_soft_select_commit on the
# device (``SS_LDS_DOMAINS`` of scheduler_kernels.hip: 28 KB of int32 counts
# in LDS; checked on load)
SPREAD_SOFT_LDS_DOMAINS = 7168
# maxSkew carried by a soft rule where a hard one is expected: never binds,
# and count + 1 - min cannot overflow int32
SPREAD_SOFT_SKEW = 1 << 30


def spread_soft_select_commit(
    alloc: torch.Tensor, used: torch.Tensor, extra: torch.Tensor,
    ready: torch.Tensor, taints: torch.Tensor, planes: torch.Tensor,
    req: torch.Tensor, tolerated: int, require: torch.Tensor,
    forbid: torch.Tensor, w_least: float, w_most: float, w_bal: float,
    dim_w: torch.Tensor, bias: Optional[torch.Tensor],
    score: torch.Tensor, cap: torch.Tensor, ntasks: int,
    queue_alloc: torch.Tensor, queue_limit: torch.Tensor,
    log_nodes: torch.Tensor, log_counts: torch.Tensor, log_len: torch.Tensor,
    placed: torch.Tensor, job_placed: torch.Tensor,
    rules,                      # 1..4 x (dom_of [N] i32, dom_count [D_r] i32
                                #         in place, max_skew >= 1, tw f32)
    rescore: bool, fuse_min: int = -1, score_fn=None,
) -> None:
    """``spread_rescore_select_commit`` with ``whenUnsatisfiable:
    ScheduleAnyway`` rules among its 1 to 4: a rule with ``tw == 0`` is hard
    and filters on its ``maxSkew`` as there; a rule with ``tw != 0`` is soft,
    never filters on counts (a node without its label is still out) and
    instead costs ``tw`` per member already in the node's domain.

    A plain sequential loop — the source of truth of the HIP
    ``spread_soft_select_kernel``.  Before every single placement each
    remaining node has ``pen = fma(tw_R, float(cnt_R[d_R]), ... fma(tw_1,
    float(cnt_1[d_1]), 0.0))`` over the soft rules in rule order, one f32 fma
    each, and ``total = score - pen``, one f32 subtraction.  Among the nodes
    with ``score > -inf``, capacity left and every hard rule's domain open,
    the highest ``total`` wins, ties to the lower index (``-0.0`` ties with
    ``0.0``).  It takes ONE instance and its domain's count rises under every
    rule.  With ``rescore`` its score is then recomputed as
    ``spread_rescore_select_commit`` does; without, it stays until the
    node's capacity is used up.  Log, budget, ``used``, counters and the
    ``fuse_min`` discard (every rule's counts come back) are
    ``spread_rescore_select_commit``'s."""
    import numpy as np
    rules = list(rules)
    if not 1 <= len(rules) <= SPREAD_MAX_RULES:
        raise ValueError(f"1 to {SPREAD_MAX_RULES} spread rules per class")
    if any(int(skew) < 1 for _, _, skew, _ in rules):
        raise ValueError("max_skew must be >= 1")
    N = score.shape[0]
    K = log_nodes.shape[0]
    log_nodes.zero_()
    log_counts.zero_()

    headroom = queue_limit - queue_alloc
    pos = req > EPS
    per_dim = torch.where(pos, (headroom + EPS) / torch.clamp(req, min=EPS),
                          torch.full_like(headroom, float(BIG_CAP)))
    quota = int(per_dim.amin().clamp(min=0, max=float(BIG_CAP)).floor())
    budget = min(int(ntasks), quota)

    one_s = torch.empty(1, dtype=torch.float32, device=score.device)
    one_c = torch.empty(1, dtype=torch.int32, device=score.device)

    def formula(n: int, k: int) -> float:
        row = slice(n, n + 1)
        score_cap(alloc[row], fma_f32(k, req, used[row]), extra[row],
                  torch.ones_like(ready[row]), torch.zeros_like(taints[row]),
                  planes[row], req, 0, torch.zeros_like(require),
                  torch.zeros_like(forbid), w_least, w_most, w_bal, dim_w,
                  None if bias is None else bias[row], one_s, one_c)
        return float(one_s)

    again = formula if score_fn is None else score_fn
    sc = score.detach().cpu().numpy().astype(np.float32)
    doms = [d.detach().cpu().numpy().astype(np.int64) for d, _, _, _ in rules]
    cnts = [c.detach().cpu().numpy().astype(np.int64) for _, c, _, _ in rules]
    before = [c.copy() for c in cnts]
    skews = [int(s) for _, _, s, _ in rules]
    tws = [float(np.float32(t)) for _, _, _, t in rules]
    rem = cap.detach().cpu().numpy().astype(np.int64)
    rem[~(sc > NEG_INF)] = 0
    for d in doms:
        rem[d < 0] = 0
    slot = {}                   # node → log entry
    nodes: list = []
    counts: list = []
    total = 0
    while total < budget:
        ok = rem > 0
        pen = torch.zeros(N, dtype=torch.float32)
        for c, d, k, tw in zip(cnts, doms, skews, tws):
            here = c[np.where(ok, d, 0)]
            if tw == 0:
                ok &= here + 1 - c.min() <= k
            else:
                pen = fma_f32(tw, torch.from_numpy(
                    here.astype(np.float32)), pen)
        live = np.flatnonzero(ok)
        if live.size == 0:
            break
        tot = (sc - pen.numpy())[live]          # f32 - f32, one rounding
        best = int(live[np.argmax(tot)])        # first maximum: lower index
        e = slot.get(best)
        if e is None:
            if len(nodes) >= K:
                break
            e = slot[best] = len(nodes)
            nodes.append(best)
            counts.append(0)
        counts[e] += 1
        rem[best] -= 1
        total += 1
        for c, d in zip(cnts, doms):
            c[d[best]] += 1
        if rem[best] <= 0:
            sc[best] = NEG_INF
        elif rescore:
            sc[best] = again(best, counts[e])
            if not sc[best] > NEG_INF:
                rem[best] = 0

    m = len(nodes)
    dev = score.device
    idx = torch.tensor(nodes, dtype=torch.long, device=dev)
    c32 = torch.tensor(counts, dtype=torch.int32, device=dev)
    log_nodes[:m] = idx.to(torch.int32)
    log_len.fill_(m)
    discard = fuse_min >= 0 and total < fuse_min
    for (_, dom_count, _, _), c in zip(rules, before if discard else cnts):
        dom_count.copy_(torch.from_numpy(c.astype(np.int32)).to(dev))
    if discard:
        placed.fill_(0)
        return
    log_counts[:m] = c32
    used.index_add_(0, idx, c32.to(torch.float32).unsqueeze(1)
                    * req.unsqueeze(0))
    queue_alloc += torch.tensor(float(total), device=dev) * req
    placed.fill_(total)
    job_placed.add_(total)


def domain_mask(score: torch.Tensor, cap: torch.Tensor,
                dom_of: torch.Tensor, dom_count: torch.Tensor,
                mode: int) -> None:
    """The static mask the inter-pod rules collapse into (modes 1 and 2 of
    the HIP ``domain_mask``): masked nodes get ``score = -inf``,
    ``cap = 0``.  ``AFFINITY`` keeps the nodes of hosting domains, or, with
    none, the domain of the best placeable node; ``ANTI_AFFINITY`` keeps
    the best node of each empty domain with ``cap = 1``.  Followed by
    ``select_commit`` and the count update it equals
    ``affinity_select_commit``; a re-scoring class runs
    ``rescore_select_commit`` behind it instead."""
    if mode not in (AFFINITY, ANTI_AFFINITY):
        raise ValueError("mode must be AFFINITY (1) or ANTI_AFFINITY (2)")
    D = dom_count.shape[0]
    sc, cp = score.tolist(), cap.tolist()
    dom, cnt = dom_of.tolist(), dom_count.tolist()
    ok = [0 <= d < D and c > 0 and s > NEG_INF
          for s, c, d in zip(sc, cp, dom)]
    heads = {}                  # domain → its best node
    for n in range(len(sc)):
        if ok[n] and (dom[n] not in heads or sc[n] > sc[heads[dom[n]]]):
            heads[dom[n]] = n
    if mode == AFFINITY:
        hosting = any(c > 0 for c in cnt)
        anchor = -1
        if not hosting and heads:
            anchor = dom[max(heads.values(), key=lambda n: (sc[n], -n))]
        keep = [ok[n] and (cnt[dom[n]] > 0 or dom[n] == anchor)
                for n in range(len(sc))]
    else:
        keep = [ok[n] and cnt[dom[n]] == 0 and heads[dom[n]] == n
                for n in range(len(sc))]
    out = ~torch.tensor(keep, dtype=torch.bool, device=score.device)
    score[out] = NEG_INF
    cap[out] = 0
    if mode == ANTI_AFFINITY:
        cap[~out] = 1


HYPERNODE = 3                   # domain-rule mode of hypernode_mask
HN_TAB_HEAD = 5                 # T, need, pin_lo, pin_hi, soft


def hypernode_table(tiers, need: int, n_leaves: int, pin=None,
                    soft: bool = False):
    """The int32 table of one network-topology group (layout in
    ``vamd_api.h``): ``tiers`` is a list, lowest tier first, of lists of
    ``(lo, hi)`` leaf ranges; ``pin`` a leaf range every candidate must
    contain, or None."""
    import numpy as np
    T = len(tiers)
    pin_lo, pin_hi = (n_leaves, 0) if pin is None else pin
    head = [T, int(need), int(pin_lo), int(pin_hi), 1 if soft else 0]
    off = HN_TAB_HEAD + T + 1
    offs, pairs = [], []
    for tier in tiers:
        offs.append(off + len(pairs))
        for lo, hi in tier:
            pairs += [int(lo), int(hi)]
    offs.append(off + len(pairs))
    return np.asarray(head + offs + pairs, dtype=np.int32)


def check_hypernode_table(tab, n_leaves: int) -> None:
    """Shape rules of a mode-3 table (host numpy int32): the kernel trusts
    the offsets, so they are checked before any launch."""
    n = tab.shape[0]
    if tab.ndim != 1 or n < 7:
        raise ValueError("hypernode table: too short")
    T, need = int(tab[0]), int(tab[1])
    if T < 1 or need < 1:
        raise ValueError("hypernode table: T and need must be >= 1")
    if n < 6 + T:
        raise ValueError("hypernode table: tier offsets cut short")
    offs = tab[5:6 + T].astype("int64")
    if offs[0] != 6 + T or (offs[1:] < offs[:-1]).any() or offs[-1] != n \
            or ((offs[1:] - offs[:-1]) % 2).any():
        raise ValueError("hypernode table: tier offsets must ascend from "
                         "the end of the header to the end of the table in "
                         "steps of whole pairs")
    pairs = tab[6 + T:].reshape(-1, 2)
    if ((pairs[:, 0] < 0) | (pairs[:, 1] < pairs[:, 0])
            | (pairs[:, 1] > n_leaves)).any():
        raise ValueError("hypernode table: a leaf range lies outside "
                         "0 <= lo <= hi <= D")


def hypernode_choice(cap, leaf_of, table, n_leaves: int):
    """The winning ``(lo, hi)`` leaf range of ``hypernode_mask``, or None.
    Plain Python integers throughout — no width to overflow."""
    D = int(n_leaves)
    tab = [int(x) for x in table.tolist()]
    T, need, pin_lo, pin_hi = tab[0], tab[1], tab[2], tab[3]
    if T < 1 or need < 1:
        raise ValueError("hypernode table: T and need must be >= 1")
    L = [0] * D
    for c, leaf in zip(cap.tolist(), leaf_of.tolist()):
        if 0 <= leaf < D:
            L[leaf] += int(c)
    P = [0] * (D + 1)
    for d in range(D):
        P[d + 1] = P[d] + L[d]
    for t in range(T):
        o0, o1 = tab[HN_TAB_HEAD + t], tab[HN_TAB_HEAD + t + 1]
        best = None
        for k in range((o1 - o0) // 2):
            lo, hi = tab[o0 + 2 * k], tab[o0 + 2 * k + 1]
            if lo < 0 or hi < lo or hi > D:
                continue
            if lo > pin_lo or pin_hi > hi:
                continue
            C = P[hi] - P[lo]
            if C >= need and (best is None or C < best[0]):
                best = (C, lo, hi)
        if best is not None:
            return best[1], best[2]
    return None


def hypernode_mask(
    score: torch.Tensor,        # [N] f32 from score_cap, in place
    cap: torch.Tensor,          # [N] i32, in place
    leaf_of: torch.Tensor,      # [N] i32 leaf id in [0, D), -1 = no hypernode
    table: torch.Tensor,        # the group's int32 table (hypernode_table)
    n_leaves: int,              # D
) -> None:
    """Confine one class to ONE network domain (hypernode), chosen from the
    live per-node ``cap`` — the source of truth for mode 3 of the HIP
    ``domain_mask``.

    Leaves are numbered depth-first, so a hypernode of any tier is a leaf
    range ``[lo, hi)`` and its capacity the sum of ``cap`` over it.  Tiers
    are tried lowest first; within a tier the eligible domain (containing
    the pin) with the smallest capacity ``>= need`` wins, ties to the lower
    table index.  Nodes outside the winner — unlabelled ones included — get
    ``score = -inf``, ``cap = 0``; kept nodes are untouched.  Without a
    winner hard mode masks every node, soft mode none.  The ordinary
    ``select_commit`` follows.
    """
    win = hypernode_choice(cap, leaf_of, table, n_leaves)
    if win is None:
        if int(table[4]) != 0:
            return
        win = (0, 0)
    leaf = leaf_of.to(torch.int64)
    out = (leaf < win[0]) | (leaf >= win[1])
    score[out] = NEG_INF
    cap[out] = 0


# -- device share: per-card packing of GPU slices ---------------------------
#
# Card planes are CPU int32 tensors [K, N]: ``mem_used``, ``cores_used`` and
# ``state`` (slice count, DEV_GONE set for an exclusive or absent card),
# plus ``mem_total`` [N].  A request is (count, memory, cores).  The oracles
# are the plain per-pod loop over ``GPUDevicePool`` — the sequential host
# rule itself; the ``*_closed`` twins are the closed form the HIP kernels
# compute (one array pass, no per-pod step).

DEV_GONE = 1 << 30              # card_state bit: exclusive or absent
DEV_MAX_CARDS = 16              # K of the card planes
DEV_MEM_LIMIT = 1 << 28         # mem_total (and a slice) stays below this
DEV_TAKE_BITS = 28              # assignment word: card << 28 | take


def check_device_request(request):
    """(count, memory, cores) as ints, or ValueError."""
    count, memory, cores = (int(x) for x in request)
    if count < 1 or not 0 <= memory < DEV_MEM_LIMIT or not 0 <= cores <= 100:
        raise ValueError(
            f"device request {(count, memory, cores)}: count >= 1, "
            f"0 <= memory < 2^28, 0 <= cores <= 100")
    return count, memory, cores


def check_card_planes(mem_used, cores_used, state) -> None:
    """ValueError unless the numpy card planes hold what the packing rule
    is closed form on: ``mem_used >= 0`` (with ``mem_total < 2^28`` that
    keeps ``mem_total - mem_used`` of a card that is not over-full in
    [0, 2^28), hence its slots below 2^28), ``cores_used >= 0`` and a
    slice count ``state & ~DEV_GONE`` in [0, 2^28).  ``mem_used`` above
    ``mem_total`` is an over-full card: no slots, nothing wrong."""
    if mem_used.min(initial=0) < 0:
        raise ValueError("device state: mem_used below 0")
    if cores_used.min(initial=0) < 0:
        raise ValueError("device state: cores_used below 0")
    slices = state & ~DEV_GONE
    if slices.min(initial=0) < 0 or slices.max(initial=0) >= DEV_MEM_LIMIT:
        raise ValueError("device state: slice count outside [0, 2^28)")


def _device_pool(mem_used, cores_used, state, mem_total, n):
    """Node n's cards as a GPUDevicePool (an absent card can never be
    taken, like an exclusive one)."""
    from ..api.devices import Card, GPUDevicePool
    pool = GPUDevicePool.__new__(GPUDevicePool)
    pool.cards = [
        Card(k, int(mem_total[n]), int(mem_used[k, n]), int(cores_used[k, n]),
             bool(int(state[k, n]) & DEV_GONE), int(state[k, n]) & ~DEV_GONE)
        for k in range(mem_used.shape[0])]
    return pool


def _card_arrays(mem_used, cores_used, state, mem_total):
    for t in (mem_used, cores_used, state, mem_total):
        if t.device.type != "cpu" or t.dtype != torch.int32:
            raise ValueError("device oracles take CPU int32 card planes")
    return (mem_used.numpy(), cores_used.numpy(), state.numpy(),
            mem_total.numpy())


def device_cap(score, cap, mem_used, cores_used, state, mem_total,
               request) -> None:
    """``cap[n] = min(cap[n], pods GPUDevicePool.allocate packs in a row)``,
    ``score[n] = -inf`` where that is 0 — the oracle of the HIP
    ``device_cap``."""
    from ..api.devices import DeviceRequest
    req = DeviceRequest(*check_device_request(request))
    mu, cu, st, total = _card_arrays(mem_used, cores_used, state, mem_total)
    cap_h = cap.cpu()
    for n in torch.nonzero(cap_h > 0).flatten().tolist():
        pool = _device_pool(mu, cu, st, total, n)
        fit = 0
        while fit < int(cap_h[n]) and pool.allocate(req) is not None:
            fit += 1
        if fit < int(cap_h[n]):
            cap[n] = fit
            if fit == 0:
                score[n] = NEG_INF


def device_commit(log_nodes, log_counts, log_len, mem_used, cores_used,
                  state, mem_total, assign, request) -> None:
    """Every logged pod takes its slices through ``GPUDevicePool.allocate``,
    one pod at a time; ``assign`` [L, K] (CPU int32) records, per entry, the
    run-length form of the picked cards: ``card << 28 | take`` in pick
    order, then zeros — the oracle of the HIP ``device_commit``."""
    from ..api.devices import DeviceRequest
    req = DeviceRequest(*check_device_request(request))
    mu, cu, st, total = _card_arrays(mem_used, cores_used, state, mem_total)
    rows = assign.numpy().view("uint32")
    nodes, counts = log_nodes.cpu().tolist(), log_counts.cpu().tolist()
    for e in range(min(int(log_len), len(nodes))):
        rows[e] = 0
        if counts[e] <= 0:
            continue
        n = nodes[e]
        pool = _device_pool(mu, cu, st, total, n)
        runs = []                           # [card, take] in pick order
        for _ in range(counts[e]):
            picked = pool.allocate(req)
            if picked is None:
                raise RuntimeError(f"device_commit: node {n} cannot pack "
                                   f"{counts[e]} pods of {request}")
            for k in picked:
                if runs and runs[-1][0] == k:
                    runs[-1][1] += 1
                else:
                    runs.append([k, 1])
        for p, (k, take) in enumerate(runs):
            rows[e, p] = (k << DEV_TAKE_BITS) | take
        for c in pool.cards:
            mu[c.index, n], cu[c.index, n] = c.mem_used, c.cores_used
            st[c.index, n] = c.slices | (DEV_GONE if c.exclusive else 0)


def device_revert(flag, log_nodes, log_len, mem_used, cores_used, state,
                  mem_total, assign, request) -> None:
    """When ``flag`` is 0 the cards release what ``assign`` recorded
    (``Card.release`` per slice) and ``assign`` is zeroed."""
    from ..api.devices import DeviceRequest
    if int(flag) != 0:
        return
    req = DeviceRequest(*check_device_request(request))
    mu, cu, st, total = _card_arrays(mem_used, cores_used, state, mem_total)
    rows = assign.numpy().view("uint32")
    nodes = log_nodes.cpu().tolist()
    for e in range(min(int(log_len), len(nodes))):
        n = nodes[e]
        pool = _device_pool(mu, cu, st, total, n)
        for word in rows[e].tolist():
            c = pool.cards[word >> DEV_TAKE_BITS]
            for _ in range(word & ((1 << DEV_TAKE_BITS) - 1)):
                c.release(req)
            mu[c.index, n], cu[c.index, n] = c.mem_used, c.cores_used
            st[c.index, n] = c.slices | (DEV_GONE if c.exclusive else 0)
        rows[e] = 0


def device_slots(mem_used, cores_used, state, mem_total, request):
    """Closed form, fact 1: slots per card [K, N] (int64 numpy) — how many
    slices of the shape each card still takes; a node packs exactly
    ``slots.sum(0) // count`` pods, whatever the order."""
    import numpy as np
    count, memory, cores = check_device_request(request)
    mu, cu, st, total = (a.astype(np.int64) for a in _card_arrays(
        mem_used, cores_used, state, mem_total))
    gone = (st & DEV_GONE) != 0
    if memory == 0 and cores == 0:
        return np.where(~gone & (st == 0), 1, 0).astype(np.int64)
    s = np.full(mu.shape, np.iinfo(np.int64).max)
    if memory > 0:
        s = np.minimum(s, np.floor_divide(total[None, :] - mu, memory))
    if cores > 0:
        s = np.minimum(s, np.floor_divide(100 - cu, cores))
    return np.where(gone | (mu > total[None, :]), 0, np.maximum(s, 0))


def device_cap_closed(score, cap, mem_used, cores_used, state, mem_total,
                      request) -> None:
    """``device_cap`` in closed form (what the HIP kernel computes)."""
    import numpy as np
    fit = device_slots(mem_used, cores_used, state, mem_total,
                       request).sum(0) // int(request[0])
    cap_h = cap.cpu().numpy().astype(np.int64)
    hit = torch.from_numpy((cap_h > 0) & (fit < cap_h))
    cap[hit] = torch.from_numpy(fit.astype(np.int32))[hit]
    score[hit & torch.from_numpy(fit == 0)] = NEG_INF


def device_commit_closed(log_nodes, log_counts, log_len, mem_used,
                         cores_used, state, mem_total, assign,
                         request) -> None:
    """``device_commit`` in closed form, fact 2: the cards of a node fill
    in the order (mem_used desc, index asc) among cards with slots, each to
    its slot count; card k takes ``clamp(cnt*count - prefix_k, 0,
    slots_k)`` with ``prefix_k`` the slots ranked before it."""
    import numpy as np
    count, memory, cores = check_device_request(request)
    slots = device_slots(mem_used, cores_used, state, mem_total, request)
    mu, cu, st, _ = _card_arrays(mem_used, cores_used, state, mem_total)
    rows = assign.numpy().view("uint32")
    K = mu.shape[0]
    nodes, counts = log_nodes.cpu().tolist(), log_counts.cpu().tolist()
    for e in range(min(int(log_len), len(nodes))):
        rows[e] = 0
        if counts[e] <= 0:
            continue
        n = nodes[e]
        s = slots[:, n]
        order = sorted((k for k in range(K) if s[k] > 0),
                       key=lambda k: (-int(mu[k, n]), k))
        prefix = 0
        for p, k in enumerate(order):
            take = int(min(max(counts[e] * count - prefix, 0), s[k]))
            prefix += int(s[k])
            if take == 0:
                break
            rows[e, p] = (k << DEV_TAKE_BITS) | take
            if memory == 0 and cores == 0:
                st[k, n] = (int(st[k, n]) + take) | DEV_GONE
            else:
                st[k, n] += take
                mu[k, n] += take * memory
                cu[k, n] += take * cores


def device_cards(row, cnt: int, count: int):
    """One card list per pod from an assignment row: the row spells the
    slice sequence, pod i owns positions [i*count, (i+1)*count)."""
    seq = []
    for word in (int(w) & 0xFFFFFFFF for w in row):
        seq.extend([word >> DEV_TAKE_BITS]
                   * (word & ((1 << DEV_TAKE_BITS) - 1)))
    return [seq[i * count:(i + 1) * count] for i in range(cnt)]


# -- numaaware: pinning CPU requests to NUMA zones --------------------------
#
# ``zone_free`` is a CPU int32 tensor [Z, N]: free millicores per zone, 0 for
# the missing zones of a smaller node.  A request is ``cpu`` millicores that
# must come from one zone.  The oracles are the plain per-pod loop of
# ``NumaState.best_zone`` / ``take`` on integers (the host's +0.1 slack is
# nothing there); ``numa_slots`` is the closed form the HIP kernels compute.

NUMA_MAX_ZONES = 8              # Z of the zone plane
NUMA_FREE_LIMIT = 1 << 28       # a zone's free millicores stay below this
NUMA_TAKE_BITS = 28             # assignment word: zone << 28 | take
NUMA_HARD, NUMA_BEST_EFFORT = 1, 2      # single-numa-node / restricted; soft


def check_numa_request(cpu, policy):
    """(cpu, policy) as ints, or ValueError."""
    cpu, policy = int(cpu), int(policy)
    if not 1 <= cpu < NUMA_FREE_LIMIT or \
            policy not in (NUMA_HARD, NUMA_BEST_EFFORT):
        raise ValueError(f"numa request {(cpu, policy)}: 1 <= cpu < 2^28, "
                         "policy 1 (hard) or 2 (best-effort)")
    return cpu, policy


def _zone_plane(zone_free):
    if zone_free.device.type != "cpu" or zone_free.dtype != torch.int32 \
            or zone_free.dim() != 2:
        raise ValueError("numa oracles take a CPU int32 zone plane [Z, N]")
    return zone_free.numpy()


def _best_zone(free, cpu: int):
    """``NumaState.best_zone`` on integers: the smallest zone that fits,
    the strict ``<`` leaving ties to the lower index."""
    best = None
    for z, f in enumerate(free):
        if f >= cpu and (best is None or f < free[best]):
            best = z
    return best


def numa_cap(score, cap, zone_free, cpu: int) -> None:
    """``cap[n] = min(cap[n], pods best_zone pins in a row)``,
    ``score[n] = -inf`` where that is 0 — the oracle of the HIP
    ``numa_cap`` (hard policies only)."""
    cpu, _ = check_numa_request(cpu, NUMA_HARD)
    zf = _zone_plane(zone_free)
    cap_h = cap.cpu()
    for n in torch.nonzero(cap_h > 0).flatten().tolist():
        free = zf[:, n].tolist()
        fit = 0
        while fit < int(cap_h[n]):
            z = _best_zone(free, cpu)
            if z is None:
                break
            free[z] -= cpu
            fit += 1
        if fit < int(cap_h[n]):
            cap[n] = fit
            if fit == 0:
                score[n] = NEG_INF


def numa_commit(log_nodes, log_counts, log_len, zone_free, assign,
                cpu: int) -> None:
    """Every logged pod asks ``best_zone`` and takes its request, one pod
    at a time; a pod that finds no zone stays unpinned.  ``assign`` [L, Z]
    (CPU int32) records, per entry, the run-length form of the picked
    zones: ``zone << 28 | take`` in pick order, then zeros — the oracle of
    the HIP ``numa_commit``."""
    cpu, _ = check_numa_request(cpu, NUMA_HARD)
    zf = _zone_plane(zone_free)
    rows = assign.numpy().view("uint32")
    nodes, counts = log_nodes.cpu().tolist(), log_counts.cpu().tolist()
    for e in range(min(int(log_len), len(nodes))):
        rows[e] = 0
        n = nodes[e]
        free = zf[:, n].tolist() if counts[e] > 0 else []
        runs = []                           # [zone, take] in pick order
        for _ in range(max(counts[e], 0)):
            z = _best_zone(free, cpu)
            if z is None:
                break
            free[z] -= cpu
            if runs and runs[-1][0] == z:
                runs[-1][1] += 1
            else:
                runs.append([z, 1])
        for p, (z, take) in enumerate(runs):
            rows[e, p] = (z << NUMA_TAKE_BITS) | take
            zf[z, n] = free[z]


def numa_revert(flag, log_nodes, log_len, zone_free, assign,
                cpu: int) -> None:
    """When ``flag`` is 0 the zones get back what ``assign`` recorded
    (``NumaState.give`` per pod) and ``assign`` is zeroed."""
    if int(flag) != 0:
        return
    cpu, _ = check_numa_request(cpu, NUMA_HARD)
    zf = _zone_plane(zone_free)
    rows = assign.numpy().view("uint32")
    nodes = log_nodes.cpu().tolist()
    for e in range(min(int(log_len), len(nodes))):
        for word in rows[e].tolist():
            for _ in range(word & ((1 << NUMA_TAKE_BITS) - 1)):
                zf[word >> NUMA_TAKE_BITS, nodes[e]] += cpu
        rows[e] = 0


def numa_slots(zone_free, cpu: int):
    """Closed form: slots per zone [Z, N] (int64 numpy) — how many pods of
    ``cpu`` millicores each zone still pins; a node pins exactly
    ``slots.sum(0)`` of them, and they fill the zones in the order
    (free asc, index asc) among zones with slots, each to its count."""
    import numpy as np
    cpu, _ = check_numa_request(cpu, NUMA_HARD)
    zf = _zone_plane(zone_free).astype(np.int64)
    return np.where(zf > 0, zf // cpu, 0)


def numa_zones(row, cnt: int):
    """One zone (or None: unpinned) per pod from an assignment row: the
    row spells the zone sequence, the pods past its end found no zone."""
    seq = []
    for word in (int(w) & 0xFFFFFFFF for w in row):
        seq.extend([word >> NUMA_TAKE_BITS]
                   * (word & ((1 << NUMA_TAKE_BITS) - 1)))
    return (seq + [None] * cnt)[:cnt]


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
