"""The one case builder of the NUMA tests: hand-written zone sets, a zone
plane that holds every family the pinning rule can go wrong on, and a
hand-built plan with NUMA classes on every route of the cycle runner."""

import numpy as np
import torch

import _deviceshare_cases as dc
import _kernel_cases as kc
from volcano_amd.ops import reference as ref

# free millicores per zone: equal zones (the tie), exact multiples of 2500,
# one millicore short of them, zero zones, Z = 1, Z = 8
ZONE_SETS = [[4000, 4000], [5000, 2500], [2499, 4999], [0, 3000, 0], [7000],
             [4000, 1000, 4000, 0, 2500, 999, 5000, 501]]
CPUS = [1, 500, 2500, 9000]             # the last is above every zone
HARD, SOFT = ref.NUMA_HARD, ref.NUMA_BEST_EFFORT


def zone_case(N, Z, seed):
    """A plane [Z, N] drawn from a small set, so ties, exact multiples,
    near misses, empty zones and nodes with fewer than Z zones (none
    included) all occur; ``cap`` holds 0, values below S and far above."""
    rng = np.random.RandomState(seed)
    free = rng.choice([0, 0, 499, 500, 1000, 2499, 2500, 4000, 4000, 7500],
                      size=(Z, N))
    n_zones = rng.randint(0, Z + 1, size=N)
    n_zones[rng.rand(N) < 0.5] = Z
    free[np.arange(Z)[:, None] >= n_zones[None, :]] = 0
    cap = rng.choice([0, 1, 2, 3, 50], size=N).astype(np.int32)
    score = np.where(cap > 0, rng.randint(1, 9, size=N) / 8.0,
                     -np.inf).astype(np.float32)
    return dict(zone_free=free.astype(np.int32), cap=cap, score=score)


def commit_case(L, Z, cpu, policy, seed):
    """A zone case plus a log of L distinct nodes.  Hard: pod counts in
    [1, S] (0 where S is 0); best-effort: up to S + 2, entry 0 always above
    S.  Entry 1 (when there is one) carries a zeroed count."""
    case = zone_case(12 * L + 40, Z, seed)
    S = ref.numa_slots(torch.from_numpy(case["zone_free"]), cpu).sum(0)
    rng = np.random.RandomState(seed + 1)
    nodes = np.concatenate([rng.permutation(np.nonzero(S > 0)[0]),
                            np.nonzero(S == 0)[0]])[:L]
    # the oracle walks pod by pod: at cpu = 1 a full node would be 30k steps
    top = [int(S[n]) if S[n] <= 200 else 40 for n in nodes]
    over = 2 if policy == SOFT else 0
    counts = np.array([rng.randint(1, t + over + 1) if t + over else 0
                       for t in top])
    if policy == SOFT:
        counts[0] = S[nodes[0]] + 2
    if L > 1:
        counts[1] = 0
    case.update(log_nodes=nodes.astype(np.int32),
                log_counts=counts.astype(np.int32), slots=S)
    return case


def numa_plan_case():
    """(PlanCase, {class: (cpu, policy)}, {class: device request}, rules):
    single-class gangs that fit and one that cannot, a discarded and a kept
    multi-class job, a spread and a hypernode class, a class with a device
    and a NUMA request, then two chain-length runs of plain jobs with a
    NUMA job between them."""
    N, R, W = 130, 2, 1
    rng = np.random.RandomState(5)
    st = kc.dyadic_state(N, R, W, 5)
    classes, jobs, numa, devices = [], [], {}, {}

    def job(cls, min_avail, reqs=(), dev=None):
        b = len(classes)
        classes.extend(cls)
        jobs.append((b, len(classes), 0, min_avail))
        numa.update({b + i: rq for i, rq in enumerate(reqs) if rq})
        if dev is not None:
            devices[b] = dev

    def cl(n, q=0, min_needed=0):
        return kc._class(rng, R, W, n, q, min_needed=min_needed, plain=True)

    job([cl(40)], 1, [(500, HARD)])
    job([cl(90, 1)], 1, [(1000, SOFT)])             # sees the zones above
    job([cl(600)], 600, [(1000, HARD)])             # gang that cannot fit
    job([cl(10), cl(3, 1, min_needed=4)], 1, [(500, HARD), None])
    job([cl(9), cl(7, 1)], 1, [(2500, HARD), (1, SOFT)])
    rules = {len(classes): "spread", len(classes) + 1: "hypernode"}
    job([cl(12)], 1, [(500, HARD)])
    job([cl(6)], 6, [(1000, HARD)])
    job([cl(8)], 1, [(500, HARD)], dev=(1, 300, 0))
    for _ in range(35):
        job([cl(int(rng.randint(1, 4)), int(rng.randint(0, 2)))], 1)
    job([cl(5)], 1, [(500, SOFT)])
    for _ in range(35):
        job([cl(int(rng.randint(1, 4)), int(rng.randint(0, 2)))], 1)
    ql, qa = kc._queues(rng, R, limit_dim0=25)
    case = kc.PlanCase("numa", N, R, W, st, classes, jobs, ql, qa, chain=True)
    return case, numa, devices, rules


def build_numa_plan(device):
    case, numa, devices, rules = numa_plan_case()
    plan = kc.build_plan(case, device)
    plan.set_numa_state(zone_case(case.N, 3, 11)["zone_free"])
    cards = dc.card_case(case.N, 4, 11)
    plan.set_device_state(cards["mem_used"], cards["cores_used"],
                          cards["state"], cards["mem_total"])
    for c, rq in numa.items():
        plan.add_numa_request(plan.classes[c], *rq)
    for c, rq in devices.items():
        plan.add_device_request(plan.classes[c], *rq)
    for c, rule in rules.items():
        if rule == "spread":
            dom_of = (np.arange(case.N) % 5).astype(np.int32)
            plan.classes[c].spread = (plan.add_spread_group(
                dom_of, np.zeros(5, dtype=np.int32)), 1)
        else:
            leaves = (case.N + 9) // 10
            row = plan.add_hypernode_row(np.arange(case.N) // 10, leaves)
            tiers = [[(l, l + 1) for l in range(leaves)], [(0, leaves)]]
            plan.classes[c].hypernode = plan.add_hypernode_group(
                row, ref.hypernode_table(tiers, 6, leaves))
    return plan, numa
