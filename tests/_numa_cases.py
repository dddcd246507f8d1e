"""The one case builder of the NUMA tests: hand-written zone sets, a zone
plane that holds every family the pinning rule can go wrong on, and a
hand-built plan with NUMA classes on every route of the cycle runner."""

import functools

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


def build_numa_plan(device, Z=3):
    """Z = 3: the small plan.  Z = 8: the same plan on eight zones, where
    classes pin into zones 4 to 7."""
    case, numa, devices, rules = numa_plan_case()
    plan = kc.build_plan(case, device)
    plan.set_numa_state(zone_case(case.N, Z, 11)["zone_free"])
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


# -- the integer limits of the packing kernels ------------------------------
#
# Zone values at the top of the contract, where the per-pod oracle cannot
# walk.  The oracle is the closed form in numpy on ``ref.numa_slots``
# (``numa_cap_closed`` / ``numa_commit_closed``); ``zone_closed_py`` derives
# it again on plain Python integers from the pieces of ``_deviceshare_cases``.
# Eight zones of 2^28 - 1 slots sum to 2^31 - 8 and a pod needs one slot, so
# no sum or product of this policy leaves int32 and no word has its sign bit
# set: of ``dc.MUTANTS`` only the three below differ from the right kernel
# on a legitimate zone plane.

TOP, INT_MAX, BIG_N = dc.TOP, dc.INT_MAX, dc.BIG_N
MUTANTS = ("mask-24", "unroll-short", "ties-to-higher")


def numa_cap_closed(score, cap, zone_free, cpu):
    """``numa_cap`` in closed form on numpy arrays, in place."""
    S = ref.numa_slots(torch.from_numpy(zone_free), cpu).sum(0)
    hit = (cap > 0) & (S < cap)
    cap[hit] = S[hit]
    score[hit & (S == 0)] = -np.inf


def numa_commit_closed(log_nodes, log_counts, zone_free, rows, cpu):
    """``numa_commit`` in closed form on numpy arrays, in place: zones with
    slots fill in the order (free asc, index asc), each taking
    ``clamp(cnt - prefix, 0, slots)``."""
    slots = ref.numa_slots(torch.from_numpy(zone_free), cpu)
    Z = zone_free.shape[0]
    words = rows.view(np.uint32)
    for e, (n, cnt) in enumerate(zip(log_nodes.tolist(),
                                     log_counts.tolist())):
        words[e] = 0
        if cnt <= 0:
            continue
        order = [z for z in np.lexsort((np.arange(Z), zone_free[:, n]))
                 if slots[z, n] > 0]
        s = slots[order, n]
        take = np.clip(cnt - (np.cumsum(s) - s), 0, s)
        for p, (z, t) in enumerate(zip(order, take.tolist())):
            if t > 0:
                words[e, p] = (int(z) << ref.NUMA_TAKE_BITS) | t
                zone_free[z, n] -= t * cpu


def zone_closed(case, cpu):
    """cap, rows, decoded runs and the plane after the commit of ``case``
    from the numpy closed form: the oracle of the GPU tests."""
    score, cap, free = (case[k].copy() for k in ("score", "cap", "zone_free"))
    numa_cap_closed(score, cap, case["zone_free"], cpu)
    rows = np.zeros((len(case["log_nodes"]), free.shape[0]), dtype=np.int32)
    numa_commit_closed(case["log_nodes"], case["log_counts"], free, rows, cpu)
    rows = rows.view(np.uint32).tolist()
    return dict(score=score, cap=cap.tolist(), rows=rows,
                runs=[[dc.pack_decode(w) for w in row if w] for row in rows],
                zone_free=free.tolist())


CLOSED_KEYS = ("cap", "rows", "runs", "zone_free")


def zone_closed_py(case, cpu, wrong=None):
    """The same figures on Python integers."""
    free = case["zone_free"].tolist()
    Z, N = case["zone_free"].shape
    slots = [[free[z][n] // cpu if free[z][n] > 0 else 0 for z in range(Z)]
             for n in range(N)]
    cap = [dc.pack_cap_py(slots[n], 1, c, (2, 4, 8), wrong)
           for n, c in enumerate(case["cap"].tolist())]
    rows, runs = [], []
    for n, cnt in zip(case["log_nodes"].tolist(),
                      case["log_counts"].tolist()):
        fill = dc.pack_fill_py([free[z][n] for z in range(Z)], slots[n], cnt,
                               1, wrong) if cnt > 0 else []
        words = [dc.pack_word(z, take, wrong) for z, take in fill]
        rows.append(words + [0] * (Z - len(words)))
        runs.append([dc.pack_decode(w, wrong) for w in words])
        for z, take in fill:
            free[z][n] -= take * cpu
    return dict(cap=cap, rows=rows, runs=runs, zone_free=free)


def _big_case(free, caps, period):
    N = free.shape[1]
    cap = np.asarray(caps, dtype=np.int64)[
        (np.arange(N) // period) % len(caps)]
    score = np.where(cap > 0, 0.5, -np.inf).astype(np.float32)
    return dict(zone_free=free.astype(np.int32), cap=cap.astype(np.int32),
                score=score)


def _fit_log(case, cpu, policy):
    """A log over the first 40 nodes: all S pods, one, and about half in
    turn (0 where S is 0), two more each under best-effort; entry 1
    zeroed."""
    S = ref.numa_slots(torch.from_numpy(case["zone_free"]), cpu).sum(0)
    over = 2 if policy == SOFT else 0
    entries = [(n, [int(S[n]), min(int(S[n]), 1), (int(S[n]) + 1) // 2][n % 3]
                + over) for n in range(40)]
    entries[1] = (1, 0)
    return dc._set_log(case, entries)


def _top_zones(Z, cpu, policy):
    """free = 2^28 - 1 and pods of one millicore.  Columns, node n holding
    pattern n % 4: A every zone at the top (all keys tie, the fill goes by
    index), B free[z] = top - z (fill order Z - 1 .. 0), C the reverse, D
    only the last zone has room.  S = 2^31 - 8 on A at Z = 8."""
    z = np.arange(Z)
    free = dc._columns([TOP + 0 * z, TOP - z, TOP - (Z - 1 - z),
                        np.where(z == Z - 1, TOP, 0)])
    case = _big_case(free, [INT_MAX, 1 << 30, 5, 0], 4)
    A, B, C, D = range(4)                   # + 4 j: the j-th such node
    S, S_B = Z * TOP, Z * TOP - Z * (Z - 1) // 2
    if policy == HARD:
        # C's first zone in fill order is zone 0: that fill ends on its brim
        log = [(A, S), (A + 4, S - 1), (A + 8, 0), (B, S_B), (B + 4, S_B - 1),
               (C, TOP - (Z - 1)), (C + 4, 1 << 24), (D, TOP), (64, 5)]
    else:
        log = [(A, S + 2), (A + 4, INT_MAX), (A + 8, 0), (B, S_B + 2),
               (B + 4, INT_MAX), (C, INT_MAX), (D, TOP + 1), (64, S + 2)]
    return dc._set_log(case, log)


def _one_slot_zones(Z, cpu, policy):
    """A pod as large as a zone (cpu = 2^28 - 1): one slot at the top
    value, none one millicore below it."""
    free = np.random.RandomState(3).choice([TOP, TOP, TOP - 1, 0],
                                           size=(Z, BIG_N))
    return _fit_log(_big_case(free, [50, 1, 3, 0], 1), cpu, policy)


def _odd_zones(Z, cpu, policy):
    """No power of two: pods of 16,385 millicores on zones from one slot
    (and one millicore short of it) to the top."""
    free = np.random.RandomState(4).choice(
        [TOP, 250_000_000, 123_456_789, 16_385, 16_384, 0], size=(Z, BIG_N))
    return _fit_log(_big_case(free, [INT_MAX, 1000, 3, 0], 1), cpu, policy)


BIG_ZONE_CASES = {
    f"{name}-Z{Z}": (build, Z, cpu)
    for name, build, cpu in (("top", _top_zones, 1),
                             ("one-slot", _one_slot_zones, TOP),
                             ("cpu16385", _odd_zones, 16_385))
    for Z in (8, 5)}


@functools.lru_cache(maxsize=None)
def big_zone_case(name, policy):
    """(case, cpu, oracle): built once, never modified."""
    build, Z, cpu = BIG_ZONE_CASES[name]
    case = build(Z, cpu, policy)
    return case, cpu, zone_closed(case, cpu)
