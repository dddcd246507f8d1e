"""The one case builder of the device-share tests: card planes that hold
every family the packing rule can go wrong on, and a hand-built plan with
device classes on every route of the cycle runner."""

import functools

import numpy as np
import torch

import _kernel_cases as kc
from _plan_spy import plans_of
from volcano_amd.ops import reference as ref

# (count, memory, cores): memory-bound, cores-bound, memory == 0 with cores,
# exclusive (one and two whole cards), S no multiple of count, both bounds
REQUESTS = [(1, 300, 0), (2, 100, 40), (3, 0, 30), (1, 0, 0), (2, 0, 0),
            (3, 250, 0), (2, 300, 10)]


def card_case(N, K, seed):
    """Planes [K, N] drawn from small sets, so ties in mem_used, full,
    exclusive and absent cards, and nodes with fewer than K cards (none
    included) all occur; ``cap`` holds 0, values below S / count and values
    far above it."""
    rng = np.random.RandomState(seed)
    mem_total = rng.choice([1000, 600], size=N).astype(np.int32)
    mem_used = rng.choice([0, 0, 200, 200, 500, 900], size=(K, N))
    cores_used = rng.choice([0, 0, 30, 60, 100], size=(K, N))
    state = (mem_used > 0).astype(np.int64) + (cores_used > 0)
    state[rng.rand(K, N) < 0.1] |= ref.DEV_GONE             # exclusive
    n_cards = rng.randint(0, K + 1, size=N)
    n_cards[rng.rand(N) < 0.5] = K
    state[np.arange(K)[:, None] >= n_cards[None, :]] = ref.DEV_GONE
    mem_used = np.minimum(mem_used, mem_total[None, :])
    cap = rng.choice([0, 1, 2, 3, 50], size=N).astype(np.int32)
    score = np.where(cap > 0, rng.randint(1, 9, size=N) / 8.0,
                     -np.inf).astype(np.float32)
    return dict(mem_used=mem_used.astype(np.int32),
                cores_used=cores_used.astype(np.int32),
                state=state.astype(np.int32), mem_total=mem_total,
                cap=cap, score=score)


def planes_of(case, device="cpu"):
    return [torch.from_numpy(case[k].copy()).to(device)
            for k in ("mem_used", "cores_used", "state", "mem_total")]


def commit_case(L, K, request, seed):
    """A card case plus a log of exactly L distinct nodes, each with a pod
    count in [1, what its cards pack]: fills end mid-card and at the brim;
    entry 1 (when there is one) carries a zeroed count, and so do the
    entries of a shape too rare for L nodes (two whole cards at K = 1)."""
    case = card_case(12 * L + 40, K, seed)
    fit = ref.device_slots(*planes_of(case), request).sum(0) // request[0]
    rng = np.random.RandomState(seed + 1)
    nodes = np.concatenate([rng.permutation(np.nonzero(fit > 0)[0]),
                            np.nonzero(fit == 0)[0]])[:L]
    assert len(nodes) == L
    counts = np.array([rng.randint(1, fit[n] + 1) if fit[n] else 0
                       for n in nodes])
    if L > 1:
        counts[1] = 0
    case.update(log_nodes=nodes.astype(np.int32),
                log_counts=counts.astype(np.int32))
    return case


def run_cluster(exact):
    """One allocate cycle on the torch runner over three nodes of two
    1000-MiB cards whose cpu admits 3 of the big pods each (and far more of
    the others), so that under ``exact`` only the cards leave pods pending:

    * ``big``  5 pods, one 600-MiB slice each: the cards hold 2 per node;
    * ``ex``   2 pods, one whole card each: one card is still free;
    * ``vg``   8 pods, one 300-MiB / 60 % slice each: one per card by cores
      (memory alone would admit 3 on a free card), none on the whole card.

    Returns (binds {pod: node}, {pod: annotations}, plans as
    [(job, ntasks, device request, forbid words)])."""
    from volcano_amd.scheduler import (FakeBinder, Scheduler, SchedulerCache,
                                       default_config)
    from volcano_amd.scheduler.config import PluginOption
    from volcano_amd.store import ObjectStore
    from volcano_amd.utils import synth
    GI = 1024 ** 3
    store, binder = ObjectStore(), FakeBinder()
    cache = SchedulerCache(store=store, binder=binder)
    config = default_config()
    config.tiers[1].plugins.append(PluginOption(
        "deviceshare", arguments={} if exact is None else {"exact": exact}))
    sched = Scheduler(cache, config)
    for i in range(3):
        node = synth.make_node(f"g{i}", cpu_milli=3000, mem=64 * GI)
        node.meta.annotations["volcano.sh/gpu-count"] = "2"
        node.meta.annotations["volcano.sh/gpu-memory-per-card"] = "1000"
        store.create("Node", node)
    store.create("Queue", synth.make_queue("default"))
    jobs = (("big", 5, 1000, 10, {"volcano.sh/gpu-number": "1",
                                  "volcano.sh/gpu-memory": "600"}),
            ("ex", 2, 250, 7, {"volcano.sh/gpu-number": "1"}),
            ("vg", 8, 250, 3, {"volcano.sh/vgpu-number": "1",
                               "volcano.sh/vgpu-memory": "300",
                               "volcano.sh/vgpu-cores": "60"}))
    for name, n, cpu, prio, ann in jobs:
        store.create("PodGroup", synth.make_podgroup(name, min_member=1))
        for i in range(n):
            pod = synth.make_pod(f"{name}-w-{i}", name, cpu_milli=cpu,
                                 mem=GI, priority=prio)
            pod.meta.annotations.update(ann)
            store.create("Pod", pod)
    plans = [[(cp.job_key, cp.ntasks, getattr(cp, "device", None),
               cp.forbid.tolist()) for cp in plan.classes]
             for plan in plans_of(sched)]
    anns = {k.split("/")[1]: dict(t.pod.meta.annotations)
            for job in cache.jobs.values() for k, t in job.tasks.items()}
    binds = {k.split("/")[1]: v for k, v in binder.binds.items()}
    return binds, anns, plans


def device_plan_case():
    """(PlanCase, {class index: request}, rules): single-class gangs that
    place and one that cannot, a discarded and a kept multi-class job, a
    spread and a hypernode class, then two chain-length runs of plain jobs
    with a device job between them."""
    N, R, W = 130, 2, 1
    rng = np.random.RandomState(5)
    st = kc.dyadic_state(N, R, W, 5)
    classes, jobs, requests = [], [], {}

    def job(cls, min_avail, reqs=()):
        b = len(classes)
        classes.extend(cls)
        jobs.append((b, len(classes), 0, min_avail))
        for i, rq in enumerate(reqs):
            if rq is not None:
                requests[b + i] = rq

    def cl(n, q=0, min_needed=0):
        return kc._class(rng, R, W, n, q, min_needed=min_needed, plain=True)

    job([cl(40)], 1, [(1, 300, 0)])
    job([cl(30, 1)], 1, [(2, 250, 0)])              # sees the slices above
    job([cl(600)], 600, [(1, 0, 0)])                # gang that cannot fit
    job([cl(10), cl(3, 1, min_needed=4)], 1, [(1, 200, 20), None])
    job([cl(9), cl(7, 1)], 1, [(3, 0, 30), (1, 300, 0)])
    rules = {len(classes): "spread", len(classes) + 1: "hypernode"}
    job([cl(12)], 1, [(1, 100, 10)])
    job([cl(6)], 6, [(2, 100, 0)])
    for _ in range(35):
        job([cl(int(rng.randint(1, 4)), int(rng.randint(0, 2)))], 1)
    job([cl(5)], 1, [(1, 0, 0)])
    for _ in range(35):
        job([cl(int(rng.randint(1, 4)), int(rng.randint(0, 2)))], 1)
    ql, qa = kc._queues(rng, R, limit_dim0=25)
    case = kc.PlanCase("device", N, R, W, st, classes, jobs, ql, qa,
                       chain=True)
    return case, requests, rules


def build_device_plan(device, K=4):
    """K = 4: the small plan.  K = 16: the same plan on sixteen cards, where
    classes place on cards 8 to 15 and their words are negative as int32."""
    case, requests, rules = device_plan_case()
    plan = kc.build_plan(case, device)
    cards = card_case(case.N, K, 11)
    plan.set_device_state(cards["mem_used"], cards["cores_used"],
                          cards["state"], cards["mem_total"])
    for c, rq in requests.items():
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
    return plan, requests


# -- the integer limits of the packing kernels ------------------------------
#
# Values at the top of the contract (every per-unit value below 2^28, sums
# above int32), where the per-pod oracles cannot walk: the oracle is the
# closed form in numpy (``ref.device_*_closed``), and ``card_closed_py``
# derives it again on plain Python integers, which cannot wrap.  The pieces
# of that derivation (``pack_cap_py``, ``pack_fill_py``, ``pack_word``,
# ``pack_decode``) are shared with the zone cases and take a ``wrong``
# switch that emulates one wrong kernel, or one wrong host decode, each.

TOP = (1 << 28) - 1
INT_MAX = (1 << 31) - 1
BIG_N = 65                      # crosses a wave boundary

MUTANTS = ("S-int32", "prefix-int32", "product-int32", "mask-24",
           "decode-sign-extends", "unroll-short", "ties-to-higher")
WRAP_MUTANTS = ("S-int32", "prefix-int32", "product-int32")


def _i32(x):
    """x as a C int holds it after a wrap."""
    return (x + (1 << 31)) % (1 << 32) - (1 << 31)


def _cdiv(a, b):
    """C division: towards zero."""
    return abs(a) // b * (1 if a >= 0 else -1)


def pack_cap_py(slots, need, cap, bounds, wrong=None):
    """The cap kernel on one node: min(cap, S / need) or cap itself.
    ``bounds`` are the unroll bounds of the policy, ascending."""
    U = len(slots)
    if wrong == "unroll-short":
        U = min(U, next(b for b in bounds if b >= U) // 2)
    S = sum(slots[:U])
    if wrong == "S-int32":
        S = _i32(S)
    fit = _cdiv(S, need)
    return fit if cap > 0 and fit < cap else cap


def pack_fill_py(keys, slots, cnt, need, wrong=None):
    """The commit kernel on one log entry: [(unit, take)] in fill order,
    the units without a take left out."""
    sign = -1 if wrong == "ties-to-higher" else 1
    order = sorted((u for u in range(len(slots)) if slots[u] > 0),
                   key=lambda u: (keys[u], sign * u))
    want = cnt * need
    if wrong == "product-int32":
        want = _i32(want)
    runs, prefix = [], 0
    for u in order:
        take = min(max(want - prefix, 0), slots[u])
        prefix += slots[u]
        if wrong == "prefix-int32":
            prefix = _i32(prefix)
        if take > 0:
            runs.append((u, take))
    return runs


def pack_word(unit, take, wrong=None):
    mask = (1 << 24) - 1 if wrong == "mask-24" else TOP
    return (unit << 28 | (take & mask)) & 0xFFFFFFFF


def pack_decode(word, wrong=None):
    """(unit, take) of a word read as uint32; the wrong decode shifts the
    int32."""
    word = int(word) & 0xFFFFFFFF
    unit = _i32(word) >> 28 if wrong == "decode-sign-extends" else word >> 28
    return unit, word & TOP


def _card_slots_py(mu, cu, st, total, request):
    _, memory, cores = request
    if st & ref.DEV_GONE:
        return 0
    if memory == 0 and cores == 0:
        return 1 if st == 0 else 0
    if mu > total:
        return 0
    s = []
    if memory > 0:
        s.append((total - mu) // memory)
    if cores > 0:
        s.append(_cdiv(100 - cu, cores))
    return max(min(s), 0)


def card_closed_py(case, request, wrong=None):
    """cap, the assignment rows, their decoded (card, take) runs and the
    planes after the commit of ``case``, on Python integers."""
    count, memory, cores = request
    mu, cu, st = (case[k].tolist()
                  for k in ("mem_used", "cores_used", "state"))
    total = case["mem_total"].tolist()
    K, N = case["mem_used"].shape
    slots = [[_card_slots_py(mu[k][n], cu[k][n], st[k][n], total[n], request)
              for k in range(K)] for n in range(N)]
    cap = [pack_cap_py(slots[n], count, c, (4, 8, 16), wrong)
           for n, c in enumerate(case["cap"].tolist())]
    rows, runs = [], []
    for n, cnt in zip(case["log_nodes"].tolist(),
                      case["log_counts"].tolist()):
        fill = pack_fill_py([-m for m in (mu[k][n] for k in range(K))],
                            slots[n], cnt, count, wrong) if cnt > 0 else []
        words = [pack_word(k, take, wrong) for k, take in fill]
        rows.append(words + [0] * (K - len(words)))
        runs.append([pack_decode(w, wrong) for w in words])
        for k, take in fill:
            if memory == 0 and cores == 0:
                st[k][n] = (st[k][n] + take) | ref.DEV_GONE
            else:
                st[k][n] += take
                mu[k][n] += take * memory
                cu[k][n] += take * cores
    return dict(cap=cap, rows=rows, runs=runs, mem_used=mu, cores_used=cu,
                state=st)


def card_closed(case, request):
    """The same figures from the numpy closed form of ``reference``: the
    oracle of the GPU tests.  ``score`` and ``cap`` stay numpy."""
    score, cap = (torch.from_numpy(case[k].copy()) for k in ("score", "cap"))
    ref.device_cap_closed(score, cap, *planes_of(case), request)
    planes = planes_of(case)
    L = len(case["log_nodes"])
    assign = torch.zeros((L, case["mem_used"].shape[0]), dtype=torch.int32)
    ref.device_commit_closed(
        torch.from_numpy(case["log_nodes"]),
        torch.from_numpy(case["log_counts"]), torch.tensor(L), *planes[:4],
        assign, request)
    rows = assign.numpy().view(np.uint32).tolist()
    return dict(score=score.numpy(), cap=cap.numpy().tolist(), rows=rows,
                runs=[[pack_decode(w) for w in row if w] for row in rows],
                mem_used=planes[0].tolist(), cores_used=planes[1].tolist(),
                state=planes[2].tolist())


CLOSED_KEYS = ("cap", "rows", "runs", "mem_used", "cores_used", "state")


def _columns(patterns, N=BIG_N):
    """[K, N]: node n holds patterns[n % len(patterns)]."""
    return np.stack([np.asarray(patterns[n % len(patterns)], dtype=np.int64)
                     for n in range(N)], axis=1)


def _big_case(mem_used, cores_used, state, mem_total, caps, period):
    """Planes as int32, and ``cap`` cycling through ``caps`` once per
    ``period`` nodes, so that every column pattern meets every cap."""
    N = mem_used.shape[1]
    cap = np.asarray(caps, dtype=np.int64)[
        (np.arange(N) // period) % len(caps)]
    score = np.where(cap > 0, 0.5, -np.inf).astype(np.float32)
    return dict(mem_used=mem_used.astype(np.int32),
                cores_used=cores_used.astype(np.int32),
                state=state.astype(np.int32),
                mem_total=np.broadcast_to(
                    np.asarray(mem_total, dtype=np.int32), (N,)).copy(),
                cap=cap.astype(np.int32), score=score)


def _set_log(case, entries):
    nodes, counts = zip(*entries)
    assert len(set(nodes)) == len(nodes)
    case.update(log_nodes=np.array(nodes, dtype=np.int32),
                log_counts=np.array(counts, dtype=np.int32))
    return case


def _fit_log(case, request):
    """A log over the nodes that pack something: full, one pod and about
    half in turn; entry 1 zeroed."""
    fit = ref.device_slots(*planes_of(case), request).sum(0) // request[0]
    nodes = np.nonzero(fit > 0)[0][:40]
    entries = [(int(n), [int(fit[n]), 1, (int(fit[n]) + 1) // 2][i % 3])
               for i, n in enumerate(nodes)]
    entries[1] = (entries[1][0], 0)
    return _set_log(case, entries)


def _top_cards(request):
    """mem_total = 2^28 - 1 and one-MiB slices on sixteen cards.  Columns,
    node n holding pattern n % 5: A all cards empty (every key ties, the
    fill goes by index), B mem_used[k] = k (fill order 15 .. 0), C
    mem_used[k] = 15 - k, D only card 15 has room (the rest full), E only
    card 8 (the rest absent).  S = 2^32 - 16 on A."""
    k = np.arange(16)
    mem_used = _columns([0 * k, k, 15 - k, np.where(k == 15, 0, TOP),
                         np.where(k == 8, 0, TOP)])
    state = (mem_used > 0).astype(np.int64)
    state[:, 4::5] = np.where(k == 8, 0, ref.DEV_GONE)[:, None]
    case = _big_case(mem_used, 0 * mem_used, state, TOP,
                     [INT_MAX, 1 << 30, 5, 0], 5)
    A, B, C, D, E = range(5)                # + 5 j: the j-th such node
    if request[0] == 7:
        # 14 cards hold 14 TOP slices on A and 14 TOP - 119 on B and C,
        # both multiples of 7: those fills end on a card boundary with a
        # prefix above 2^31; S // 7 pods leave two slices of the last card
        log = [(A, 16 * TOP // 7), (A + 5, 2 * TOP), (A + 10, 0),
               (B, 2 * TOP - 17), (B + 5, 300_000_000),
               (B + 10, (16 * TOP - 120) // 7), (C, 2 * TOP - 17),
               (C + 5, 1), (D, TOP // 7), (E, 1), (64, TOP // 7)]
    else:
        log = [(A, INT_MAX), (A + 5, TOP), (A + 10, 0), (B, INT_MAX),
               (B + 5, TOP - 15), (C, 1 << 30), (D, TOP), (E, TOP), (64, 5)]
    return _set_log(case, log)


def _one_slot_cards(request):
    """A slice as large as a card: memory = mem_total = 2^28 - 1 (one MiB
    less on every fourth node, which then packs nothing): one slot on an
    empty card, none on a card with one MiB used; take * memory at its
    top."""
    rng = np.random.RandomState(3)
    mem_used = rng.choice([0, 0, 0, 1, TOP], size=(16, BIG_N))
    state = (mem_used > 0).astype(np.int64)
    state[rng.rand(16, BIG_N) < 0.1] = ref.DEV_GONE
    total = np.where(np.arange(BIG_N) % 4 == 3, TOP - 1, TOP)
    case = _big_case(mem_used, 0 * mem_used, state, total, [50, 1, 3, 0], 1)
    return _fit_log(case, request)


def _mid_cards(request):
    """No power of two anywhere: 250,000,000 MiB cards and slices of 16,385
    MiB; memory bounds some cards (50 slots, 0 slots one MiB short) and
    cores others (100, 63, 1, 0 slots at one percent each)."""
    total = 250_000_000
    rng = np.random.RandomState(4)
    mem_used = rng.choice([0, 123_456_789, total - 50 * 16_385 - 7,
                           total - 16_384, total], size=(16, BIG_N))
    cores_used = rng.choice([0, 37, 99, 100], size=(16, BIG_N))
    state = (mem_used > 0).astype(np.int64) + (cores_used > 0)
    state[rng.rand(16, BIG_N) < 0.1] = ref.DEV_GONE
    case = _big_case(mem_used, cores_used, state, total,
                     [INT_MAX, 1000, 3, 0], 1)
    return _fit_log(case, request)


def _overfull_cards(request):
    """mem_used above mem_total, up to the top of int32: such a card is
    over-full and has no slot; its neighbours pack as usual."""
    rng = np.random.RandomState(6)
    mem_used = rng.choice([0, 500, 1001, 1 << 30, INT_MAX], size=(5, BIG_N))
    state = (mem_used > 0).astype(np.int64)
    case = _big_case(mem_used, 0 * mem_used, state, 1000, [50, 1, 3, 0], 1)
    return _fit_log(case, request)


BIG_CARD_CASES = {
    "top-1x1MiB": (_top_cards, (1, 1, 0)),
    "top-7x1MiB": (_top_cards, (7, 1, 0)),
    "one-slot-1": (_one_slot_cards, (1, TOP, 0)),
    "one-slot-3": (_one_slot_cards, (3, TOP, 0)),
    "mid-1-both": (_mid_cards, (1, 16_385, 1)),
    "mid-3-both": (_mid_cards, (3, 16_385, 1)),
    "mid-2-memory": (_mid_cards, (2, 16_385, 0)),
    "overfull-1": (_overfull_cards, (1, 300, 0)),
    "overfull-2": (_overfull_cards, (2, 100, 40)),
}


@functools.lru_cache(maxsize=None)
def big_card_case(name):
    """(case, request, oracle): built once, never modified."""
    build, request = BIG_CARD_CASES[name]
    case = build(request)
    return case, request, card_closed(case, request)
