"""The one case builder of the device-share tests: card planes that hold
every family the packing rule can go wrong on, and a hand-built plan with
device classes on every route of the cycle runner."""

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


def build_device_plan(device):
    case, requests, rules = device_plan_case()
    plan = kc.build_plan(case, device)
    cards = card_case(case.N, 4, 11)
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
