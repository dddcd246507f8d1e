"""Inputs shared by the network-topology (hypernode) tests: the two
scheduler scenarios the host-side domain choice gets wrong, and the kernel
cases of ``test_hypernode_gpu``."""

import numpy as np

from volcano_amd.ops import reference as ref

GI = 1024 ** 3
INT_MAX = 2 ** 31 - 1


def schedule(scenario, device="cpu", exact=True):
    """One cycle with ``network-topology-aware`` -> {pod: node}.

    ``two-gangs``: racks a and b hold one gang of 4 each; two such gangs
    arrive in one cycle.  ``fragmented``: rack a has the larger summed idle
    CPU (3 x 1.5) but no node fits one 2-CPU pod; rack b (2 x 2) fits the
    gang of 2."""
    from volcano_amd.api.objects import (HyperNode, HyperNodeMember,
                                         MemberSelector, ObjectMeta)
    from volcano_amd.scheduler import (FakeBinder, Scheduler, SchedulerCache,
                                       default_config)
    from volcano_amd.scheduler.config import PluginOption
    from volcano_amd.store import ObjectStore
    from volcano_amd.utils import synth
    store, binder = ObjectStore(), FakeBinder()
    config = default_config()
    if device == "cuda":
        config.use_hip = True
        config.device = "cuda"
    config.tiers[1].plugins.append(PluginOption(
        "network-topology-aware", arguments={"exact": exact}))
    sched = Scheduler(SchedulerCache(store=store, binder=binder,
                                     device=device), config)
    if scenario == "two-gangs":
        racks = {"a": [4000, 4000], "b": [4000, 4000]}
        gangs = {"g1": 4, "g2": 4}
    else:
        racks = {"a": [1500, 1500, 1500], "b": [2000, 2000]}
        gangs = {"g1": 2}
    for rack, cpus in racks.items():
        names = [f"{rack}{i}" for i in range(len(cpus))]
        for name, cpu in zip(names, cpus):
            store.create("Node", synth.make_node(name, cpu_milli=cpu,
                                                 mem=64 * GI))
        store.create("HyperNode", HyperNode(
            meta=ObjectMeta(name=f"rack-{rack}"), tier=1,
            members=[HyperNodeMember(
                type="Node", selector=MemberSelector(exact_match=names))]))
    store.create("Queue", synth.make_queue("default"))
    for name, n in gangs.items():
        pg = synth.make_podgroup(name, min_member=n)
        pg.spec.network_topology = {"mode": "hard", "highestTierAllowed": 1}
        store.create("PodGroup", pg)
        for i in range(n):
            store.create("Pod", synth.make_pod(f"{name}-w-{i}", name,
                                               cpu_milli=2000, mem=GI))
    sched.run_once()
    return dict(binder.binds)


def racks_of(binds, gang):
    return {node[0] for pod, node in binds.items()
            if pod.split("/")[-1].startswith(f"{gang}-")}


def kernel_case(N, D, T, *, interleaved, seed=5, caps="random"):
    """score, cap, leaf_of and the tier lists of a T-tier tree over D
    leaves (tier t groups 4**t leaves).  ``caps``: seeded randint(0, 4),
    or ``equal`` (every leaf the same capacity)."""
    rng = np.random.RandomState(seed)
    n = np.arange(N)
    leaf_of = (n % D if interleaved else n * D // N).astype(np.int32)
    cap = rng.randint(0, 4, size=N).astype(np.int32)
    if caps == "equal":
        cap[:] = 1
        leaf_of = (n % D).astype(np.int32)
        leaf_of[N - N % D:] = -1
    else:
        leaf_of[rng.rand(N) < 0.1] = -1
    score = rng.randint(-8, 9, size=N).astype(np.float32) / 4
    score[cap == 0] = -np.inf
    tiers = [[(lo, min(lo + 4 ** t, D)) for lo in range(0, D, 4 ** t)]
             for t in range(T)]
    return score, cap, leaf_of, tiers


def huge_case():
    """Leaf 0 holds two caps of 2**31 - 1 (an int32 sum wraps to -2), leaf
    1 has capacity 10, need is 11: only leaf 0 fits."""
    cap = np.array([INT_MAX, INT_MAX, 4, 6, 3], dtype=np.int32)
    leaf_of = np.array([0, 0, 1, 1, -1], dtype=np.int32)
    score = np.array([1, 2, 5, 4, 9], dtype=np.float32)
    return score, cap, leaf_of, ref.hypernode_table(
        [[(0, 1), (1, 2)]], 11, 2)


def leaf_caps(cap, leaf_of, D):
    out = [0] * D
    for c, l in zip(cap.tolist(), leaf_of.tolist()):
        if l >= 0:
            out[l] += c
    return out


def table_for(need_kind, cap, leaf_of, tiers, D, *, pin, soft):
    """need: 1 / C of the tightest leaf / that + 1 / sum(cap) + 1."""
    L = leaf_caps(cap, leaf_of, D)
    tight = min((c for c in L if c > 0), default=1)
    need = {"one": 1, "tight": tight, "tight+1": tight + 1,
            "all+1": sum(L) + 1}[need_kind]
    mid = D // 2
    return ref.hypernode_table(tiers, min(need, INT_MAX), D,
                               (mid, mid + 1) if pin else None, soft)
