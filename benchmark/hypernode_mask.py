"""Cost of the network-topology domain choice on the device.

Times mode 3 of ``vamd_domain_mask`` (``hypernode_mask_kernel``) with HIP
events at N = 10k — racks of 32 under three tiers, and D = N — and mode 1
(affinity, anchor path) on the same arrays in the same run, for scale; then
mode 3 with one factor varied at a time (tiers, run length, where the sums
live, number of pairs).  Tables are validated on the host beforehand and
the wrapper is called with ``check=False``: the timed window holds one
asynchronous launch and nothing else, for both modes alike.

Then the host choice made without ``exact``: a scheduler session over 10k
nodes under the same racks-of-32 tree is opened and the plugin's own
topology hook (``choose_domain`` inside) is timed per job.

    python benchmark/hypernode_mask.py

Needs a GPU.  Every launch is timed on its own between two events, after
score and cap are restored; 300 launches after 20 of warm-up; median and
the 10th / 90th percentile in microseconds (this includes the launch)."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from volcano_amd.ops import hip
from volcano_amd.ops import reference as ref

DEV = "cuda"
ITERS = 300


def tiers_for(D, group):
    out = [[(l, l + 1) for l in range(D)]]
    if D > group:
        out.append([(lo, min(lo + group, D)) for lo in range(0, D, group)])
    out.append([(0, D)])
    return out


def time_op(fn, score0, cap0):
    score, cap = score0.clone(), cap0.clone()
    times = []
    for it in range(ITERS + 20):
        score.copy_(score0)
        cap.copy_(cap0)
        a, b = torch.cuda.Event(enable_timing=True), \
            torch.cuda.Event(enable_timing=True)
        a.record()
        fn(score, cap)
        b.record()
        b.synchronize()
        if it >= 20:
            times.append(a.elapsed_time(b) * 1000.0)
    times.sort()
    return statistics.median(times), times[len(times) // 10], \
        times[-len(times) // 10]


def main():
    hip._load()
    N = 10000
    rng = np.random.RandomState(3)
    cap0 = torch.from_numpy(rng.randint(0, 4, size=N).astype(np.int32)).to(DEV)
    s = rng.rand(N).astype(np.float32)
    score0 = torch.from_numpy(s).to(DEV)
    score0[cap0 == 0] = float("-inf")
    scratch = hip.spread_scratch(N, DEV)
    for label, D, leaf in (("racks of 32, D=313", 313, np.arange(N) // 32),
                           ("D=N", N, np.arange(N))):
        leaf_of = torch.from_numpy(leaf.astype(np.int32)).to(DEV)
        tiers = tiers_for(D, 8)
        for need in (16, 200):
            host_tab = ref.hypernode_table(tiers, need, D)
            ref.check_hypernode_table(host_tab, D)
            tab = torch.from_numpy(host_tab).to(DEV)
            m3 = time_op(lambda sc, cp: hip.hypernode_mask(
                sc, cp, leaf_of, tab, D, scratch, check=False), score0, cap0)
            print(f"mode 3  {label:22s} need={need:4d}  "
                  f"median {m3[0]:7.1f} us  [p10 {m3[1]:.1f} - p90 {m3[2]:.1f}]")
        cnt = torch.zeros(D, dtype=torch.int32, device=DEV)
        m1 = time_op(lambda sc, cp: hip.domain_mask(
            sc, cp, leaf_of, cnt, 1, scratch), score0, cap0)
        print(f"mode 1  {label:22s} anchor     "
              f"median {m1[0]:7.1f} us  [p10 {m1[1]:.1f} - p90 {m1[2]:.1f}]")

    print()
    n = np.arange(N)

    def run(label, D, leaf, tiers, need=16):
        leaf_of = torch.from_numpy(leaf.astype(np.int32)).to(DEV)
        host_tab = ref.hypernode_table(tiers, need, D)
        ref.check_hypernode_table(host_tab, D)
        tab = torch.from_numpy(host_tab).to(DEV)
        m = time_op(lambda sc, cp: hip.hypernode_mask(
            sc, cp, leaf_of, tab, D, scratch, check=False), score0, cap0)
        print(f"{label:58s} median {m[0]:7.1f} us  [p10 {m[1]:.1f} - p90 {m[2]:.1f}]")

    leaves = lambda D: [(l, l + 1) for l in range(D)]
    run("D=313 contiguous, T=1 (leaf tier only, first tier wins)", 313, n // 32, [leaves(313)])
    run("D=313 contiguous, T=3, winner in tier 0", 313, n // 32,
        [leaves(313), [(lo, min(lo + 8, 313)) for lo in range(0, 313, 8)], [(0, 313)]])
    run("D=313 contiguous, T=3, winner in tier 2 (need 9000)", 313, n // 32,
        [leaves(313), [(lo, min(lo + 8, 313)) for lo in range(0, 313, 8)], [(0, 313)]], need=9000)
    run("D=313 interleaved (one atomic per node), T=1", 313, n % 313, [leaves(313)])
    run("D=1 (one run per wave), T=1", 1, n * 0, [[(0, 1)]])
    run("D=4095 interleaved, sums in LDS, T=1", 4095, n % 4095, [leaves(4095)])
    run("D=4096 interleaved, sums in global scratch, T=1", 4096, n % 4096, [leaves(4096)])
    run("D=4095 interleaved, LDS, T=1 with ONE pair", 4095, n % 4095, [[(0, 4095)]])
    run("D=4096 interleaved, global, T=1 with ONE pair", 4096, n % 4096, [[(0, 4096)]])
    run("D=N global, T=1 with ONE pair", N, n, [[(0, N)]])
    run("D=N global, T=1, N pairs", N, n, [leaves(N)])

    print()
    host_choice()


def host_choice():
    """The plugin's own topology hook (``choose_domain`` without
    ``exact``) per job, in a session over 10k nodes, racks of 32, 8 racks
    per pod, one spine: 354 domains."""
    from volcano_amd.api.objects import (HyperNode, HyperNodeMember,
                                         MemberSelector, ObjectMeta)
    from volcano_amd.scheduler import (FakeBinder, Scheduler, SchedulerCache,
                                       default_config)
    from volcano_amd.scheduler.config import PluginOption
    from volcano_amd.store import ObjectStore
    from volcano_amd.utils import synth
    N, GI = 10000, 1024 ** 3
    store = ObjectStore()
    config = default_config()
    config.tiers[1].plugins.append(PluginOption("network-topology-aware"))
    sched = Scheduler(SchedulerCache(store=store, binder=FakeBinder()),
                      config)
    nodes = synth.make_nodes(N, cpu_milli=32000, mem=64 * GI)
    for nd in nodes:
        store.create("Node", nd)
    names = [nd.meta.name for nd in nodes]

    def hn(name, tier, typ, members):
        store.create("HyperNode", HyperNode(
            meta=ObjectMeta(name=name), tier=tier,
            members=[HyperNodeMember(
                type=typ, selector=MemberSelector(exact_match=members))]))

    racks = [f"rack-{i:04d}" for i in range((N + 31) // 32)]
    for i, r in enumerate(racks):
        hn(r, 1, "Node", names[32 * i:32 * i + 32])
    pods = [f"pod-{i:03d}" for i in range((len(racks) + 7) // 8)]
    for i, p in enumerate(pods):
        hn(p, 2, "HyperNode", racks[8 * i:8 * i + 8])
    hn("spine", 3, "HyperNode", pods)
    store.create("Queue", synth.make_queue("default"))
    # per pod 1 CPU: 16 fit the first rack; 2000 fit no rack (1024 CPUs)
    # and fall through all 313 to the first pod of racks; 20000 fit no
    # pod either and fall through to the spine
    shapes = (("first rack fits", 16), ("first tier-2 domain fits", 2000),
              ("only the spine fits", 20000))
    reps = 5
    for label, n in shapes:
        for k in range(reps):
            name = f"j{n}-{k}"
            pg = synth.make_podgroup(name, min_member=n)
            pg.spec.network_topology = {"mode": "hard",
                                        "highestTierAllowed": 3}
            store.create("PodGroup", pg)
            for i in range(n):
                store.create("Pod", synth.make_pod(
                    f"{name}-w-{i}", name, cpu_milli=1000, mem=GI))
    t0 = time.perf_counter()
    ssn = sched.open_session()
    print(f"open_session, {N} nodes, {len(racks) + len(pods) + 1} domains: "
          f"{time.perf_counter() - t0:6.2f} s")
    hook = next(h for h in ssn.class_constraint_hooks
                if getattr(h, "is_topology", False))
    words = ssn.node_tensors.labels.max_words
    for label, n in shapes:
        times = []
        for k in range(reps):
            job = next(j for j in ssn.jobs.values()
                       if j.key.endswith(f"j{n}-{k}"))
            tc = job.pending_classes()[0]
            require = np.zeros(words, dtype=np.int64)
            forbid = np.zeros(words, dtype=np.int64)
            t0 = time.perf_counter()
            hook(tc, job, require, forbid)
            times.append((time.perf_counter() - t0) * 1e6)
            assert require.any()         # a domain bit was set
        times.sort()
        print(f"host choose_domain, gang of {n:5d}, {label:26s} "
              f"median {times[len(times) // 2]:9.1f} us  "
              f"[{times[0]:.1f} - {times[-1]:.1f}] per job")
    sched.close_session(ssn)


if __name__ == "__main__":
    main()
