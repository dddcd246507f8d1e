"""Re-scoring select (nodeorder ``exact: true``) on the CPU: the oracle by
hand, against the static select where re-scoring cannot matter, and through
the scheduler."""

import pytest
import torch

import _kernel_cases as kc
from volcano_amd.ops import reference as ref


def run_select(st, ntasks, *, w_least=1.0, w_most=0.0, bias=None,
               static=False, K=None):
    """One select on a state dict -> (nodes, counts, used, queue_alloc,
    placed, job_placed)."""
    N, R = st["alloc"].shape
    zw = torch.zeros(st["planes"].shape[1], dtype=torch.int64)
    score, cap = kc.oracle_score_cap(st, w_least=w_least, w_most=w_most,
                                     bias=bias)
    K = max(1, min(ntasks, N)) if K is None else K
    ln = torch.zeros(K, dtype=torch.int32)
    lc = torch.zeros(K, dtype=torch.int32)
    ll, pl = (torch.zeros((), dtype=torch.int32) for _ in range(2))
    jp = torch.full((), 5, dtype=torch.int32)
    used, qa = st["used"].clone(), torch.ones(R)
    tail = (ntasks, qa, torch.full((R,), 1.0e9), ln, lc, ll, pl, jp)
    if static:
        ref.select_commit(score, cap, st["req"], ntasks, used, *tail[1:])
    else:
        ref.rescore_select_commit(
            st["alloc"], used, st["extra"], st["ready"], st["taints"],
            st["planes"], st["req"], 0, zw, zw, w_least, w_most, 0.0,
            st["dim_w"], bias, score, cap, *tail)
    m = int(ll)
    return ln[:m].tolist(), lc[:m].tolist(), used, qa, int(pl), int(jp)


def twins(n=3):
    one = torch.ones(n, 1)
    return dict(alloc=16 * one, used=0 * one, extra=0 * one,
                ready=torch.ones(n, dtype=torch.bool),
                taints=torch.zeros(n, dtype=torch.int64),
                planes=torch.zeros(n, 1, dtype=torch.int64),
                req=torch.ones(1), dim_w=torch.ones(1))


@pytest.mark.parametrize("ntasks, counts", [(3, [1, 1, 1]), (4, [2, 1, 1])])
def test_twin_nodes_take_turns(ntasks, counts):
    nodes, got, used, qa, placed, _ = run_select(twins(), ntasks)
    assert (nodes, got) == ([0, 1, 2], counts)
    assert used[:, 0].tolist() == [float(c) for c in counts]
    assert placed == ntasks and float(qa[0]) == 1.0 + ntasks


@pytest.mark.parametrize("N, R, ntasks", [(65, 1, 40), (300, 4, 700),
                                          (1025, 4, 1)])
def test_rising_scores_equal_the_static_fill(N, R, ntasks):
    """w_least = w_bal = 0: the chosen node's score never falls, so the
    sequential result is the static one, bit for bit."""
    st = kc.dyadic_state(N, R, 1, seed=N)
    a = run_select(st, ntasks, w_least=0.0, w_most=1.0, bias=st["bias"])
    b = run_select(st, ntasks, w_least=0.0, w_most=1.0, bias=st["bias"],
                   static=True)
    assert a[:2] == b[:2] and a[4:] == b[4:] and a[4] > 0
    assert kc.same_bits(a[2], b[2]) and kc.same_bits(a[3], b[3])


@pytest.mark.parametrize("exact, spread", [(True, [1, 1, 1]),
                                           (False, [0, 0, 3])])
def test_nodeorder_exact_spreads_a_job_over_twin_nodes(exact, spread):
    from volcano_amd.scheduler import (FakeBinder, Scheduler, SchedulerCache,
                                       default_config)
    from volcano_amd.scheduler.config import PluginOption
    from volcano_amd.store import ObjectStore
    from volcano_amd.utils import synth
    store, binder = ObjectStore(), FakeBinder()
    cache = SchedulerCache(store=store, binder=binder)
    config = default_config()
    config.tiers[1].plugins = [
        p for p in config.tiers[1].plugins
        if p.name not in ("nodeorder", "binpack")] + [PluginOption(
            "nodeorder", arguments={"balancedresource.weight": 0,
                                    **({"exact": True} if exact else {})})]
    for name in "abc":
        store.create("Node", synth.make_node(name, cpu_milli=8000,
                                             mem=64 << 30))
    store.create("Queue", synth.make_queue("default"))
    store.create("PodGroup", synth.make_podgroup("g", min_member=3))
    for i in range(3):
        store.create("Pod", synth.make_pod(f"g-w-{i}", "g", cpu_milli=1000,
                                           mem=1 << 30))
    Scheduler(cache, config).run_once()
    per_node = sorted(list(binder.binds.values()).count(n) for n in "abc")
    assert per_node == spread
