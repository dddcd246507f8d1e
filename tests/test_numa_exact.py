"""NUMA pinning per placement (``numaaware`` with ``exact: true``) on the
torch runner, and the closed form of the rule against the real per-pod
``NumaState.best_zone`` / ``take`` loop.  Integers only: every comparison
is equality."""

import numpy as np
import pytest
import torch

import _deviceshare_cases as dc
import _numa_cases as nc
from volcano_amd.api.objects import Numatopology, NumaZone, ObjectMeta
from volcano_amd.ops import reference as ref
from volcano_amd.scheduler.plugins.numaaware import (ANN_PINNED, ANN_POLICY,
                                                     NumaState)

GI = 1024 ** 3


def host_loop(zones, cpu, pods):
    """The real ledger, one pod at a time: (zone or None per pod, free)."""
    st = NumaState(Numatopology(meta=ObjectMeta(name="n"), zones=[
        NumaZone(z, f, GI) for z, f in enumerate(zones)]))
    seq = []
    for _ in range(pods):
        seq.append(st.best_zone(float(cpu)))
        if seq[-1] is not None:
            st.take(seq[-1], float(cpu))
    return seq, st.free


@pytest.mark.parametrize("cpu", nc.CPUS)
@pytest.mark.parametrize("zones", nc.ZONE_SETS, ids=str)
def test_closed_form_equals_per_pod_loop(zones, cpu):
    Z = len(zones)
    plane = torch.tensor(zones, dtype=torch.int32).reshape(Z, 1)
    slots = ref.numa_slots(plane, cpu)[:, 0]
    S = int(slots.sum())
    seq, _ = host_loop(zones, cpu, S + 1)
    # capacity: the host pins exactly S pods, the next one finds nothing
    assert seq[S] is None and None not in seq[:S]
    # fill order, for every m = 0 .. S + 1 at once: the pods of zone z among
    # the first m are clamp(m - prefix_z, 0, slots_z), prefix_z the slots
    # ranked before z in (free asc, index asc) among zones with slots
    order = sorted((z for z in range(Z) if slots[z] > 0),
                   key=lambda z: (zones[z], z))
    prefix = np.zeros(Z, dtype=np.int64)
    prefix[order] = np.cumsum([0] + [slots[z] for z in order[:-1]])
    m = np.arange(S + 2)[:, None]
    closed = np.clip(m - prefix[None, :], 0, slots[None, :])
    picks = np.array([[z == p for z in range(Z)] for p in seq]).reshape(-1, Z)
    host = np.concatenate([np.zeros((1, Z), np.int64), np.cumsum(picks, 0)])
    assert np.array_equal(closed, host)

    # the oracles the GPU tests compare against, at the edges of m: hard
    # (numa_cap admits min(cap, S)) and best-effort (pod S + 1 is unpinned)
    caps = [0, max(S - 1, 0), S, S + 1]
    cap = torch.tensor(caps, dtype=torch.int32)
    score = torch.where(cap > 0, 1.0, -np.inf)
    ref.numa_cap(score, cap, plane.repeat(1, 4).contiguous(), cpu)
    assert cap.tolist() == [min(c, S) for c in caps]
    assert (score > -np.inf).tolist() == [min(c, S) > 0 for c in caps]
    for pods in sorted({0, 1, max(S - 1, 0), S, S + 1}):
        live, row = plane.clone(), torch.zeros((1, Z), dtype=torch.int32)
        log = (torch.tensor([0], dtype=torch.int32),
               torch.tensor([pods], dtype=torch.int32), torch.tensor(1))
        ref.numa_commit(*log, live, row, cpu)
        want, free = host_loop(zones, cpu, pods)
        assert ref.numa_zones(row[0].numpy(), pods) == want
        assert live[:, 0].tolist() == free
        ref.numa_revert(0, log[0], log[2], live, row, cpu)
        assert torch.equal(live, plane) and not row.any()


# ---- the integer limits: values near 2^28 --------------------------------

def per_pod(case, cpu):
    """cap, rows and plane of the per-pod oracles on a commit case."""
    cap = torch.from_numpy(case["cap"].copy())
    ref.numa_cap(torch.from_numpy(case["score"].copy()), cap,
                 torch.from_numpy(case["zone_free"].copy()), cpu)
    plane = torch.from_numpy(case["zone_free"].copy())
    L = len(case["log_nodes"])
    rows = torch.zeros((L, plane.shape[0]), dtype=torch.int32)
    ref.numa_commit(torch.from_numpy(case["log_nodes"]),
                    torch.from_numpy(case["log_counts"]), torch.tensor(L),
                    plane, rows, cpu)
    return cap.numpy(), rows.numpy(), plane.numpy()


# nc.CPUS with 8000 for 9000 in the role "above every zone": scaled by 2^15
# a request must stay below 2^28, and 9000 * 2^15 does not
@pytest.mark.parametrize("policy", [nc.HARD, nc.SOFT])
@pytest.mark.parametrize("cpu", [1, 500, 2500, 8000])
@pytest.mark.parametrize("Z", [2, 4, 5, 8])
def test_per_pod_rule_is_scale_invariant(Z, cpu, policy):
    """The link between the closed form at large values and the per-pod
    rule: millicores scaled by 2^15 (7500 stays below 2^28) change no pick
    of ``best_zone``."""
    f = 1 << 15
    case = nc.commit_case(8, Z, cpu, policy, seed=Z)
    big = dict(case, zone_free=case["zone_free"] * f)
    assert big["zone_free"].dtype == np.int32 and \
        big["zone_free"].max() == 7500 * f < ref.NUMA_FREE_LIMIT
    cap, rows, plane = per_pod(case, cpu)
    cap_f, rows_f, plane_f = per_pod(big, cpu * f)
    assert np.array_equal(cap, cap_f) and np.array_equal(rows, rows_f)
    assert np.array_equal(plane.astype(np.int64) * f, plane_f)
    assert rows.any() == (cpu <= 7500)


@pytest.mark.parametrize("policy", [nc.HARD, nc.SOFT])
@pytest.mark.parametrize("name", list(nc.BIG_ZONE_CASES))
def test_big_cases_agree_on_python_integers(name, policy):
    """numpy's closed form and the plain-integer derivation agree, so no
    case of the family rests on a wrapped numpy value."""
    case, cpu, want = nc.big_zone_case(name, policy)
    got = nc.zone_closed_py(case, cpu)
    for key in nc.CLOSED_KEYS:
        assert want[key] == got[key], key
    Z = case["zone_free"].shape[0]
    assert any(any(row) for row in want["rows"])
    assert want["cap"] != case["cap"].tolist()          # the clamp bites
    assert all(0 < take <= nc.TOP and 0 <= zone < Z
               for run in want["runs"] for zone, take in run)
    assert min(min(col) for col in want["zone_free"]) >= 0
    S = ref.numa_slots(torch.from_numpy(case["zone_free"]), cpu).sum(0)
    pinned = [sum(t for _, t in run) for run in want["runs"]]
    counts = case["log_counts"].tolist()
    assert pinned == [min(c, int(S[n])) for n, c in
                      zip(case["log_nodes"].tolist(), counts)]
    assert (policy == nc.SOFT) == any(c > p for c, p in zip(counts, pinned))


def test_top_case_holds_the_figures_it_exists_for():
    TOP = nc.TOP
    case, cpu, want = nc.big_zone_case("top-Z8", nc.SOFT)
    S = ref.numa_slots(torch.from_numpy(case["zone_free"]), cpu).sum(0)
    assert S[0] == 2 ** 31 - 8 and S[1] == 2 ** 31 - 8 - 28
    assert case["cap"][0] == nc.INT_MAX and want["cap"][0] == 2 ** 31 - 8
    counts = case["log_counts"].tolist()
    assert counts[0] == S[0] + 2 and counts[1] == nc.INT_MAX
    # all keys tie: zones 0 .. 7 in turn, each to the brim
    assert want["rows"][0] == [z << 28 | TOP for z in range(8)]
    # free[z] = top - z: zones 7 .. 0
    assert want["runs"][3] == [(z, TOP - z) for z in range(7, -1, -1)]
    assert not any(want["zone_free"][z][0] for z in range(8))
    case, cpu, want = nc.big_zone_case("top-Z8", nc.HARD)
    assert case["log_counts"][1] == S[0] - 1
    assert want["runs"][1][7] == (7, TOP - 1)
    case, cpu, want = nc.big_zone_case("one-slot-Z5", nc.HARD)
    slots = ref.numa_slots(torch.from_numpy(case["zone_free"]), cpu)
    assert cpu == TOP and slots.max() == 1
    assert not slots[case["zone_free"] == TOP - 1].any()
    assert slots[case["zone_free"] == TOP].all()


@pytest.mark.parametrize("mutant", dc.MUTANTS)
def test_every_wrong_kernel_fails_a_big_case(mutant):
    """The three wrong kernels a legitimate zone plane can tell from the
    right one are caught by the big family; the 24-bit mask passes the
    small-value family.  The int32 wraps and the decode that shifts the
    int32 are the right kernel here (S <= 8 (2^28 - 1) < 2^31, one slot per
    pod, zone << 28 never reaches bit 31): asserted, so that the list
    changes with the limits."""
    killed = {}
    for name in nc.BIG_ZONE_CASES:
        for policy in (nc.HARD, nc.SOFT):
            case, cpu, want = nc.big_zone_case(name, policy)
            got = nc.zone_closed_py(case, cpu, mutant)
            keys = [k for k in nc.CLOSED_KEYS if want[k] != got[k]]
            if keys:
                killed[name, policy] = keys
    print(mutant, "caught by", killed)
    assert bool(killed) == (mutant in nc.MUTANTS), mutant
    if mutant != "mask-24":
        return
    for Z in (1, 2, 3, 8):
        for cpu in nc.CPUS:
            case = nc.commit_case(20, Z, cpu, nc.SOFT, seed=Z)
            want = nc.zone_closed(case, cpu)
            got = nc.zone_closed_py(case, cpu, mutant)
            assert all(want[k] == got[k] for k in nc.CLOSED_KEYS), (Z, cpu)
            assert np.array_equal(per_pod(case, cpu)[1].view(np.uint32),
                                  np.array(want["rows"], dtype=np.uint32))
    print(mutant, "passes the small-value family")


def run_cluster(policy, nodes, exact=True):
    """Three 2500 m pods of one gang on ``nodes`` = {name: zone sizes}; the
    aggregate cpu of the first node admits all three.  Returns (binds,
    {pod: pinned zone or None}, {node: zone free})."""
    from volcano_amd.scheduler import (FakeBinder, Scheduler, SchedulerCache,
                                       default_config)
    from volcano_amd.scheduler.config import PluginOption
    from volcano_amd.store import ObjectStore
    from volcano_amd.utils import synth
    store, binder = ObjectStore(), FakeBinder()
    cache = SchedulerCache(store=store, binder=binder)
    config = default_config()
    config.tiers[1].plugins.append(PluginOption(
        "numaaware", arguments={"exact": exact}))
    sched = Scheduler(cache, config)
    for name, zones in nodes.items():
        store.create("Node", synth.make_node(name, cpu_milli=sum(zones),
                                             mem=64 * GI))
        store.create("Numatopology", Numatopology(
            meta=ObjectMeta(name=name),
            zones=[NumaZone(z, f, 16 * GI) for z, f in enumerate(zones)]))
    store.create("Queue", synth.make_queue("default"))
    store.create("PodGroup", synth.make_podgroup("g", min_member=3))
    for i in range(3):
        pod = synth.make_pod(f"g-w-{i}", "g", cpu_milli=2500, mem=GI)
        pod.meta.annotations[ANN_POLICY] = policy
        store.create("Pod", pod)
    sched.run_once()
    pins = {k.split("/")[1]: t.pod.meta.annotations.get(ANN_PINNED)
            for k, t in cache.jobs["default/g"].tasks.items()}
    binds = {k.split("/")[1]: v for k, v in binder.binds.items()}
    free = {n: st.free for n, st in cache._numa_states.items()}
    return binds, pins, free


def test_exact_pins_every_pod_of_a_gang_in_one_cycle():
    binds, pins, free = run_cluster(
        "single-numa-node", {"a": [4000, 4000], "b": [4000]})
    assert len(binds) == 3
    assert all(pins[p] is not None for p in binds), pins
    assert min(f for zs in free.values() for f in zs) >= 0
    assert list(binds.values()).count("a") <= 2
    assert sum(sum(zs) for zs in free.values()) == 12000 - 3 * 2500


def test_exact_best_effort_pins_what_fits():
    binds, pins, free = run_cluster("best-effort", {"a": [4000, 4000]})
    assert binds == {f"g-w-{i}": "a" for i in range(3)}
    assert sorted(p is not None for p in pins.values()) == [False, True, True]
    assert free == {"a": [1500, 1500]}
