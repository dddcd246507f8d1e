"""``numa_cap`` / ``numa_commit`` / ``numa_revert`` and the routing of NUMA
classes by ``vamd_run_cycle`` against the per-pod ``best_zone`` oracle and,
at values that oracle cannot walk, against the closed form.  Integers only:
every comparison is equality."""

import functools

import numpy as np
import pytest
import torch

import _kernel_cases as kc
import _numa_cases as nc
from volcano_amd.ops import reference as ref
from volcano_amd.scheduler import plan as planmod

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODE_VARS = ("VAMD_MEGACYCLE", "VAMD_CHAIN_CHUNK", "VAMD_NO_CHAIN")


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize("cpu", nc.CPUS)
@pytest.mark.parametrize("Z", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("N", [1, 63, 65, 1025])
def test_numa_cap(N, Z, cpu):
    from volcano_amd.ops import hip
    case = nc.zone_case(N, Z, seed=N + Z)
    want = [torch.from_numpy(case[k].copy()) for k in ("score", "cap")]
    ref.numa_cap(*want, torch.from_numpy(case["zone_free"]), cpu)
    got = [_d(case["score"]), _d(case["cap"])]
    hip.numa_cap(*got, _d(case["zone_free"]), cpu)
    score, cap = (g.cpu().numpy() for g in got)
    assert np.array_equal(want[0].numpy().view(np.int32), score.view(np.int32))
    assert np.array_equal(want[1].numpy(), cap)
    assert ((cap > 0) == (score > -np.inf)).all()
    # nodes that entered with cap == 0 are untouched, whatever their score
    assert not cap[case["cap"] == 0].any()


@pytest.mark.parametrize("policy", [nc.HARD, nc.SOFT])
@pytest.mark.parametrize("cpu", nc.CPUS)
@pytest.mark.parametrize("L,Z", [(1, 2), (8, 8), (9, 3), (67, 8),
                                 (8197, 8), (6, 4), (7, 5)])
def test_numa_commit_then_revert(L, Z, cpu, policy):
    from volcano_amd.ops import hip
    case = nc.commit_case(L, Z, cpu, policy, seed=L)
    if policy == nc.SOFT:
        assert case["log_counts"][0] > case["slots"][case["log_nodes"][0]]
    # the log slot is longer than the log: the tail must stay untouched
    pad = np.zeros(3, dtype=np.int32)
    nodes = np.concatenate([case["log_nodes"], pad])
    counts = np.concatenate([case["log_counts"], pad + 1])
    want = torch.from_numpy(case["zone_free"].copy())
    want_rows = torch.full((L + 3, Z), 7, dtype=torch.int32)
    ref.numa_commit(torch.from_numpy(nodes), torch.from_numpy(counts),
                    torch.tensor(L), want, want_rows, cpu)
    got = _d(case["zone_free"])
    rows = torch.full((L + 3, Z), 7, dtype=torch.int32, device=DEV)
    log = (_d(nodes), _d(counts), _d(np.array([L], dtype=np.int32)))
    hip.numa_commit(*log, got, rows, cpu)
    assert torch.equal(want, got.cpu()) and torch.equal(want_rows, rows.cpu())
    assert (want_rows[L:] == 7).all()

    keep, drop = (_d(np.array([f], dtype=np.uint8)) for f in (1, 0))
    hip.numa_revert(keep, log[0], log[2], got, rows, cpu)
    assert torch.equal(want, got.cpu()) and torch.equal(want_rows, rows.cpu())
    hip.numa_revert(drop, log[0], log[2], got, rows, cpu)
    assert np.array_equal(case["zone_free"], got.cpu().numpy())
    assert not rows[:L].any() and (rows[L:] == 7).all()


@pytest.mark.parametrize("policy", [nc.HARD, nc.SOFT])
@pytest.mark.parametrize("name", list(nc.BIG_ZONE_CASES))
def test_numa_cap_at_the_integer_limits(name, policy):
    """free and cpu near 2^28, S = 2^31 - 8, against the closed form, which
    tests/test_numa_exact.py pins to plain integers and, by scale
    invariance, to the per-pod rule.  (The policy only picks the log, which
    the cap does not read: both planes are the same.)"""
    from volcano_amd.ops import hip
    case, cpu, want = nc.big_zone_case(name, policy)
    got = [_d(case["score"]), _d(case["cap"])]
    hip.numa_cap(*got, _d(case["zone_free"]), cpu)
    score, cap = (g.cpu().numpy() for g in got)
    assert np.array_equal(want["score"].view(np.int32), score.view(np.int32))
    assert want["cap"] == cap.tolist()
    assert ((cap > 0) == (score > -np.inf)).all()


@pytest.mark.parametrize("policy", [nc.HARD, nc.SOFT])
@pytest.mark.parametrize("name", list(nc.BIG_ZONE_CASES))
def test_numa_commit_then_revert_at_the_integer_limits(name, policy):
    from volcano_amd.ops import hip
    case, cpu, want = nc.big_zone_case(name, policy)
    L, Z = len(case["log_nodes"]), case["zone_free"].shape[0]
    # the log slot is longer than the log: the tail must stay untouched
    pad = np.zeros(3, dtype=np.int32)
    nodes = np.concatenate([case["log_nodes"], pad])
    counts = np.concatenate([case["log_counts"], pad + 1])
    want_rows = np.array(want["rows"] + [[7] * Z] * 3, dtype=np.uint32)
    want_free = np.array(want["zone_free"], dtype=np.int32)
    got = _d(case["zone_free"])
    rows = torch.full((L + 3, Z), 7, dtype=torch.int32, device=DEV)
    log = (_d(nodes), _d(counts), _d(np.array([L], dtype=np.int32)))

    def check(free, words):
        assert np.array_equal(free, got.cpu().numpy())
        assert np.array_equal(words, rows.cpu().numpy().view(np.uint32))

    hip.numa_commit(*log, got, rows, cpu)
    check(want_free, want_rows)
    keep, drop = (_d(np.array([f], dtype=np.uint8)) for f in (1, 0))
    hip.numa_revert(keep, log[0], log[2], got, rows, cpu)
    check(want_free, want_rows)
    hip.numa_revert(drop, log[0], log[2], got, rows, cpu)
    want_rows[:L] = 0
    check(case["zone_free"], want_rows)


def test_numa_cap_grid_stride_wraps():
    """One node more than a wave past 4096 blocks of 256: the tail is
    reached only by the second trip of the grid-stride loop."""
    from volcano_amd.ops import hip
    stride, cpu = 4096 * 256, 2500
    case = nc.zone_case(stride + 65, 2, seed=2)
    score, cap = case["score"].copy(), case["cap"].copy()
    nc.numa_cap_closed(score, cap, case["zone_free"], cpu)
    # non-vacuous: the clamp changes cap and score past the first stride
    assert (cap[stride:] != case["cap"][stride:]).any()
    assert (score[stride:] != case["score"][stride:]).any()
    got = [_d(case["score"]), _d(case["cap"])]
    hip.numa_cap(*got, _d(case["zone_free"]), cpu)
    assert np.array_equal(score.view(np.int32),
                          got[0].cpu().numpy().view(np.int32))
    assert np.array_equal(cap, got[1].cpu().numpy())


@functools.lru_cache(maxsize=None)
def plan_oracle8():
    """run_plan_torch on the NUMA plan over eight zones: computed once,
    never modified."""
    plan, numa = nc.build_numa_plan("cpu", 8)
    res = planmod.run_plan_torch(plan)
    snap = kc.snapshot(plan, res)
    zones = {c: res.class_zones(c) for c in numa}
    # non-vacuous: hard and best-effort classes pin into zones 4 to 7, and
    # the rows hold those zones in their upper bits
    rows = np.asarray(res.numa_assign).view(np.uint32)
    assert (rows >> ref.NUMA_TAKE_BITS >= 4).any()
    high = {c for c in numa if any(z is not None and z >= 4
                                   for z in zones[c])}
    assert {0, 1, 2, 5} <= high and None in zones[1]
    assert all(len(zones[c]) == snap["class_placed"][c] for c in numa)
    assert not np.array_equal(plan.numa_plane.numpy(), plan.numa_state)
    return snap, res.numa_assign, res.dev_assign, zones, \
        plan.numa_plane.numpy()


@functools.lru_cache(maxsize=None)
def plan_oracle():
    """run_plan_torch on the NUMA plan: computed once, never modified."""
    plan, numa = nc.build_numa_plan("cpu")
    res = planmod.run_plan_torch(plan)
    snap = kc.snapshot(plan, res)
    zones = {c: res.class_zones(c) for c in numa}
    # non-vacuous: the gang that fits and the one that cannot, the
    # best-effort class with pinned and unpinned pods, the discarded
    # multi-class job and the kept one, both domain rules, the class with
    # both requests
    placed, flag = snap["class_placed"], snap["job_flag"]
    assert placed[0] == 40 and placed[1] > 0 and placed[2] == 0
    assert None in zones[1] and 0 in zones[1] and None not in zones[0]
    assert flag[3] == 0 and flag[4] == 1 and placed[5] > 0 and placed[6] > 0
    assert placed[7] > 0 and placed[8] == 6 and placed[9] > 0
    assert res.dev_assign[plan.classes[9].log_off].any()
    assert all(len(zones[c]) == placed[c] for c in numa)
    assert not np.array_equal(plan.numa_plane.numpy(), plan.numa_state)
    return snap, res.numa_assign, res.dev_assign, zones, \
        plan.numa_plane.numpy()


def _run_plan(monkeypatch, mode, oracle, Z):
    for var in MODE_VARS:
        monkeypatch.delenv(var, raising=False)
    if mode == "megacycle":
        monkeypatch.setenv("VAMD_MEGACYCLE", "1")
    elif mode == "chain":
        monkeypatch.setenv("VAMD_CHAIN_CHUNK", "16")
    want, want_rows, want_cards, want_zones, want_plane = oracle()
    plan, numa = nc.build_numa_plan(DEV, Z)
    res = planmod.run_plan_hip(plan)
    kc.compare_results(want, kc.snapshot(plan, res))
    assert np.array_equal(want_rows, res.numa_assign)
    assert np.array_equal(want_cards, res.dev_assign)
    assert {c: res.class_zones(c) for c in numa} == want_zones
    assert np.array_equal(want_plane, plan.numa_plane.cpu().numpy())


@pytest.mark.parametrize("mode", ["default", "megacycle", "chain"])
def test_plans_with_numa_classes(monkeypatch, mode):
    _run_plan(monkeypatch, mode, plan_oracle, 3)


@pytest.mark.parametrize("mode", ["default", "megacycle", "chain"])
def test_plans_with_numa_classes_on_eight_zones(monkeypatch, mode):
    _run_plan(monkeypatch, mode, plan_oracle8, 8)
