"""``numa_cap`` / ``numa_commit`` / ``numa_revert`` and the routing of NUMA
classes by ``vamd_run_cycle`` against the per-pod ``best_zone`` oracle.
Integers only: every comparison is equality."""

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
@pytest.mark.parametrize("Z", [1, 2, 3, 8])
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
                                 (8197, 8)])
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


@pytest.mark.parametrize("mode", ["default", "megacycle", "chain"])
def test_plans_with_numa_classes(monkeypatch, mode):
    for var in MODE_VARS:
        monkeypatch.delenv(var, raising=False)
    if mode == "megacycle":
        monkeypatch.setenv("VAMD_MEGACYCLE", "1")
    elif mode == "chain":
        monkeypatch.setenv("VAMD_CHAIN_CHUNK", "16")
    want, want_rows, want_cards, want_zones, want_plane = plan_oracle()
    plan, numa = nc.build_numa_plan(DEV)
    res = planmod.run_plan_hip(plan)
    kc.compare_results(want, kc.snapshot(plan, res))
    assert np.array_equal(want_rows, res.numa_assign)
    assert np.array_equal(want_cards, res.dev_assign)
    assert {c: res.class_zones(c) for c in numa} == want_zones
    assert np.array_equal(want_plane, plan.numa_plane.cpu().numpy())
