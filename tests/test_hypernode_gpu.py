"""Mode 3 of ``vamd_domain_mask`` (network-topology domain choice) against
``reference.hypernode_mask``: score and cap bit for bit, then the log,
counters and usage of the select that follows; and its routing by
``vamd_run_cycle``.  Everything is integer or exact in f32: no tolerance."""

import numpy as np
import pytest
import torch

import _affinity_cases as ac
import _hypernode_cases as hc
from volcano_amd.ops import hip
from volcano_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

DEV = "cuda"
BIG = 1.0e18
SHAPES = [(63, 1, 1), (65, 3, 2), (1025, 65, 3), (2049, 2049, 2),
          (hip.HYPERNODE_LDS_LEAVES + 1, hip.HYPERNODE_LDS_LEAVES + 1, 2)]
NEEDS = ["one", "tight", "tight+1", "all+1"]


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def select(score, cap, ntasks, dev, bulk):
    """select_commit over one resource dim -> (log, counters, used)."""
    N = score.shape[0]
    K = min(ntasks, N)
    t = lambda *a, **k: torch.zeros(*a, device=dev, **k)
    req = torch.ones(1, device=dev)
    ql = torch.full((1,), BIG, device=dev)
    ln, lc = t(K, dtype=torch.int32), t(K, dtype=torch.int32)
    ll, placed, jp = (t(1, dtype=torch.int32) for _ in range(3))
    if dev == "cpu":
        used = t(N, 1)
        ref.select_commit(score, cap, req, ntasks, used, t(1), ql, ln, lc,
                          ll[0], placed[0], jp[0])
    else:
        used = t(1, N)
        hip.select_commit(score, cap, req, ntasks, used, t(1), ql, ln, lc,
                          ll, placed, jp, -1,
                          torch.empty(4 * N, dtype=torch.int32, device=dev)
                          if bulk else None)
    n = int(ll)
    return (ln[:n].tolist(), lc[:n].tolist(), int(placed), int(jp),
            used.flatten().tolist())


def check(score, cap, leaf_of, table, D):
    """Mask, then the serial and (N >= 512) the sort-based select."""
    N = score.shape[0]
    want_s, want_c = torch.from_numpy(score.copy()), torch.from_numpy(cap.copy())
    ref.hypernode_mask(want_s, want_c, torch.from_numpy(leaf_of),
                       torch.from_numpy(table), D)
    for ntasks in (5, 600) if N >= 512 else (5,):
        got_s, got_c = _d(score.copy()), _d(cap.copy())
        hip.hypernode_mask(got_s, got_c, _d(leaf_of), _d(table), D)
        assert np.array_equal(got_s.cpu().numpy().view(np.int32),
                              want_s.numpy().view(np.int32))
        assert got_c.cpu().tolist() == want_c.tolist()
        assert select(got_s, got_c, ntasks, DEV, ntasks >= 512) == \
            select(want_s.clone(), want_c.clone(), ntasks, "cpu", False)


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("pin", [False, True], ids=["nopin", "pin"])
@pytest.mark.parametrize("need", NEEDS)
@pytest.mark.parametrize("N,D,T", SHAPES)
def test_mask_and_select_equal_the_oracle(N, D, T, need, pin, soft):
    interleaved = (NEEDS.index(need) + pin + soft) % 2 == 0
    score, cap, leaf_of, tiers = hc.kernel_case(N, D, T,
                                                interleaved=interleaved)
    check(score, cap, leaf_of,
          hc.table_for(need, cap, leaf_of, tiers, D, pin=pin, soft=soft), D)


@pytest.mark.parametrize("N,D,T", SHAPES[1:])
def test_equal_capacities_go_to_the_lower_index(N, D, T):
    score, cap, leaf_of, tiers = hc.kernel_case(N, D, T, interleaved=True,
                                                caps="equal")
    L = hc.leaf_caps(cap, leaf_of, D)
    assert len(set(L)) == 1
    check(score, cap, leaf_of, ref.hypernode_table(tiers, L[0], D), D)


def test_leaf_sums_do_not_wrap():
    score, cap, leaf_of, table = hc.huge_case()
    check(score, cap, leaf_of, table, 2)


def test_argument_checks():
    score, cap, leaf_of, tiers = hc.kernel_case(65, 3, 2, interleaved=True)
    table = ref.hypernode_table(tiers, 1, 3)
    args = [_d(score), _d(cap), _d(leaf_of), _d(table), 3]
    for at, bad in ((2, _d(leaf_of[:-1])), (2, _d(leaf_of.astype(np.int64))),
                    (4, 66), (3, _d(np.r_[0, table[1:]].astype(np.int32))),
                    (3, _d(np.r_[table[0], 0, table[2:]].astype(np.int32)))):
        call = list(args)
        call[at] = bad
        with pytest.raises(ValueError):
            hip.hypernode_mask(*call)


@pytest.mark.parametrize("scenario", ["two-gangs", "fragmented"])
def test_scenarios_on_the_hip_plane(scenario):
    want = hc.schedule(scenario, "cpu")
    assert len(want) == (8 if scenario == "two-gangs" else 2)
    assert hc.schedule(scenario, "cuda") == want


def mixed_plan(device, N):
    """The affinity plan (affinity, anti, spread, plain, a chain run) with
    single-class plain jobs turned into hypernode classes: the first two
    and two of the last of the small jobs, and — so that one hard miss
    reverts in the select — one whose need nothing can hold."""
    case = ac.affinity_plan_case(N=N)
    plan = ac.build_affinity_plan(case, device)
    D = 16
    leaf_of = (np.arange(N) * D // N).astype(np.int32)
    leaf_of[::9] = -1
    row = plan.add_hypernode_row(leaf_of, D)
    tiers = [[(l, l + 1) for l in range(D)], [(0, 8), (8, 16)], [(0, 16)]]
    C = len(plan.classes)
    for k, c in enumerate((2, 3, C - 2, C - 1)):
        jp = next(j for j in plan.jobs if j.class_begin == c)
        assert jp.class_end == c + 1
        need = 10 ** 9 if k == 1 else max(1, jp.min_available)
        plan.classes[c].hypernode = plan.add_hypernode_group(
            row, ref.hypernode_table(tiers[:1 + k % 3], need, D,
                                     soft=k == 3))
    return plan


@pytest.mark.parametrize("N", [65, 1500])
@pytest.mark.parametrize("mode", [{}, {"VAMD_MEGACYCLE": 1},
                                  {"VAMD_CHAIN_CHUNK": 8}],
                         ids=["default", "megacycle", "chain8"])
def test_plan_mixing_hypernode_spread_and_affinity(monkeypatch, mode, N):
    from volcano_amd.scheduler.plan import run_plan_hip, run_plan_torch
    for var in ("VAMD_MEGACYCLE", "VAMD_CHAIN_CHUNK", "VAMD_NO_CHAIN"):
        monkeypatch.delenv(var, raising=False)
    oracle = mixed_plan("cpu", N)
    want = ac.plan_snapshot(oracle, run_plan_torch(oracle))
    hyper = [c for c, cp in enumerate(oracle.classes)
             if cp.hypernode is not None]
    placed = [int(want["class_placed"][c]) for c in hyper]
    assert placed[1] == 0 and sum(p > 0 for p in placed) >= 2
    for var, val in mode.items():
        monkeypatch.setenv(var, str(val))
    plan = mixed_plan(DEV, N)
    got = ac.plan_snapshot(plan, run_plan_hip(plan))
    torch.cuda.synchronize()
    ac.compare_plans(want, got)
