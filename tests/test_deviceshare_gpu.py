"""``device_cap`` / ``device_commit`` / ``device_revert`` and the routing of
device classes by ``vamd_run_cycle`` against the per-pod ``GPUDevicePool``
oracle.  Integers only: every comparison is equality."""

import functools

import numpy as np
import pytest
import torch

import _deviceshare_cases as dc
import _kernel_cases as kc
from volcano_amd.ops import reference as ref
from volcano_amd.scheduler import plan as planmod

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODE_VARS = ("VAMD_MEGACYCLE", "VAMD_CHAIN_CHUNK", "VAMD_NO_CHAIN")


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same(want, got):
    for w, g in zip(want, got):
        assert np.array_equal(w.cpu().numpy(), g.cpu().numpy())


@pytest.mark.parametrize("request_", dc.REQUESTS, ids=str)
@pytest.mark.parametrize("K", [1, 3, 8, 16])
@pytest.mark.parametrize("N", [1, 63, 65, 1025])
def test_device_cap(N, K, request_):
    from volcano_amd.ops import hip
    case = dc.card_case(N, K, seed=N + K)
    want = [torch.from_numpy(case[k].copy()) for k in ("score", "cap")]
    ref.device_cap(*want, *dc.planes_of(case), request_)
    got = [_d(case["score"]), _d(case["cap"])]
    hip.device_cap(*got, *dc.planes_of(case, DEV), request_)
    assert np.array_equal(want[0].numpy().view(np.int32),
                          got[0].cpu().numpy().view(np.int32))
    assert np.array_equal(want[1].numpy(), got[1].cpu().numpy())
    assert ((got[1] > 0) == (got[0] > -np.inf)).all()


@pytest.mark.parametrize("request_", dc.REQUESTS, ids=str)
@pytest.mark.parametrize("L,K", [(1, 3), (4, 16), (5, 1), (67, 8),
                                 (4099, 16)])
def test_device_commit_then_revert(L, K, request_):
    from volcano_amd.ops import hip
    case = dc.commit_case(L, K, request_, seed=L)
    # the log slot is longer than the log: the tail must stay untouched
    pad = np.zeros(3, dtype=np.int32)
    nodes = np.concatenate([case["log_nodes"], pad])
    counts = np.concatenate([case["log_counts"], pad + 1])
    want = dc.planes_of(case)
    want_rows = torch.zeros((L + 3, K), dtype=torch.int32)
    ref.device_commit(torch.from_numpy(nodes), torch.from_numpy(counts),
                      torch.tensor(L), *want, want_rows, request_)
    got = dc.planes_of(case, DEV)
    rows = torch.zeros((L + 3, K), dtype=torch.int32, device=DEV)
    log = (_d(nodes), _d(counts), _d(np.array([L], dtype=np.int32)))
    hip.device_commit(*log, *got, rows, request_)
    _same(want + [want_rows], got + [rows])
    assert want_rows.any() == bool(case["log_counts"].any())

    keep, drop = (_d(np.array([f], dtype=np.uint8)) for f in (1, 0))
    hip.device_revert(keep, log[0], log[2], *got, rows, request_)
    _same(want + [want_rows], got + [rows])
    hip.device_revert(drop, log[0], log[2], *got, rows, request_)
    _same(dc.planes_of(case) + [torch.zeros_like(want_rows)], got + [rows])


@functools.lru_cache(maxsize=None)
def plan_oracle():
    """run_plan_torch on the device plan: computed once, never modified."""
    plan, requests = dc.build_device_plan("cpu")
    res = planmod.run_plan_torch(plan)
    snap = kc.snapshot(plan, res)
    cards = {c: res.class_cards(c) for c in requests}
    planes = [plan.device_planes[k].numpy() for k in
              ("mem_used", "cores_used", "state")]
    # non-vacuous: the gang that cannot fit, the discarded multi-class job
    # (whose device class had placed), the kept one, both domain rules
    placed, flag = snap["class_placed"], snap["job_flag"]
    assert placed[0] > 0 and placed[1] > 0 and placed[2] == 0
    assert flag[3] == 0 and flag[4] == 1 and placed[5] > 0 and placed[6] > 0
    assert placed[7] > 0 and placed[8] == 6
    assert all(len(cards[c]) == placed[c] for c in requests)
    return snap, res.dev_assign, cards, planes


@pytest.mark.parametrize("mode", ["default", "megacycle", "chain"])
def test_plans_with_device_classes(monkeypatch, mode):
    for var in MODE_VARS:
        monkeypatch.delenv(var, raising=False)
    if mode == "megacycle":
        monkeypatch.setenv("VAMD_MEGACYCLE", "1")
    elif mode == "chain":
        monkeypatch.setenv("VAMD_CHAIN_CHUNK", "16")
    want, want_rows, want_cards, want_planes = plan_oracle()
    plan, requests = dc.build_device_plan(DEV)
    res = planmod.run_plan_hip(plan)
    kc.compare_results(want, kc.snapshot(plan, res))
    assert np.array_equal(want_rows, res.dev_assign)
    assert {c: res.class_cards(c) for c in requests} == want_cards
    for name, w in zip(("mem_used", "cores_used", "state"), want_planes):
        assert np.array_equal(w, plan.device_planes[name].cpu().numpy()), name
