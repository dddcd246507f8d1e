"""``device_cap`` / ``device_commit`` / ``device_revert`` and the routing of
device classes by ``vamd_run_cycle`` against the per-pod ``GPUDevicePool``
oracle and, at values that oracle cannot walk, against the closed form.
Integers only: every comparison is equality."""

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
@pytest.mark.parametrize("K", [1, 3, 4, 5, 8, 9, 16])
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
                                 (4099, 16), (6, 4), (7, 5), (10, 9)])
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


@pytest.mark.parametrize("name", list(dc.BIG_CARD_CASES))
def test_device_cap_at_the_integer_limits(name):
    """Values near 2^28 and S above int32 (and the over-full cards) against
    the closed form, which tests/test_deviceshare_exact.py pins to plain
    integers and, by scale invariance, to the per-pod rule."""
    from volcano_amd.ops import hip
    case, request_, want = dc.big_card_case(name)
    got = [_d(case["score"]), _d(case["cap"])]
    hip.device_cap(*got, *dc.planes_of(case, DEV), request_)
    score, cap = (g.cpu().numpy() for g in got)
    assert np.array_equal(want["score"].view(np.int32), score.view(np.int32))
    assert want["cap"] == cap.tolist()
    assert ((cap > 0) == (score > -np.inf)).all()


@pytest.mark.parametrize("name", list(dc.BIG_CARD_CASES))
def test_device_commit_then_revert_at_the_integer_limits(name):
    from volcano_amd.ops import hip
    case, request_, want = dc.big_card_case(name)
    L, K = len(case["log_nodes"]), case["state"].shape[0]
    # the log slot is longer than the log: the tail must stay untouched
    pad = np.zeros(3, dtype=np.int32)
    nodes = np.concatenate([case["log_nodes"], pad])
    counts = np.concatenate([case["log_counts"], pad + 1])
    want_rows = np.array(want["rows"] + [[7] * K] * 3, dtype=np.uint32)
    want_planes = [np.array(want[k], dtype=np.int32)
                   for k in ("mem_used", "cores_used", "state")]
    got = dc.planes_of(case, DEV)
    rows = torch.full((L + 3, K), 7, dtype=torch.int32, device=DEV)
    log = (_d(nodes), _d(counts), _d(np.array([L], dtype=np.int32)))

    def check(planes, words):
        for w, g in zip(planes + [case["mem_total"]], got):
            assert np.array_equal(w, g.cpu().numpy())
        assert np.array_equal(words, rows.cpu().numpy().view(np.uint32))

    hip.device_commit(*log, *got, rows, request_)
    check(want_planes, want_rows)
    keep, drop = (_d(np.array([f], dtype=np.uint8)) for f in (1, 0))
    hip.device_revert(keep, log[0], log[2], *got, rows, request_)
    check(want_planes, want_rows)
    hip.device_revert(drop, log[0], log[2], *got, rows, request_)
    want_rows[:L] = 0
    check([case[k] for k in ("mem_used", "cores_used", "state")], want_rows)


def test_device_cap_grid_stride_wraps():
    """One node more than a wave past 4096 blocks of 256: the tail is
    reached only by the second trip of the grid-stride loop."""
    from volcano_amd.ops import hip
    stride, request_ = 4096 * 256, (2, 100, 40)
    case = dc.card_case(stride + 65, 2, seed=2)
    want = [torch.from_numpy(case[k].copy()) for k in ("score", "cap")]
    ref.device_cap_closed(*want, *dc.planes_of(case), request_)
    score, cap = (w.numpy() for w in want)
    # non-vacuous: the clamp changes cap and score past the first stride
    assert (cap[stride:] != case["cap"][stride:]).any()
    assert (score[stride:] != case["score"][stride:]).any()
    got = [_d(case["score"]), _d(case["cap"])]
    hip.device_cap(*got, *dc.planes_of(case, DEV), request_)
    assert np.array_equal(score.view(np.int32),
                          got[0].cpu().numpy().view(np.int32))
    assert np.array_equal(cap, got[1].cpu().numpy())


@functools.lru_cache(maxsize=None)
def plan_oracle16():
    """run_plan_torch on the device plan over sixteen cards: computed once,
    never modified."""
    plan, requests = dc.build_device_plan("cpu", 16)
    res = planmod.run_plan_torch(plan)
    snap = kc.snapshot(plan, res)
    cards = {c: res.class_cards(c) for c in requests}
    planes = [plan.device_planes[k].numpy() for k in
              ("mem_used", "cores_used", "state")]
    # non-vacuous: words with the sign bit set (cards 8 to 15), in single-
    # and multi-slice classes, a whole-card class among them
    rows = np.asarray(res.dev_assign)
    assert rows.dtype == np.int32 and (rows < 0).any()
    high = {c for c in requests if any(k >= 8 for pod in cards[c]
                                       for k in pod)}
    assert {0, 1, 5, 44} <= high
    assert all(len(cards[c]) == snap["class_placed"][c] for c in requests)
    return snap, res.dev_assign, cards, planes


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


def _run_plan(monkeypatch, mode, oracle, K):
    for var in MODE_VARS:
        monkeypatch.delenv(var, raising=False)
    if mode == "megacycle":
        monkeypatch.setenv("VAMD_MEGACYCLE", "1")
    elif mode == "chain":
        monkeypatch.setenv("VAMD_CHAIN_CHUNK", "16")
    want, want_rows, want_cards, want_planes = oracle()
    plan, requests = dc.build_device_plan(DEV, K)
    res = planmod.run_plan_hip(plan)
    kc.compare_results(want, kc.snapshot(plan, res))
    assert np.array_equal(want_rows, res.dev_assign)
    assert {c: res.class_cards(c) for c in requests} == want_cards
    for name, w in zip(("mem_used", "cores_used", "state"), want_planes):
        assert np.array_equal(w, plan.device_planes[name].cpu().numpy()), name


@pytest.mark.parametrize("mode", ["default", "megacycle", "chain"])
def test_plans_with_device_classes(monkeypatch, mode):
    _run_plan(monkeypatch, mode, plan_oracle, 4)


@pytest.mark.parametrize("mode", ["default", "megacycle", "chain"])
def test_plans_with_device_classes_on_sixteen_cards(monkeypatch, mode):
    """Words with the sign bit set through the whole cycle and the host's
    decode (``class_cards``)."""
    _run_plan(monkeypatch, mode, plan_oracle16, 16)
