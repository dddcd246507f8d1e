"""``rescore_select`` and its routing in ``vamd_run_cycle`` against the
oracle (``reference.rescore_select_commit``), bit for bit: log, ``log_len``,
counters, ``used`` and ``queue_alloc``."""

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
WEIGHTS = {"least": (1.0, 0.0, False), "most": (0.0, 1.0, False),
           "both+bias": (2.0, 0.5, True)}


def run_both(st, ntasks, w_least, w_most, w_bal=0.0, bias=None, K=None,
             limit=1.0e9, fuse_min=-1, inexact=False, static=False):
    """One select on the device and in the oracle -> (want, got), each
    (nodes, counts, log_len, placed, job_placed, used, queue_alloc)."""
    from volcano_amd.ops import hip
    N, R = st["alloc"].shape
    W = st["planes"].shape[1]
    K = max(1, min(ntasks, N)) if K is None else K
    zw = torch.zeros(W, dtype=torch.int64)
    ql = torch.full((R,), float(limit))
    planes = dict(alloc=st["alloc"], used=st["used"], extra=st["extra"],
                  pl=st["planes"])
    d = {k: v.t().contiguous().to(DEV) for k, v in planes.items()}
    fixed = {k: st[k].to(DEV) for k in ("taints", "req", "dim_w")}
    ready = st["ready"].to(torch.uint8).to(DEV)
    bias_d = None if bias is None else bias.to(DEV)
    score_d = torch.empty(N, device=DEV)
    cap_d = torch.empty(N, dtype=torch.int32, device=DEV)

    def device_score(used_t):
        hip.score_cap(d["alloc"], used_t, d["extra"], ready, fixed["taints"],
                      d["pl"], fixed["req"], 0, zw.to(DEV), zw.to(DEV),
                      w_least, w_most, w_bal, fixed["dim_w"], bias_d, score_d,
                      cap_d)

    device_score(d["used"])
    if inexact:
        # the oracle runs on the kernel's own score bits
        score, cap = score_d.cpu(), cap_d.cpu()

        def score_fn(n, k):
            used_k = d["used"].clone()
            used_k[:, n] += float(k) * fixed["req"]     # integers: exact
            device_score(used_k)
            s = float(score_d[n])
            device_score(d["used"])
            return s
    else:
        score, cap = kc.oracle_score_cap(st, w_least=w_least, w_most=w_most,
                                         w_bal=w_bal, bias=bias)
        score_fn = None
        assert kc.same_bits(score, score_d.cpu())

    def outputs(dev):
        return [torch.zeros(K, dtype=torch.int32, device=dev),
                torch.zeros(K, dtype=torch.int32, device=dev),
                torch.zeros(1, dtype=torch.int32, device=dev),
                torch.zeros(1, dtype=torch.int32, device=dev),
                torch.full((1,), 7, dtype=torch.int32, device=dev)]

    def result(out, used, qa):
        m = int(out[2])
        return (out[0][:m].tolist(), out[1][:m].tolist(), m, int(out[3]),
                int(out[4]), used.cpu(), qa.cpu())

    want = None
    if not static:          # the static select is held to the caller's want
        out, used, qa = outputs("cpu"), st["used"].clone(), torch.ones(R)
        ref.rescore_select_commit(
            st["alloc"], used, st["extra"], st["ready"], st["taints"],
            st["planes"], st["req"], 0, zw, zw, w_least, w_most, w_bal,
            st["dim_w"], bias, score.clone(), cap, ntasks, qa, ql, out[0],
            out[1], out[2][0], out[3][0], out[4][0], fuse_min, score_fn)
        want = result(out, used, qa)

    out, qa = outputs(DEV), torch.ones(R, device=DEV)
    if static:
        hip.select_commit(score_d, cap_d, fixed["req"], ntasks, d["used"], qa,
                          ql.to(DEV), *out, fuse_min)
    else:
        hip.rescore_select(
            d["alloc"], d["used"], d["extra"], ready, fixed["taints"],
            d["pl"], fixed["req"], 0, zw.to(DEV), zw.to(DEV), w_least, w_most,
            w_bal, fixed["dim_w"], bias_d, score_d, cap_d, ntasks, qa,
            ql.to(DEV), *out, fuse_min)
    torch.cuda.synchronize()
    return want, result(out, d["used"].t(), qa)


def same(want, got):
    assert want[:5] == got[:5]
    assert kc.same_bits(want[5], got[5]) and kc.same_bits(want[6], got[6])


@pytest.mark.parametrize("weights", list(WEIGHTS))
@pytest.mark.parametrize("ntasks", [1, 37, 10 ** 6])
@pytest.mark.parametrize("R", [1, 4])
@pytest.mark.parametrize("N", [63, 65, 1025, 2049])
def test_kernel_equals_oracle(N, R, ntasks, weights):
    w_least, w_most, biased = WEIGHTS[weights]
    st = kc.dyadic_state(N, R, 1, seed=N + R)
    args = (st, ntasks, w_least, w_most)
    kw = dict(bias=st["bias"] if biased else None)
    want, got = run_both(*args, **kw)
    assert want[3] >= 1
    same(want, got)
    if weights == "most":
        same(want, run_both(*args, static=True, **kw)[1])


def flat(N, alive, bias=None):
    """One dim of 16 units, one requested; only ``alive`` can take work."""
    one = torch.ones(N, 1)
    ready = torch.zeros(N, dtype=torch.bool)
    ready[list(alive)] = True
    b = torch.zeros(N)
    for n, v in (bias or {}).items():
        b[n] = v
    return dict(alloc=16 * one, used=0 * one, extra=0 * one, ready=ready,
                taints=torch.zeros(N, dtype=torch.int64),
                planes=torch.zeros(N, 1, dtype=torch.int64),
                req=torch.ones(1), dim_w=torch.ones(1), bias=b)


BRANCHES = {
    # name: (state, ntasks, (w_least, w_most), keywords, (nodes, counts))
    "quota-ends-a-run": (flat(70, range(70)), 40, (0.0, 1.0),
                         dict(limit=6.0), ([0], [5])),
    "log-capped": (flat(70, range(5)), 9, (1.0, 0.0), dict(K=2),
                   ([0, 1], [1, 1])),
    "failed-gang": (flat(70, range(3)), 4, (1.0, 0.0), dict(fuse_min=10),
                    ([0, 1, 2], [0, 0, 0])),
    "twins-take-turns": (flat(70, range(5)), 12, (1.0, 0.0), {},
                         ([0, 1, 2, 3, 4], [3, 3, 2, 2, 2])),
    # after one instance node 5 ties node 2 exactly (0.9375): the run ends
    # and the second instance goes to node 2; a run that went on would log
    # ([5], [2]).  With the runner-up at the higher index the run goes on,
    # which no output tells from a fresh reduce: that case only has to agree.
    "tie-runner-lower": (flat(70, (2, 5), {5: 1 / 16}), 2, (1.0, 0.0), {},
                         ([5, 2], [1, 1])),
    "tie-runner-higher": (flat(70, (2, 5), {2: 1 / 16}), 3, (1.0, 0.0), {},
                          ([2, 5], [2, 1])),
    "runner-in-own-slice": (flat(1030, (3, 1027)), 7, (1.0, 0.0), {},
                            ([3, 1027], [4, 3])),
}


@pytest.mark.parametrize("name", list(BRANCHES))
def test_forced_branch(name):
    st, ntasks, (w_least, w_most), kw, log = BRANCHES[name]
    want, got = run_both(st, ntasks, w_least, w_most, bias=st["bias"], **kw)
    assert want[:2] == log
    same(want, got)
    if name == "failed-gang":
        assert got[3] == 0 and not got[5].any() and got[6].tolist() == [1.0]


@pytest.mark.parametrize("N", [65, 1025])
def test_inexact_inputs_follow_the_kernels_own_scores(N):
    st = kc.dyadic_state(N, 4, 1, seed=N, inexact=True)
    want, got = run_both(st, 40, 1.0, 0.0, w_bal=1.0, bias=st["bias"],
                         inexact=True)
    assert want[3] == 40 and len(want[0]) > 1
    same(want, got)


def rescore_plan(device):
    """The device-share plan with every class of two or more instances
    flagged: plain single-class gangs (one cannot fit), a discarded and a
    kept multi-class job, device requests, a hypernode class, an affinity
    class, and plain classes inside the chain-length runs."""
    plan, _ = dc.build_device_plan(device)
    for cp in plan.classes:
        cp.rescore = cp.ntasks >= 2
    aff = plan.classes[12]
    dom_of = (np.arange(plan.nt.n) % 7).astype(np.int32)
    aff.affinity = (plan.add_spread_group(dom_of, np.zeros(7, np.int32)),
                    ref.AFFINITY)
    aff.ntasks_override, aff.rescore = 5, True
    plan.finalize()
    return plan


@functools.lru_cache(maxsize=None)
def plan_oracle():
    """run_plan_torch on the flagged plan: computed once, never modified.
    Usage is integral, so the discarded gang's revert restores it exactly."""
    plan = rescore_plan("cpu")
    res = planmod.run_plan_torch(plan)
    snap = kc.snapshot(plan, res)
    flagged = set(np.flatnonzero(plan.class_rescore).tolist())
    assert {0, 1, 3, 8, 12} <= flagged and len(flagged) > 20
    assert plan.classes[7].spread is not None and 7 not in flagged
    # the discarded multi-class job had placed over several nodes
    assert snap["job_flag"][3] == 0 and snap["log_len"][3] > 1
    assert snap["class_placed"][2] == 0 and snap["class_placed"][12] > 0
    return snap, res.dev_assign


@pytest.mark.parametrize("mode", ["default", "megacycle", "chain"])
def test_plan_with_flagged_classes(monkeypatch, mode):
    for var in MODE_VARS:
        monkeypatch.delenv(var, raising=False)
    if mode == "megacycle":
        monkeypatch.setenv("VAMD_MEGACYCLE", "1")
    elif mode == "chain":
        monkeypatch.setenv("VAMD_CHAIN_CHUNK", "16")
    want, want_rows = plan_oracle()
    plan = rescore_plan(DEV)
    res = planmod.run_plan_hip(plan)
    kc.compare_results(want, kc.snapshot(plan, res))
    assert np.array_equal(want_rows, res.dev_assign)
