"""``spread_soft_select`` and its routing in ``vamd_run_cycle`` against the
oracle (``reference.spread_soft_select_commit``), bit for bit: log, counters,
every rule's counts, ``used`` and ``queue_alloc``."""

import functools

import numpy as np
import pytest
import torch

import _domain_score_cases as dsc
import _kernel_cases as kc
import _spread_cases as sc
import test_spread_gpu as sg
import test_spread_multi_gpu as smg
import test_spread_soft as cpu
from test_rescore_gpu import flat
from volcano_amd.ops import reference as ref
from volcano_amd.scheduler import plan as planmod

pytestmark = pytest.mark.gpu

DEV = sg.DEV
TW, SKEW = cpu.TW, ref.SPREAD_SOFT_SKEW


def run_both(st, rules, ntasks, rescore, *, w_bal=0.0, K=None, limit=1.0e9,
             fuse_min=-1, inexact=False, score_cap=None):
    """Oracle and device -> (want, got), tuples of ``test_spread_soft.run``.
    ``inexact`` feeds the oracle the kernel's own score bits."""
    from volcano_amd.ops import hip
    N, R = st["alloc"].shape
    K = max(1, min(ntasks, N)) if K is None else K
    zw = torch.zeros(st["planes"].shape[1], dtype=torch.int64, device=DEV)
    d = {k: st[k].t().contiguous().to(DEV)
         for k in ("alloc", "used", "extra", "planes")}
    fixed = {k: st[k].to(DEV) for k in ("taints", "req", "dim_w", "bias")}
    ready = st["ready"].to(torch.uint8).to(DEV)
    score_d = torch.empty(N, device=DEV)
    cap_d = torch.empty(N, dtype=torch.int32, device=DEV)

    def device_score(used_t):
        hip.score_cap(d["alloc"], used_t, d["extra"], ready, fixed["taints"],
                      d["planes"], fixed["req"], 0, zw, zw, 1.0, 0.0, w_bal,
                      fixed["dim_w"], fixed["bias"], score_d, cap_d)

    def score_fn(n, k):         # the kernel's own score bits for the oracle
        used_k = d["used"].clone()
        used_k[:, n] += float(k) * fixed["req"]         # integers: exact
        device_score(used_k)
        s = float(score_d[n])
        device_score(d["used"])
        return s

    device_score(d["used"])
    if score_cap is not None:
        score_d.copy_(score_cap[0])
        cap_d.copy_(score_cap[1])
    elif inexact:
        score_cap = (score_d.cpu(), cap_d.cpu())
    want = cpu.run(st, rules, ntasks, rescore, w_bal=w_bal, K=K, limit=limit,
                   fuse_min=fuse_min, score_cap=score_cap,
                   score_fn=score_fn if inexact else None)
    ln, lc = (torch.zeros(K, dtype=torch.int32, device=DEV) for _ in range(2))
    ll, pl = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2))
    jp = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    rs = [(torch.from_numpy(dom).to(DEV), torch.from_numpy(c.copy()).to(DEV),
           k, tw) for dom, c, k, tw in rules]
    qa, ql = torch.ones(R, device=DEV), torch.full((R,), limit, device=DEV)
    hip.spread_soft_select(
        d["alloc"], d["used"], d["extra"], fixed["req"], 1.0, 0.0, w_bal,
        fixed["dim_w"], fixed["bias"], score_d, cap_d, ntasks, qa, ql, ln, lc,
        ll, pl, jp, rs, rescore, fuse_min)
    torch.cuda.synchronize()
    m = int(ll)
    return want, (ln[:m].tolist(), lc[:m].tolist(), int(pl), int(jp),
                  [r[1].tolist() for r in rs], d["used"].t().cpu(), qa.cpu())


RULESETS = ["S3", "SN", "H3-SN", "S65-HN", "H31-S32-S65-SN"]


@pytest.mark.parametrize("rescore", [False, True])
@pytest.mark.parametrize("family", list(dsc.FAMILIES))
@pytest.mark.parametrize("ruleset", RULESETS)
@pytest.mark.parametrize("N", [65, 1025, 2049])
def test_kernel_equals_oracle(N, ruleset, family, rescore):
    st, rules, sc = cpu.family_case(family, N, N + len(ruleset), ruleset)
    want, got = run_both(st, rules, 120, rescore, score_cap=sc)
    assert want[2] > 1
    cpu.same(want, got)


@pytest.mark.parametrize("rescore", [False, True])
@pytest.mark.parametrize("N", [65, 1025])
def test_inexact_inputs_follow_the_kernels_own_scores(N, rescore):
    st = kc.dyadic_state(N, 4, 1, seed=N, inexact=True)
    rules = cpu.family_case("grid", N, N, "H3-SN")[1]
    want, got = run_both(st, rules, 40, rescore, w_bal=1.0, inexact=True)
    assert want[2] > 1
    cpu.same(want, got)


def zones(N, D, tw, skew=1, count=None, without=()):
    dom = (np.arange(N) % D).astype(np.int32)
    dom[list(without)] = -1
    return (dom, np.array(count or [0] * D, dtype=np.int32),
            SKEW if tw else skew, tw)


all70 = functools.partial(flat, 70, range(70))
TIE = cpu.rounding_tie(70)
LIMIT = ref.SPREAD_SOFT_LDS_DOMAINS
# ``flat`` scores 0.9375 + bias, less 1/16 per staged instance (re-score).
# name: (state, rules, ntasks, rescore, keywords, (nodes, counts))
BRANCHES = {
    # both rules split even / odd.  The soft one keeps the even nodes 0.18
    # cheaper, but n0 shuts the hard even zone: n1, then n0 again
    "hard-zone-shut": (all70(), [zones(70, 2, 0.0),
                                 zones(70, 2, TW, count=[0, 9])], 3, False,
                       {}, ([0, 1], [2, 1])),
    # n1 lifts the hard minimum: zone 0 reopens for n2
    "minimum-rises": (all70(), [zones(70, 2, 0.0), zones(70, 70, TW)], 4,
                      True, {}, ([0, 1, 2, 3], [1] * 4)),
    # n0 stays ahead by its bias through three members of its zone
    "wins-again": (all70({0: 0.5}), [zones(70, 2, TW)], 3, False, {},
                   ([0], [3])),
    # the best node has a hard zone and no soft hostname
    "unlabelled-under-soft": (all70({4: 1.0}),
                              [zones(70, 2, 0.0, skew=5),
                               zones(70, 70, TW, without=[4])], 2, False, {},
                              ([0, 1], [1, 1])),
    "rounding-tie": (all70(), TIE[0], 2, False, dict(score_cap=TIE[1]),
                     ([0, 1], [1, 1])),
    "queue-budget": (all70(), [zones(70, 3, TW)], 10, False, dict(limit=4.0),
                     ([0, 1, 2], [1] * 3)),
    # n0 resumes its entry; a third node would need a third one
    "log-capped": (all70({0: 0.5}), [zones(70, 2, TW)], 40, True, dict(K=2),
                   None),
    "failed-gang": (all70(), [zones(70, 2, 0.0, count=[3, 2]),
                              zones(70, 70, TW)], 4, False,
                    dict(fuse_min=10), ([1, 0, 3, 2], [0] * 4)),
    "table-at-the-limit": (flat(LIMIT, range(LIMIT)), [zones(LIMIT, LIMIT, TW)],
                           5, False, {}, (list(range(5)), [1] * 5)),
}


@pytest.mark.parametrize("name", list(BRANCHES))
def test_forced_branch(name):
    st, rules, ntasks, rescore, kw, log = BRANCHES[name]
    want, got = run_both(st, rules, ntasks, rescore, **kw)
    assert log is None or want[:2] == log
    cpu.same(want, got)
    if name == "log-capped":
        assert len(want[0]) == 2 and 2 < want[2] < ntasks
    if name == "failed-gang":
        assert got[2] == 0 and got[6].tolist() == [1.0]
        assert kc.same_bits(got[5], st["used"])
        assert got[4] == [r[1].tolist() for r in rules]


def soft_plan(device):
    """The plan of test_spread_multi_gpu: the reverting gang role hard zone +
    soft hostname, the kept two-rule class all soft and re-scoring."""
    case = sc.spread_plan_case(bulk=False)
    plan = smg.build(case, device)
    r = case.roles
    gang, kept = plan.classes[r["gang_spread"]], plan.classes[r["spread"]]
    gang.spread_rules, gang.spread_soft = [(0, 1), (1, SKEW)], [0.0, TW]
    kept.spread_rules, kept.spread_soft = [(0, SKEW), (1, SKEW)], [TW, TW]
    kept.spread, kept.rescore = kept.spread_rules[0], True
    plan.finalize()
    return plan, r


@functools.lru_cache(maxsize=None)
def plan_oracle():
    plan, r = soft_plan("cpu")
    snap = sc.spread_snapshot(plan, planmod.run_plan_torch(plan))
    assert plan.class_spread_soft.any(axis=1).sum() == 2
    assert snap["log_len"][r["gang_spread"]] > 0
    assert snap["class_placed"][r["gang_spread"]] == 0
    assert min(snap["class_placed"][r[k]] for k in ("spread", "host")) > 1
    return snap


@pytest.mark.parametrize("mode", [{}, {"VAMD_MEGACYCLE": 1},
                                  {"VAMD_CHAIN_CHUNK": 4}],
                         ids=["default", "megacycle", "chain4"])
def test_plan_with_soft_spread_classes(monkeypatch, mode):
    want = plan_oracle()
    sg.set_mode(monkeypatch, **mode)
    plan, _ = soft_plan(DEV)
    res = planmod.run_plan_hip(plan)
    torch.cuda.synchronize()
    sc.compare_spread(want, sc.spread_snapshot(plan, res))
