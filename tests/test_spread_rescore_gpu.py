"""``spread_rescore_select`` and its routing in ``vamd_run_cycle`` against the
oracle (``reference.spread_rescore_select_commit``), bit for bit: log,
counters, every rule's counts, ``used`` and ``queue_alloc``."""

import functools

import numpy as np
import pytest
import torch

import _kernel_cases as kc
import _spread_cases as sc
import test_spread_gpu as sg
import test_spread_multi_gpu as smg
import test_spread_rescore as cpu
from test_rescore_gpu import flat
from volcano_amd.scheduler import plan as planmod

pytestmark = pytest.mark.gpu

DEV = sg.DEV


def run_both(st, rules, ntasks, w_least, w_most, *, w_bal=0.0, K=None,
             limit=1.0e9, fuse_min=-1, inexact=False, cap_of=None,
             static=False):
    """One select in the oracle and on the device -> (want, got), each the
    tuple of ``test_spread_rescore.run``.  ``static`` runs
    ``spread_multi_select`` on the device and no oracle."""
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
                      d["planes"], fixed["req"], 0, zw, zw, w_least, w_most,
                      w_bal, fixed["dim_w"], fixed["bias"], score_d, cap_d)

    def score_fn(n, k):         # the kernel's own score bits for the oracle
        used_k = d["used"].clone()
        used_k[:, n] += float(k) * fixed["req"]         # integers: exact
        device_score(used_k)
        s = float(score_d[n])
        device_score(d["used"])
        return s

    device_score(d["used"])
    want = None
    if not static:
        want = cpu.run(
            st, rules, ntasks, w_least, w_most, w_bal=w_bal, K=K, limit=limit,
            fuse_min=fuse_min, cap_of=cap_of,
            **(dict(score_cap=(score_d.cpu(), cap_d.cpu()),
                    score_fn=score_fn) if inexact else {}))
    for n, c in (cap_of or {}).items():
        cap_d[n] = c
    ln, lc = (torch.zeros(K, dtype=torch.int32, device=DEV) for _ in range(2))
    ll, pl = (torch.zeros(1, dtype=torch.int32, device=DEV) for _ in range(2))
    jp = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    rs = [(torch.from_numpy(dom).to(DEV), torch.from_numpy(c.copy()).to(DEV),
           k) for dom, c, k in rules]
    qa, ql = torch.ones(R, device=DEV), torch.full((R,), limit, device=DEV)
    tail = (ntasks, qa, ql, ln, lc, ll, pl, jp, rs, fuse_min)
    if static:
        hip.spread_multi_select(score_d, cap_d, fixed["req"], ntasks,
                                d["used"], *tail[1:])
    else:
        hip.spread_rescore_select(
            d["alloc"], d["used"], d["extra"], fixed["req"], w_least, w_most,
            w_bal, fixed["dim_w"], fixed["bias"], score_d, cap_d, *tail)
    torch.cuda.synchronize()
    m = int(ll)
    return want, (ln[:m].tolist(), lc[:m].tolist(), int(pl), int(jp),
                  [c.tolist() for _, c, _ in rs], d["used"].t().cpu(),
                  qa.cpu())


# D per rule: a zone rule, hostname, both, and both sides of the 32- / 64-bit
# bitmap words
RULESETS = {"3": (3,), "N": ("N",), "3-N": (3, "N"), "65-N": (65, "N"),
            "31-32-65-N": (31, 32, 65, "N")}


def draw_rules(N, ds, seed):
    """Every domain owns a node, 5% of the nodes carry no label, counts 0/1,
    skews 1 and 2 in turn."""
    rng = np.random.RandomState(seed)
    rules = []
    for k, D in enumerate(N if d == "N" else d for d in ds):
        dom = np.concatenate([np.arange(D), rng.randint(0, D, size=N - D)])
        dom = dom[rng.permutation(N)].astype(np.int32)
        dom[rng.rand(N) < 0.05] = -1
        rules.append((dom, rng.randint(0, 2, size=D).astype(np.int32),
                      1 + (seed + k) % 2))
    return rules


@pytest.mark.parametrize("ruleset", list(RULESETS))
@pytest.mark.parametrize("N", [65, 1025, 2049])
def test_kernel_equals_oracle(N, ruleset):
    st = kc.dyadic_state(N, 4, 1, seed=N)
    rules = draw_rules(N, RULESETS[ruleset], N + len(ruleset))
    want, got = run_both(st, rules, 120, 1.0, 0.0)
    assert want[2] > 1
    cpu.same(want, got)


@pytest.mark.parametrize("N", [65, 1025])
def test_inexact_inputs_follow_the_kernels_own_scores(N):
    st = kc.dyadic_state(N, 4, 1, seed=N, inexact=True)
    want, got = run_both(st, draw_rules(N, (3, "N"), N), 40, 1.0, 0.0,
                         w_bal=1.0, inexact=True)
    assert want[2] > 1
    cpu.same(want, got)


def zones(N, D, skew=1, count=None, without=()):
    dom = (np.arange(N) % D).astype(np.int32)
    dom[list(without)] = -1
    return (dom, np.array(count or [0] * D, dtype=np.int32), skew)


def all70(bias=None, full=None):
    st = flat(70, range(70), bias)
    if full is not None:
        st["used"][full] = 15.0         # of 16: room for one
    return st


# Scores on ``flat``: 0.9375 + bias, less 1/16 per staged instance.
# name: (state, rules, ntasks, keywords, (nodes, counts))
BRANCHES = {
    # n0 shuts zone 0, n1 zone 1; a stale best would offer n3 before n2
    "zone-shut": (all70(), [zones(70, 3)], 7, {}, (list(range(7)), [1] * 7)),
    # n1 lifts the minimum: zone 0 reopens and n2 beats the re-scored n0
    "minimum-rises": (all70(), [zones(70, 2)], 4, {}, ([0, 1, 2, 3], [1] * 4)),
    # only n0 sits at both minima; placing it lifts both at once
    "two-minima-rise": (all70(), [zones(70, 2, count=[0, 1]),
                                  zones(70, 3, count=[0, 1, 1])], 4, {},
                        ([0, 1, 2, 3], [1] * 4)),
    # n0 stays ahead by its bias and wins whenever zone 0 is open
    "slot-resume": (all70({0: 0.5}), [zones(70, 2)], 5, {},
                    ([0, 1, 3], [3, 1, 1])),
    # n0 would win again at 2.0: out on capacity, or on the fit test when
    # the capacity it was handed is too large
    "full-on-capacity": (all70({0: 2.0}, full=0), [zones(70, 2, skew=2)], 3,
                         {}, ([0, 1, 2], [1] * 3)),
    "full-on-fit-test": (all70({0: 2.0}, full=0), [zones(70, 2, skew=2)], 3,
                         dict(cap_of={0: 5}), ([0, 1, 2], [1] * 3)),
    # the best node has a zone and no hostname
    "unlabelled-under-second": (all70({4: 1.0}),
                                [zones(70, 2, skew=5),
                                 zones(70, 70, without=[4])], 2, {},
                                ([0, 1], [1, 1])),
    "queue-budget": (all70(), [zones(70, 3)], 10, dict(limit=4.0),
                     ([0, 1, 2], [1] * 3)),
    # n0 resumes its entry; n3 would need a third one
    "log-capped": (all70({0: 0.5}), [zones(70, 2)], 6, dict(K=2),
                   ([0, 1], [2, 1])),
    "failed-gang": (all70(), [zones(70, 2, count=[3, 2]), zones(70, 70)], 4,
                    dict(fuse_min=10), ([1, 0, 3, 2], [0] * 4)),
}


@pytest.mark.parametrize("name", list(BRANCHES))
def test_forced_branch(name):
    st, rules, ntasks, kw, log = BRANCHES[name]
    want, got = run_both(st, rules, ntasks, 1.0, 0.0, **kw)
    assert want[:2] == log
    cpu.same(want, got)
    if name == "failed-gang":
        assert got[2] == 0 and got[6].tolist() == [1.0]
        assert kc.same_bits(got[5], st["used"])
        assert got[4] == [c.tolist() for _, c, _ in rules]


@pytest.mark.parametrize("weights", list(cpu.STATIC))
def test_static_scores_equal_the_multi_rule_select(weights):
    w_most, cap_one = cpu.STATIC[weights]
    st = kc.dyadic_state(1025, 4, 1, seed=5, cap_one=cap_one)
    args = (st, draw_rules(1025, (3, "N"), 5), 120, 0.0, w_most)
    static = run_both(*args, static=True)[1]
    assert static[2] > 1
    cpu.same(static, run_both(*args)[1])


def flagged_plan(device):
    """The plan of test_spread_multi_gpu with every spread class flagged: a
    two-rule role in a gang that reverts, a kept two-rule class, and the
    one-rule classes of the hostname group, one of them a failed gang."""
    case = sc.spread_plan_case(bulk=False)
    plan = smg.build(case, device)
    for cp in plan.classes:
        cp.rescore = cp.spread is not None
    plan.finalize()
    return plan, case.roles


@functools.lru_cache(maxsize=None)
def plan_oracle():
    """run_plan_torch on the flagged plan: computed once, never modified."""
    plan, r = flagged_plan("cpu")
    snap = sc.spread_snapshot(plan, planmod.run_plan_torch(plan))
    flagged = np.flatnonzero(plan.class_spread_rescore).tolist()
    rules = {len(plan.classes[c].spread_rules or [0]) for c in flagged}
    assert rules == {1, 2} and not plan.class_rescore.any()
    assert snap["log_len"][r["gang_spread"]] > 0
    assert snap["class_placed"][r["gang_spread"]] == 0
    assert min(snap["class_placed"][r[k]] for k in ("spread", "host")) > 1
    return snap


@pytest.mark.parametrize("mode", [{}, {"VAMD_MEGACYCLE": 1},
                                  {"VAMD_CHAIN_CHUNK": 4}],
                         ids=["default", "megacycle", "chain4"])
def test_plan_with_flagged_spread_classes(monkeypatch, mode):
    want = plan_oracle()
    sg.set_mode(monkeypatch, **mode)
    plan, _ = flagged_plan(DEV)
    res = planmod.run_plan_hip(plan)
    torch.cuda.synchronize()
    sc.compare_spread(want, sc.spread_snapshot(plan, res))
