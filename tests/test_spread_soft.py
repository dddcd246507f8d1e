"""``whenUnsatisfiable: ScheduleAnyway`` topology spread on the CPU:
``reference.spread_soft_select_commit`` by hand, against the oracles it must
collapse into, and through the scheduler."""

import numpy as np
import pytest
import torch

import _domain_score_cases as dsc
import _kernel_cases as kc
import test_spread_e2e as e2e
from test_rescore import twins
from test_spread_rescore import same
from volcano_amd.ops import reference as ref
from volcano_amd.utils import synth

TW = 0.02                   # soft.weight 2.0 on the 0-1 score scale
TINY = 2.0 ** -60           # a penalty below half an ulp of every |score| >= 1e-3


def run(st, rules, ntasks, rescore, oracle="soft", *, w_least=1.0, w_most=0.0,
        w_bal=0.0, K=None, limit=1.0e9, fuse_min=-1, score_cap=None,
        score_fn=None):
    """One select of ``oracle`` on a state dict and ``(dom_of, count, skew,
    tw)`` numpy rules -> (nodes, counts, placed, job_placed, [count per rule],
    used, queue_alloc).  ``score_cap`` replaces the oracle's score and cap."""
    N, R = st["alloc"].shape
    zw = torch.zeros(st["planes"].shape[1], dtype=torch.int64)
    score, cap = score_cap or kc.oracle_score_cap(
        st, w_least=w_least, w_most=w_most, w_bal=w_bal, bias=st.get("bias"))
    score, cap = score.clone(), cap.clone()
    K = max(1, min(ntasks, N)) if K is None else K
    ln, lc = (torch.zeros(K, dtype=torch.int32) for _ in range(2))
    ll, pl = (torch.zeros((), dtype=torch.int32) for _ in range(2))
    jp = torch.full((), 7, dtype=torch.int32)
    used, qa, ql = st["used"].clone(), torch.ones(R), torch.full((R,), limit)
    rs = [(torch.from_numpy(d), torch.from_numpy(c.copy()), k, tw)
          for d, c, k, tw in rules]
    hard = [r[:3] for r in rs]
    inputs = (st["alloc"], used, st["extra"], st["ready"], st["taints"],
              st["planes"], st["req"], 0, zw, zw, w_least, w_most, w_bal,
              st["dim_w"], st.get("bias"), score, cap, ntasks, qa, ql)
    out = (ln, lc, ll, pl, jp)
    static = (score, cap, st["req"], ntasks, used, qa, ql, *out)
    if oracle == "soft":
        ref.spread_soft_select_commit(*inputs, *out, rs, rescore, fuse_min,
                                      score_fn)
    elif oracle == "hard" and rescore:
        ref.spread_rescore_select_commit(*inputs, *out, hard)
    elif oracle == "hard":
        ref.spread_multi_select_commit(*static, hard)
    elif rescore:
        ref.rescore_select_commit(*inputs, *out)
    else:
        ref.select_commit(*static)
    m = int(ll)
    return (ln[:m].tolist(), lc[:m].tolist(), int(pl), int(jp),
            [r[1].tolist() for r in rs], used, qa)


def family_case(family, N, seed, spec, tw=TW, labelled=False):
    """A dyadic state, the rules of ``spec`` — hard ``H<D>`` (skews 1 and 2 in
    turn) and soft ``S<D>`` of weight ``tw``, counts 0/1, every domain owning
    a node, 5% of the nodes without a label — and a score vector of
    ``family`` with a tenth of the nodes infeasible."""
    rng = np.random.RandomState(seed)
    rules = []
    for k, word in enumerate(spec.split("-")):
        D = N if word[1:] == "N" else int(word[1:])
        dom = np.concatenate([np.arange(D), rng.randint(0, D, size=N - D)])
        dom = dom[rng.permutation(N)].astype(np.int32)
        if not labelled:
            dom[rng.rand(N) < 0.05] = -1
        soft = word[0] == "S"
        rules.append((dom, rng.randint(0, 2, size=D).astype(np.int32),
                      ref.SPREAD_SOFT_SKEW if soft else 1 + (seed + k) % 2,
                      tw if soft else 0.0))
    score = np.array(dsc.FAMILIES[family](N, rng), dtype=np.float32)
    if labelled:
        # no weight is lost against a zero or a denormal: those scores leave
        score[np.abs(score) < 1e-3] = 1.0
    score[rng.rand(N) < 0.1] = -np.inf
    cap = torch.from_numpy(rng.randint(0, 4, size=N).astype(np.int32))
    return (kc.dyadic_state(N, 4, 1, seed=seed), rules,
            (torch.from_numpy(score), cap))


@pytest.mark.parametrize("rescore", [True, False])
@pytest.mark.parametrize("family", list(dsc.FAMILIES))
def test_zero_weights_equal_the_hard_oracles(family, rescore):
    st, rules, sc = family_case(family, 300, 11, "H3-HN")
    got = run(st, rules, 40, rescore, score_cap=sc)
    assert got[2] > 1
    same(got, run(st, rules, 40, rescore, "hard", score_cap=sc))


@pytest.mark.parametrize("rescore", [True, False])
@pytest.mark.parametrize("family", list(dsc.FAMILIES))
def test_lost_weights_equal_the_plain_selects(family, rescore):
    """Soft rules only, every node labelled, 40 instances of weight 2^-60:
    ``score - pen == score`` for every score of 1e-3 and more."""
    st, rules, sc = family_case(family, 300, 12, "S3-SN", TINY, labelled=True)
    got = run(st, rules, 40, rescore, score_cap=sc)
    assert got[2] == 40 and len(got[0]) > 1
    same(got, run(st, rules, 40, rescore, "plain", score_cap=sc), upto=4)


def test_twin_nodes_in_two_zones():
    """Static scores, one soft zone rule: n0, then zone 1 is cheaper: n2;
    both zones cost the same again and the tie goes back to n0, then n2."""
    zone = np.array([0, 0, 1, 1], dtype=np.int32)
    rule = [(zone, np.zeros(2, np.int32), ref.SPREAD_SOFT_SKEW, TW)]
    for ntasks, per_node in ((2, [1, 0, 1, 0]), (4, [2, 0, 2, 0])):
        got = run(twins(4), rule, ntasks, False, w_least=0.0, w_most=1.0)
        assert got[5][:, 0].tolist() == [float(k) for k in per_node]
        assert got[0] == [0, 2] and got[4] == [[ntasks // 2] * 2]


def rounding_tie(N=4):
    """n0 scores one ulp BELOW n1 in the same zone; two members at 0.5 cost
    1.0 and both totals round to -2.0: the tie goes to n0, which no head
    keyed on the raw score would offer.  Zone 1 is far behind."""
    score = torch.full((N,), -9.0)
    score[0], score[1] = -1.0 - 2.0 ** -23, -1.0
    zone = (np.arange(N) >= 2).astype(np.int32)
    rule = [(zone, np.array([2, 0], np.int32), ref.SPREAD_SOFT_SKEW, 0.5)]
    return rule, (score, torch.ones(N, dtype=torch.int32))


def test_penalty_rounds_two_scores_onto_one_total():
    rule, sc = rounding_tie()
    got = run(twins(4), rule, 2, False, score_cap=sc)
    assert got[:2] == ([0, 1], [1, 1]) and got[4] == [[4, 0]]


def soft_job(store, name, replicas, when):
    store.create("PodGroup", synth.make_podgroup(name, min_member=1))
    for i in range(replicas):
        p = synth.make_pod(f"{name}-w-{i}", name, cpu_milli=500, mem=e2e.GI,
                           role="w")
        p.affinity = {"topologySpread": {
            "group": "web", "topologyKey": "zone", "maxSkew": 1,
            **({"whenUnsatisfiable": when} if when else {})}}
        store.create("Pod", p)


@pytest.mark.parametrize("when, placed", [("ScheduleAnyway", 4),
                                          ("DoNotSchedule", 2), (None, 2)])
def test_four_replicas_one_slot_in_the_second_zone(when, placed):
    """Zone a holds one member from an earlier cycle and has room; zone b has
    one free slot.  Hard: b, a, then a is shut and b is full.  Soft: all
    four land."""
    store, binder, sched = e2e.mk(exact=True)
    e2e.inventory(store, {"a0": ("a", 8000), "b0": ("b", 600)})
    soft_job(store, "first", 1, when)
    sched.run_once()
    assert list(binder.binds.values()) == ["a0"]
    soft_job(store, "web", 4, when)
    sched.run_once()
    nodes = sorted(binder.binds.values())
    assert len(nodes) == 1 + placed
    assert when == "ScheduleAnyway" or nodes.count("b0") == 1
