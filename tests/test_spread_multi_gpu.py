"""``vamd_spread_multi_select`` and its routing in ``vamd_run_cycle`` against
``reference.spread_multi_select_commit``: log, counters, usage, queue
allocation and every rule's counts, bit for bit."""

import functools

import numpy as np
import pytest
import torch

import _domain_score_cases as dsc
import _spread_cases as sc
import test_spread_gpu as sg
from test_spread_multi import run_multi
from volcano_amd.ops import reference as ref

pytestmark = pytest.mark.gpu

# D per rule: both sides of the 32- / 64-bit bitmap words and the wave step
RULESETS = {"3-N": (3, "N"), "65-N": (65, "N"), "33-64": (33, 64),
            "31-32-65-N": (31, 32, 65, "N"), "N": ("N",)}


def make(N, ds, fam, seed, **kw):
    """-> (case, rules); rules 1.. draw a map, counts 0/1, a skew in {1, 2}."""
    ds = [N if d == "N" else d for d in ds]
    case = sc.random_case(f"m{seed}", N, ds[0], 1 + seed % 2,
                          (1, 5, 64)[seed % 3], seed,
                          scores=dsc.FAMILIES[fam], **kw)
    rng = np.random.RandomState(seed + 1)
    rules = [(case.dom_of, case.dom_count, case.max_skew)]
    for k, D in enumerate(ds[1:]):
        dom = np.concatenate([np.arange(D), rng.randint(0, D, size=N - D)])
        dom = dom[rng.permutation(N)].astype(np.int32)
        dom[rng.rand(N) < 0.05] = -1
        rules.append((dom, rng.randint(0, 2, size=D).astype(np.int32),
                      1 + (seed + k) % 2))
    return case, rules


def both_minima_rise():
    """D = (33, 64), N = 65: only node 5 has both its domains at the minimum
    0; placing it lifts both minima at once and reopens everything."""
    case, _ = make(65, (33, 64), "grid", 3, unlabeled=0.0, infeasible=0.0,
                   ntasks=40)
    idx = np.arange(65, dtype=np.int32)
    c1, c2 = np.ones(33, dtype=np.int32), np.ones(64, dtype=np.int32)
    c1[5] = c2[5] = 0
    case.cap[5] = 1
    return case, [(idx % 33, c1, 1), (idx % 64, c2, 1)]


def unlabeled_under_second():       # the best node: the first label only
    case, rules = make(1025, (3, "N"), "dense", 4, unlabeled=0.0)
    top = int(np.argmax(np.where(case.cap > 0, case.score, -np.inf)))
    rules[1][0][top] = -1
    return case, rules


P = functools.partial
# name -> (inputs, what the oracle's run of them must show: the branch is
# really taken); c = case, r = rules, w = the oracle's result
FEATURES = {
    "both-minima-rise": (both_minima_rise, lambda c, r, w:
                         w["log_nodes"][0] == 5 and w["before"] > 3),
    "unlabeled-under-second": (unlabeled_under_second, lambda c, r, w:
                               (r[0][0] >= 0).all() and (r[1][0] < 0).any()),
    # zone 2 has no feasible node: its count holds the minimum down
    "dead-domain": (P(make, 1025, (3, "N"), "grid", 5, dead_domain=True,
                      ntasks=200), lambda c, r, w:
                    w["before"] < c.ntasks and w["counts"][0][2] == r[0][1][2]
                    == w["counts"][0].min()),
    "minimum-rises": (P(make, 2049, (3, "N"), "special", 6, ntasks=200,
                        unlabeled=0.0), lambda c, r, w:
                      w["counts"][0].min() - r[0][1].min() >= 3),
    "log-capped": (P(make, 65, (3, "N"), "ladder", 7, ntasks=200),
                   lambda c, r, w: c.K < c.ntasks),
    "quota": (P(make, 1025, (65, "N"), "dense", 8, quota=11, ntasks=50),
              lambda c, r, w: w["before"] == sc.quota_of(c) < c.ntasks),
    "gang-revert": (P(make, 1025, (31, 32, 65, "N"), "grid", 9, ntasks=60,
                      fuse_min=2000), lambda c, r, w:
                    w["placed"] == 0 and not w["log_counts"].any() and all(
                        a.tolist() == x[1].tolist()
                        for a, x in zip(w["counts"], r))),
}
SHAPES = {f"{fam}-N{N}-D{tag}": functools.partial(make, N, ds, fam,
                                                  100 * f + 10 * i + j)
          for f, fam in enumerate(dsc.FAMILIES)
          for i, N in enumerate((65, 1025, 2049))
          for j, (tag, ds) in enumerate(RULESETS.items())}
ALL = {**SHAPES, **{k: v[0] for k, v in FEATURES.items()}}


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Case, rules and the oracle result: computed once, never modified."""
    case, rules = ALL[name]()
    want = run_multi(case, rules)
    want["before"] = want["placed"]
    if 0 <= want["placed"] < case.fuse_min:       # the fused gang revert
        t = torch.from_numpy
        placed = torch.tensor(want["placed"])
        jp = torch.tensor(want["job_placed"])
        ref.spread_multi_revert(
            torch.zeros((), dtype=torch.uint8), t(want["log_nodes"]),
            t(want["log_counts"]), torch.tensor(want["log_len"]), t(case.req),
            t(want["used"]), t(want["queue_alloc"]), placed, jp, want["rules"])
        want.update(placed=int(placed), job_placed=int(jp))
    return case, rules, want


def run_hip(case, rules, single=False):
    from volcano_amd.ops import hip
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(sg.DEV)
    used_t, qa = d(case.used.T.copy()), d(case.queue_alloc.copy())
    ln, lc = (torch.zeros(case.K, dtype=torch.int32, device=sg.DEV)
              for _ in range(2))
    ll, placed = (torch.zeros(1, dtype=torch.int32, device=sg.DEV)
                  for _ in range(2))
    jp = torch.full((1,), 7, dtype=torch.int32, device=sg.DEV)
    rs = [(d(dom), d(cnt.copy()), k) for dom, cnt, k in rules]
    head = (d(case.score.copy()), d(case.cap.copy()), d(case.req),
            case.ntasks, used_t, qa, d(case.queue_limit), ln, lc, ll, placed,
            jp)
    if single:
        hip.spread_select(*head, *rs[0], case.fuse_min)
    else:
        hip.spread_multi_select(*head, rs, case.fuse_min)
    torch.cuda.synchronize()
    return dict(log_nodes=ln.cpu().numpy(), log_counts=lc.cpu().numpy(),
                log_len=int(ll), placed=int(placed), job_placed=int(jp),
                used=used_t.t().cpu().numpy(), queue_alloc=qa.cpu().numpy(),
                counts=[c.cpu().numpy() for _, c, _ in rs])


def compare(want, got):
    n = want["log_len"]
    for key in ("log_len", "placed", "job_placed"):
        assert got[key] == want[key], key
    for key in ("log_nodes", "log_counts"):
        assert got[key][:n].tolist() == want[key][:n].tolist(), key
    for r, (a, b) in enumerate(zip(want["counts"], got["counts"])):
        assert b.tolist() == a.tolist(), f"counts of rule {r}"
    assert sg.same_bits(got["used"], want["used"]), "used differs"
    assert sg.same_bits(got["queue_alloc"], want["queue_alloc"])


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name):
    case, rules, want = oracle(name)
    got = run_hip(case, rules)
    compare(want, got)
    if len(rules) == 1:            # (N,) alone: the existing kernel agrees
        compare(got, run_hip(case, rules, single=True))


@pytest.mark.parametrize("name", list(FEATURES))
def test_features(name):
    case, rules, want = oracle(name)
    assert want["before"] > 0 and FEATURES[name][1](case, rules, want)
    compare(want, run_hip(case, rules))


def build(case, device):
    """A two-rule role in a gang that reverts, then a kept two-rule class of
    the same groups, then the plan's one-rule classes of the host group."""
    plan = sc.build_spread_plan(case, device)
    r = case.roles
    plan.classes[r["gang_spread"]].spread_rules = [(0, 1), (1, 1)]
    plan.classes[r["spread"]].spread_rules = [(0, 2), (1, 1)]
    for c, cp in enumerate(plan.classes):     # the plan is finalized already
        plan.check_spread_rules(c, cp)
    return plan


@functools.lru_cache(maxsize=None)
def plan_oracle():
    from volcano_amd.scheduler.plan import run_plan_torch
    case = sc.spread_plan_case(bulk=False)
    plan = build(case, "cpu")
    snap = sc.spread_snapshot(plan, run_plan_torch(plan))
    r = case.roles
    assert snap["log_len"][r["gang_spread"]] > 0
    assert snap["class_placed"][r["gang_spread"]] == 0
    assert min(snap["class_placed"][r[k]] for k in ("spread", "host")) > 0
    return case, snap


@pytest.mark.parametrize("mode", [{}, {"VAMD_MEGACYCLE": 1},
                                  {"VAMD_CHAIN_CHUNK": 4}],
                         ids=["default", "megacycle", "chain4"])
def test_plan_with_two_rule_classes(monkeypatch, mode):
    from volcano_amd.scheduler.plan import run_plan_hip
    case, want = plan_oracle()
    sg.set_mode(monkeypatch, **mode)
    plan = build(case, sg.DEV)
    res = run_plan_hip(plan)
    torch.cuda.synchronize()
    sc.compare_spread(want, sc.spread_snapshot(plan, res))
