"""The inputs of ``test_domain_scores_gpu.py`` can tell a wrong kernel from a
right one: the sequential oracles agree with the independent models and with
each other on signed, denormal and near-tied scores, every wrong variant of
the integer key is caught by some case, and the cases reach the branches
they exist for.  Everything is bit for bit; no tolerance anywhere."""

import functools

import numpy as np
import pytest

import _affinity_cases as ac
import _domain_score_cases as dc
import _kernel_cases as kc
import _spread_cases as sc

ALL = {**dc.SPREAD_CASES, **dc.AFFINITY_CASES}


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32),
                          np.ascontiguousarray(b).view(np.int32))


def same_result(want, got, *, counts=True):
    n = want["log_len"]
    assert got["log_len"] == n
    assert list(got["log_nodes"][:n]) == list(want["log_nodes"][:n])
    assert list(got["log_counts"][:n]) == list(want["log_counts"][:n])
    assert got["placed"] == want["placed"]
    assert got["job_placed"] == want["job_placed"]
    if counts:
        assert list(got["dom_count"]) == list(want["dom_count"])
    assert same_bits(got["used"], want["used"])
    assert same_bits(got["queue_alloc"], want["queue_alloc"])


# ---- the families ---------------------------------------------------------

def test_special_values_are_those_of_the_plain_select_test():
    import test_ops_gpu_edges as edges
    drawn = edges.special_scores(4096, 0).numpy()
    finite = drawn[drawn > dc.NEG_INF]
    assert set(finite.view(np.uint32).tolist()) == \
        set(dc.SPECIAL.view(np.uint32).tolist())


@pytest.mark.parametrize("family", list(dc.FAMILIES))
def test_families(family):
    s = dc.FAMILIES[family](4096, np.random.RandomState(1))
    assert s.dtype == np.float32 and s.shape == (4096,)
    assert np.isfinite(s).all()                 # no NaN, no +inf, no -inf yet
    assert (s < 0).any() and (s > 0).any()
    u = s.view(np.uint32)
    denormal = (s != 0) & (np.abs(s) < dc.MIN_NORMAL)
    if family == "special":
        assert denormal.any() and (u == 0x80000000).any() and (u == 0).any()
    if family == "ladder":
        v = np.unique(s)
        # one ulp apart: below and above +-1, around +-0.7, and on both
        # sides of the smallest normal
        for lo, hi in ((0.99, 1.01), (-1.01, -0.99), (0.69, 0.71),
                       (-0.71, -0.69), (0.0, 2.0 ** -125),
                       (-(2.0 ** -125), 0.0)):
            w = v[(v > lo) & (v < hi)]
            assert len(w) == 7
            assert (np.diff(np.sort(w.view(np.int32))) == 1).all()
        assert denormal.any() and (np.abs(s) == dc.MIN_NORMAL).any()
        assert (s == 1.0).any() and (s < 1.0)[s > 0.9].any()
    if family == "dense":
        assert len(np.unique(s)) > 4000 and 0.4 < (s < 0).mean() < 0.6
    if family == "grid":
        assert (u == 0x80000000).sum() > 100 and (u == 0).sum() > 100
        assert len(np.unique(s)) == 7


def test_default_draws_are_unchanged():
    """``scores=None`` leaves the cases of the older files as they were."""
    a = sc.random_case("x", 65, 3, 1, 5, 3)
    assert set(np.unique(a.score[a.score > sc.NEG_INF])) <= \
        {0.0, 0.25, 0.5, 0.75}
    b = ac.base_case("x", 65, 3, 4, 3, ac.ANTI)
    assert set(np.unique(b.score[b.score > ac.NEG_INF])) <= \
        {0.0, 0.25, 0.5, 0.75}
    plain = sc.spread_plan_case(N=65, bulk=False)
    twin = sc.spread_plan_case(N=65, bulk=False, inexact=True)
    assert plain.base.w_bal == 0.0 and twin.base.w_bal == 1.0
    assert plain.base.jobs == twin.base.jobs
    assert all(np.array_equal(p[0], t[0])
               for p, t in zip(plain.groups, twin.groups))


# ---- 2a: oracle against the independent models ---------------------------

def model_expected(case):
    if dc.rule_of(case) == dc.SPREAD:
        seq, count, _ = sc.model_of(case)
    else:
        seq, count = ac.model_of(case)
    return dc.expected(case, seq, count)


@pytest.mark.parametrize("name", list(ALL))
def test_oracle_equals_model(name):
    case, got = dc.oracle(name)
    want = model_expected(case)
    same_result(want, got)
    assert got["reverted"] == want["reverted"]


# ---- 2b: the oracles agree with each other -------------------------------

@pytest.mark.parametrize("name", list(dc.RELATION_CASES))
def test_domain_rule_that_cannot_bind_is_the_plain_select(name):
    """Spread with unbounded skew over labelled nodes and zero counts,
    anti-affinity over one domain per node (caps clipped to 1), affinity
    with a single hosting domain: each is reference.select_commit."""
    case, got = dc.oracle(name)
    assert got["placed"] > 0 and not got["reverted"]
    kind = name.split("-")[0]
    if kind == "spread":
        assert case.max_skew == dc.UNBOUNDED and (case.dom_of >= 0).all()
        assert not case.dom_count.any()
        want = dc.plain_select(case, mask_cap=True)
    elif kind == "anti":
        assert np.array_equal(case.dom_of, np.arange(case.N))
        assert not case.dom_count.any()
        want = dc.plain_select(case, clip=True)
    else:
        assert case.D == 1 and case.dom_count.tolist() == [1]
        want = dc.plain_select(case)
    same_result(want, got, counts=False)


# ---- 2c: wrong keys -------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fill_log(name, mutant=None):
    case, _ = dc.oracle(name)
    seq, count = dc.key_fill(case, dc.MUTANTS[mutant] if mutant
                             else dc.spread_key)
    return sc.log_of(seq), count


@pytest.mark.parametrize("name", list(ALL) + list(dc.RELATION_CASES))
def test_fill_by_the_right_key_is_the_oracle(name):
    case, got = dc.oracle(name)
    (nodes, counts), count = fill_log(name)
    n = got["log_len"]
    before = got["before"]
    assert before["log_nodes"][:n].tolist() == nodes
    assert before["log_counts"][:n].tolist() == counts
    assert before["placed"] == sum(counts)
    if not got["reverted"]:
        assert got["dom_count"].tolist() == count


# family -> the mutants it must catch on its own
KILLS = {
    "special": {"no-negative-flip", "no-zero-fold", "denormals-flushed",
                "index-not-inverted", "upper-48-bits"},
    "ladder": {"no-negative-flip", "denormals-flushed"},
    "dense": {"no-negative-flip"},
    "grid": {"no-negative-flip", "no-zero-fold", "index-not-inverted",
             "upper-48-bits"},
}


@pytest.mark.parametrize("mutant", list(dc.MUTANTS))
def test_every_wrong_key_changes_a_log(mutant):
    """Which family catches which wrong key:

    * no flip of negative patterns: every family (two negative scores are
      ordered the wrong way round);
    * no -0.0 fold: special and grid, the two with both zeros (-0.0 at the
      lower index loses against +0.0);
    * denormals flushed: special and ladder, the two with denormals (1e-45,
      1e-40 and the steps below 2**-126 collapse onto zero);
    * index not inverted, key cut to 48 bits: special and grid, the two with
      tie groups (the tie goes to the wrong node).  ladder ties too, dense
      has no ties and cannot catch either.

    The families named catch it in a spread and in an anti-affinity case
    (the two rules whose kernels use the key), and every wrong key changes
    the log of some case of each of the three rules."""
    killed = {fam: {dc.SPREAD: 0, dc.AFFINITY: 0, dc.ANTI: 0}
              for fam in dc.FAMILIES}
    for name in ALL:
        fam = next(f for f in dc.FAMILIES if f"{f}-" in name)
        if fill_log(name, mutant)[0] != fill_log(name)[0]:
            killed[fam][dc.rule_of(dc.oracle(name)[0])] += 1
    print(mutant, killed)
    for fam, must in KILLS.items():
        if mutant in must:
            assert killed[fam][dc.SPREAD] and killed[fam][dc.ANTI], \
                (mutant, fam, killed[fam])
    for rule in (dc.SPREAD, dc.AFFINITY, dc.ANTI):
        assert any(killed[fam][rule] for fam in dc.FAMILIES), (mutant, rule)
    if mutant in ("no-zero-fold", "denormals-flushed"):
        assert not any(killed["dense"].values())


# ---- 2d: the spread cases reach what they exist for ----------------------

FLOORS = dict(blocked=10, tie3=10, negative_over_blocked=10, zero_pair=5,
              denormal=5, rescan=5, multi_count=5)


def test_spread_cases_are_not_vacuous():
    seen = dict.fromkeys(FLOORS, 0)
    for name in dc.SPREAD_CASES:
        case, got = dc.oracle(name)
        seq, _, flags = dc.key_fill(case, stats=True)
        assert sc.log_of(seq)[0] == \
            got["log_nodes"][:got["log_len"]].tolist()
        for k, v in flags.items():
            seen[k] += bool(v)
        seen["multi_count"] += bool((got["before"]["log_counts"] > 1).any())
    print(seen)
    for k, floor in FLOORS.items():
        assert seen[k] >= floor, (k, seen)


def test_feature_cases():
    for fam in dc.FAMILIES:
        case, got = dc.oracle(f"{fam}-gang-revert")
        assert got["reverted"] and got["before"]["placed"] > 0
        assert got["dom_count"].tolist() == case.dom_count.tolist()
        assert same_bits(got["used"], case.used)
        case, got = dc.oracle(f"{fam}-quota")
        assert got["placed"] == sc.quota_of(case) == 11 < case.ntasks
        case, got = dc.oracle(f"{fam}-dead-domain")
        assert got["placed"] < case.ntasks          # stopped by the skew
        case, got = dc.oracle(f"{fam}-unbalanced")
        assert case.dom_count.max() - case.dom_count.min() > case.max_skew
        assert got["placed"] > 0
        case, got = dc.oracle(f"{fam}-cap-one")
        assert case.cap.max() == 1 and (case.N, case.D) == (1025, 3)
        assert got["log_len"] == got["placed"] == case.ntasks
    for name in dc.SPREAD_CASES:
        case, _ = dc.oracle(name)
        assert case.ntasks <= 160 and case.ntasks * case.N <= 160 * 2049


def test_affinity_cases():
    heads = []                  # scores of the nodes anti-affinity placed on
    for name in dc.AFFINITY_CASES:
        case, got = dc.oracle(name)
        assert got["placed"] > 0, name
        if case.mode == dc.ANTI:
            heads.append(case.score[got["log_nodes"][:got["log_len"]]])
        if name.startswith("aff-empty"):
            assert not case.dom_count.any()
        elif name.startswith("aff-hosting"):
            assert (case.dom_count > 0).any() and (case.dom_count == 0).any()
        else:
            assert case.ntasks == 600
            assert (case.dom_count > 0).any() and (case.dom_count == 0).any()
            if case.D > 3:
                assert got["log_len"] >= 20        # an order worth comparing
    # a domain's head is negative, a denormal, -0.0 and +0.0 somewhere
    h = np.concatenate(heads)
    bits = h.view(np.uint32)
    assert (h < 0).sum() >= 20
    assert ((h != 0) & (np.abs(h) < dc.MIN_NORMAL)).sum() >= 20
    assert (bits == 0x80000000).sum() >= 5 and (bits == 0).sum() >= 5


# ---- section 4: scores of the score kernel's formula ---------------------

@pytest.mark.parametrize("name", list(dc.SCORED_STATES))
def test_shifted_scores_straddle_zero(name):
    """The bias shift of -1.25 puts at least 20 % of the feasible oracle
    scores on each side of zero (measured: 24 % to 76 % negative over the
    twelve states)."""
    st, kw = dc.scored_state(name)
    score, cap = kc.oracle_score_cap(st, **kw)
    s = score.numpy()
    feas = s[s > dc.NEG_INF]
    neg = float((feas < 0).mean())
    print(name, len(feas), round(neg, 3))
    assert len(feas) >= 20
    assert 0.2 <= neg <= 0.8
    # and the domain rules have something to decide on them
    for rule in (dc.SPREAD, "aff-empty", "aff-hosting", "anti"):
        case = dc.scored_case(name, s, cap.numpy(), rule, 3)
        assert dc.run_oracle(case)["placed"] > 0


# ---- whole plans ----------------------------------------------------------

def test_spread_twin_plan_roles():
    """The role conditions of the exact spread plan hold on its inexact,
    bias-shifted twin (plain run_plan_torch)."""
    import test_spread_gpu as tsg
    case = dc.spread_twin()
    signs = []
    with dc.recording_signs(signs):
        snap, records = sc.run_plan_oracle(case)
    # the bulk-sized spread class walks far down both sides of zero
    assert any(r["negative"] >= 100 and r["positive"] >= 100 for r in signs)
    tsg.plan_non_vacuous(True, oracle=lambda bulk: (case, snap, records))
    assert case.base.w_bal == 1.0
    scores = np.concatenate([np.asarray(r["score"]) for r in records])
    scores = scores[scores > sc.NEG_INF]
    assert (scores < 0).mean() >= 0.2 and (scores > 0).mean() >= 0.2
    # inexact: the scores are no multiples of 2**-10
    assert (np.round(scores * 1024) != scores * 1024).mean() > 0.9


@pytest.mark.parametrize("N", list(dc.AFFINITY_TWINS))
def test_affinity_twin_plan_roles(N):
    case = dc.affinity_twin(N)
    signs = []
    with dc.recording_signs(signs):
        snap, records = ac.run_plan_oracle(case)
    dc.affinity_plan_conditions(case, snap, records)
    assert case.base.w_bal == 1.0
    # some anti-affinity head (N = 65) / a long affinity fill (N = 1500)
    # lies below zero
    few = 1 if N < 512 else 20
    assert any(r["rule"] == "affinity" and r["negative"] >= few
               and (r["positive"] >= few or r["arg"] == dc.ANTI)
               for r in signs), signs
    plain, _ = ac.run_plan_oracle(case, rules=False)
    assert not np.array_equal(plain["log_nodes"], snap["log_nodes"])
