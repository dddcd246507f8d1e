"""``reference.affinity_select_commit`` against the independent per-instance
model of ``_affinity_cases`` (bit-equal: the inputs are exact in f32), the
properties each named case exists for, and non-vacuity against the
unconstrained ``select_commit``."""

import functools

import numpy as np
import pytest
import torch

import _affinity_cases as ac
from volcano_amd.ops import reference as ref

ALL = {**{f"aff-{k}": v for k, v in ac.AFFINITY_CASES.items()},
       **{f"anti-{k}": v for k, v in ac.ANTI_CASES.items()}}


@functools.lru_cache(maxsize=None)
def oracle(name):
    case = ALL[name]()
    return case, ac.run_oracle(case)


def expected(case):
    """What the model says the oracle must leave behind."""
    seq, count = ac.model_of(case)
    nodes, counts = ac.log_of(seq)
    revert = case.fuse_min >= 0 and len(seq) < case.fuse_min
    used = case.used.copy()
    qa = case.queue_alloc.copy()
    if not revert:
        for n, k in zip(nodes, counts):
            used[n] += np.float32(k) * case.req
        qa += np.float32(len(seq)) * case.req
    return dict(nodes=nodes, counts=[0] * len(nodes) if revert else counts,
                placed=0 if revert else len(seq),
                dom_count=case.dom_count.tolist() if revert else count,
                used=used, queue_alloc=qa, reverted=revert, seq=seq)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32),
                          np.ascontiguousarray(b).view(np.int32))


@pytest.mark.parametrize("name", list(ALL))
def test_oracle_equals_model(name):
    case, got = oracle(name)
    want = expected(case)
    n = len(want["nodes"])
    assert got["log_len"] == n
    assert got["log_nodes"][:n].tolist() == want["nodes"]
    assert got["log_counts"][:n].tolist() == want["counts"]
    assert got["placed"] == want["placed"]
    assert got["job_placed"] == 7 + want["placed"]
    assert got["dom_count"].tolist() == want["dom_count"]
    assert got["reverted"] == want["reverted"]
    assert same_bits(got["used"], want["used"])
    assert same_bits(got["queue_alloc"], want["queue_alloc"])


def test_shapes_are_covered():
    shapes = {(c.N, c.D, len(c.req)) for c in (f() for f in ALL.values())}
    for nd in ((1, 1), (63, 3), (65, 3), (1025, 1025), (1500, 7)):
        assert any(s[:2] == nd for s in shapes), nd
    assert {s[2] for s in shapes} == {1, 4}
    for lst in (ac.AFFINITY_CASES, ac.ANTI_CASES):
        assert any(c.N >= 512 and c.ntasks >= 512
                   for c in (f() for f in lst.values()))


@pytest.mark.parametrize("cases,prefix", [(ac.AFFINITY_CASES, "aff-"),
                                          (ac.ANTI_CASES, "anti-")],
                         ids=["affinity", "anti"])
def test_rule_changes_the_outcome(cases, prefix):
    """Non-vacuity: without the rule at least half of the cases log
    something else."""
    differ = 0
    for name in cases:
        case, got = oracle(prefix + name)
        nodes, counts, _ = ac.run_unconstrained(case)
        n = got["log_len"]
        before = got["before"]
        differ += (before["log_nodes"][:n].tolist(),
                   before["log_counts"][:n].tolist()) != (nodes, counts)
    assert 2 * differ >= len(cases), (differ, len(cases))


# ---- affinity -------------------------------------------------------------

def test_empty_group_anchors_at_the_best_node():
    case, got = oracle("aff-anchor-best")
    best = int(got["log_nodes"][0])
    assert case.score[best] == 1.0
    d = case.dom_of[best]
    n = got["log_len"]
    assert (case.dom_of[got["log_nodes"][:n]] == d).all()
    assert got["placed"] == case.ntasks and n > 1
    assert got["dom_count"].tolist() == [0, 0, case.ntasks]


def test_anchor_tie_goes_to_the_lower_index():
    case, got = oracle("aff-anchor-tie")
    top = np.flatnonzero(case.score == 1.0)
    assert len(top) == 2 and case.dom_of[top[0]] != case.dom_of[top[1]]
    assert got["log_nodes"][0] == top[0]
    assert got["dom_count"][case.dom_of[top[1]]] == 0


def test_signed_zero_tie():
    for name in ("aff-zero-tie", "anti-zero-tie"):
        case, got = oracle(name)
        zeros = np.flatnonzero(case.score == 0.0)
        assert len(zeros) == 2
        assert np.signbit(case.score[zeros[0]]) and \
            not np.signbit(case.score[zeros[1]])
        assert got["log_nodes"][0] == zeros[0]
        assert zeros[1] not in got["log_nodes"][:got["log_len"]].tolist() \
            or name.startswith("aff")


def test_best_node_without_label_is_skipped():
    case, got = oracle("aff-best-unlabelled")
    best = int(np.argmax(case.score))
    assert case.dom_of[best] < 0 and case.cap[best] >= case.ntasks
    assert best not in got["log_nodes"][:got["log_len"]].tolist()
    assert got["placed"] == case.ntasks


def test_fill_runs_across_both_hosting_domains():
    case, got = oracle("aff-two-of-three")
    n = got["log_len"]
    doms = case.dom_of[got["log_nodes"][:n]]
    assert set(doms.tolist()) == {0, 2}
    sc = case.score[got["log_nodes"][:n]]
    assert (np.diff(sc) <= 0).all()            # one fill, by score
    assert got["dom_count"][1] == 0
    assert got["placed"] == case.ntasks


def test_members_in_infeasible_domains_block_the_class():
    case, got = oracle("aff-dead-domains")
    assert got["placed"] == 0 and got["log_len"] == 0
    assert got["dom_count"].tolist() == case.dom_count.tolist()
    assert ac.run_unconstrained(case)[2] == case.ntasks


def test_budget_zero_places_no_anchor():
    case, got = oracle("aff-budget-zero")
    assert ac.quota_of(case) == 0
    assert got["placed"] == 0 and got["dom_count"].tolist() == [0, 0, 0]


def test_identity_map_anchor_capacity():
    case, got = oracle("aff-identity-cap3")
    assert got["placed"] == 3 and got["log_len"] == 1
    assert got["log_nodes"][0] == 700 and got["dom_count"][700] == 3
    assert got["dom_count"].sum() == 3


def test_fuse_min_revert_gives_the_anchor_back():
    for name in ("aff-fuse-min-revert", "anti-fuse-min-revert"):
        case, got = oracle(name)
        assert got["reverted"] and got["before"]["placed"] > 0
        assert got["before"]["dom_count"].tolist() != \
            case.dom_count.tolist()
        assert got["dom_count"].tolist() == case.dom_count.tolist()
        assert got["placed"] == 0 and not got["log_counts"].any()


# ---- anti-affinity --------------------------------------------------------

def test_one_per_open_domain_in_head_order():
    case, got = oracle("anti-one-per-open")
    n = got["log_len"]
    assert n == 3 and got["log_counts"][:n].tolist() == [1, 1, 1]
    nodes = got["log_nodes"][:n]
    assert sorted(case.dom_of[nodes].tolist()) == [0, 1, 2]
    sc = case.score[nodes]
    assert (np.diff(sc) <= 0).all()
    ok = (case.score > ac.NEG_INF) & (case.cap > 0)
    for node in nodes:
        peers = np.flatnonzero(ok & (case.dom_of == case.dom_of[node]))
        assert case.score[node] == case.score[peers].max()
        assert node == peers[case.score[peers] == case.score[node]][0]
    assert got["dom_count"].tolist() == [1, 1, 1]


def test_occupied_domains_are_closed():
    case, got = oracle("anti-occupied-closed")
    n = got["log_len"]
    assert n == 2 and got["placed"] == 2
    assert 0 not in case.dom_of[got["log_nodes"][:n]].tolist()
    assert got["dom_count"].tolist() == [1, 1, 1]


def test_head_tie_goes_to_the_lower_index():
    case, got = oracle("anti-head-tie")
    top = np.flatnonzero((case.score == 1.0) & (case.dom_of == 1))
    assert len(top) == 2
    nodes = got["log_nodes"][:got["log_len"]].tolist()
    assert top[0] in nodes and top[1] not in nodes


def test_more_tasks_than_open_domains():
    case, got = oracle("anti-more-than-open")
    assert got["placed"] == 3 < case.ntasks


def test_caps_are_clipped_to_one():
    case, got = oracle("anti-caps-clipped")
    n = got["log_len"]
    assert (case.cap[got["log_nodes"][:n]] > 1).all()
    assert got["log_counts"][:n].tolist() == [1] * n and n == 3


def test_identity_map_is_the_plain_fill_with_unit_caps():
    case, got = oracle("anti-identity")
    nodes, counts, placed = ac.run_unconstrained(case, clip=True)
    n = got["log_len"]
    assert got["log_nodes"][:n].tolist() == nodes
    assert got["log_counts"][:n].tolist() == counts
    assert got["placed"] == placed == case.ntasks


def test_budget_clamp():
    case, got = oracle("anti-budget-clamp")
    assert ac.quota_of(case) == 2 < case.ntasks
    assert got["placed"] == 2 and got["dom_count"].sum() == 2


def test_mode_is_validated():
    case = ac.b_single_node()
    case.mode = 0
    with pytest.raises(ValueError):
        ac.run_oracle(case)


def test_plan_validation():
    """finalize() rejects an unknown group, a bundle and a second rule."""
    from volcano_amd.scheduler.plan import BundleEntry
    case = ac.affinity_plan_case(N=65)
    c = case.roles["aff_anchor"]
    for breakage in ("group", "mode", "bundle", "spread"):
        plan = ac.build_affinity_plan(case, "cpu")
        cp = plan.classes[c]
        if breakage == "group":
            cp.affinity = (len(plan.spread_groups), 1)
        elif breakage == "mode":
            cp.affinity = (0, 3)
        elif breakage == "bundle":
            cp.bundle = [BundleEntry("j", [], 1, 1)]
        else:
            cp.spread = (1, 1)
        plan.bias = None            # already folded by the first finalize
        with pytest.raises(ValueError):
            plan.finalize()


@pytest.mark.parametrize("N", [65, 1500])
def test_plan_oracle_is_not_vacuous(N):
    case = ac.affinity_plan_case(N=N)
    snap, records = ac.run_plan_oracle(case)
    r = case.roles
    assert len(records) == len(case.affinity)
    placed = snap["class_placed"]
    # the first job anchored, then reverted in place: counts restored
    assert records[0]["placed"] == 6 and sum(records[0]["after"]) == 6
    assert placed[r["aff_revert"]] == 0
    assert records[1]["count"] == [0, 0, 0] and records[1]["placed"] == 9
    # the gang's affinity role placed, the job reverted, counts came back
    gang = records[2]
    assert gang["placed"] == 7 and placed[r["gang_aff"]] == 0
    later = [rec for rec in records if rec["mode"] == ac.AFFINITY][3]
    assert later["count"] == records[1]["after"]
    # anti: open racks only, the later job sees the first one's racks shut
    anti = [rec for rec in records if rec["mode"] == ac.ANTI]
    assert anti[0]["placed"] == 3 and anti[1]["count"] == anti[0]["after"]
    assert anti[1]["placed"] == 2 and min(anti[1]["after"]) >= 1
    assert placed[r["spread"]] > 0 and placed[r["host"]] > 0
    if N >= 512:
        assert placed[r["aff_bulk"]] >= 512
    # and the rules matter: the same plan without them decides otherwise
    plain, _ = ac.run_plan_oracle(case, rules=False)
    assert not np.array_equal(plain["log_nodes"], snap["log_nodes"])
