"""CPU checks of the inputs the GPU kernel tests rely on.

* every dyadic case scores bit-identically in f32 and in float64, so the
  GPU tests may demand bit-equal scores and exact tie order;
* the f32 oracle's error with the balanced-allocation term, which fixes
  the tolerance the GPU test allows the kernel;
* every plan case is non-vacuous on the oracle alone (reverts, quota cuts,
  index-decided ties, exhausted candidate lists, wide touched sets);
* the result comparator notices a swapped tie and an off-by-one count.
"""

import functools

import numpy as np
import pytest
import torch

import _kernel_cases as kc


def _score_inputs():
    for N in kc.SCORE_NS:
        for R, W in kc.SCORE_RW:
            for seed in range(3):
                yield kc.dyadic_state(N, R, W, seed)
    yield kc.dyadic_state(*kc.GRID_WRAP, seed=0)


def test_dyadic_scores_are_exact_in_f32():
    checked = 0
    for st in _score_inputs():
        for bias in (None, st["bias"]):
            for wl, wm in kc.SCORE_WEIGHTS:
                s, cap = kc.oracle_score_cap(st, w_least=wl, w_most=wm,
                                             bias=bias, tolerated=-1)
                want = torch.from_numpy(kc.score_f64(
                    st, w_least=wl, w_most=wm, bias=bias)).float()
                feas = s > kc.NEG_INF
                assert kc.same_bits(s[feas], want[feas])
                checked += int(feas.sum())
    assert checked > 1000


def test_f32_oracle_error_with_balanced_term():
    worst = 0.0
    for st in _score_inputs():
        for bias in (None, st["bias"]):
            for wl, wm in kc.SCORE_WEIGHTS:
                s, _ = kc.oracle_score_cap(st, w_least=wl, w_most=wm,
                                           w_bal=kc.W_BAL, bias=bias,
                                           tolerated=-1)
                want = kc.score_f64(st, w_least=wl, w_most=wm,
                                    w_bal=kc.W_BAL, bias=bias)
                feas = (s > kc.NEG_INF).numpy()
                if feas.any():
                    worst = max(worst, float(np.abs(
                        s.double().numpy()[feas] - want[feas]).max()))
    # the recorded figure is what was measured, not a loose cap
    assert 0.5 * kc.BAL_ERR_F32 < worst <= kc.BAL_ERR_F32, worst


CASES = kc.plan_cases()


@functools.lru_cache(maxsize=None)
def _oracle(name):
    case = CASES[name][0]()
    snap, records, plan = kc.run_oracle(case)
    return case, snap, records, plan


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_case_is_non_vacuous(name):
    case, snap, records, _ = _oracle(name)
    _, base, chunks = CASES[name]
    cond = kc.plan_conditions(case, snap, records)
    for key in base:
        assert cond[key], f"{name}: oracle run shows no {key}"
    for chunk, key in chunks:
        cond = kc.plan_conditions(case, snap, records, chunk=chunk)
        assert cond[key], f"{name}: chunk {chunk} shows no {key}"
    rs = {c["req"].shape[0] for c in case.classes}
    assert rs == {case.R}
    assert {c["use_future"] for c in case.classes} == {True, False}
    assert any(c["bias_row"] is not None for c in case.classes)
    assert any(c["bias_row"] is None for c in case.classes)
    assert {c["queue_idx"] for c in case.classes} == {0, 1, 2}


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_case_scores_are_exact(name):
    """Every score the oracle computed while running the plan — against
    usage that earlier classes already changed — is exact too."""
    case, _, records, plan = _oracle(name)
    for c, rec in enumerate(records):
        cp = plan.classes[c]
        st = dict(case.state, used=rec["used"])
        bias = plan.bias if cp.bias is None else torch.from_numpy(cp.bias)
        want = torch.from_numpy(kc.score_f64(
            st, req=torch.from_numpy(cp.req), w_least=cp.w_least,
            w_most=cp.w_most, bias=bias)).float()
        feas = rec["score"] > kc.NEG_INF
        assert kc.same_bits(rec["score"][feas], want[feas]), f"class {c}"


def test_bulk_plan_cases_hold_a_bulk_class_that_reverts():
    case, snap, _, _ = _oracle("bulk-multi-R5W1")
    assert case.classes[0]["ntasks"] == 600
    assert snap["job_flag"][0] == 0 and snap["log_len"][0] > 0
    assert snap["class_placed"][0] == 0
    case, snap, _, _ = _oracle("bulk-single-R5W1")
    assert case.classes[0]["ntasks"] == 600 and snap["class_placed"][0] >= 300


def _copy(snap):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v)
            for k, v in snap.items()}


def _tied_pair(snap, records):
    """Two consecutive log entries of one class with equal scores."""
    for c, rec in enumerate(records):
        off, n = int(snap["log_off"][c]), int(snap["log_len"][c])
        nodes = snap["log_nodes"][off:off + n]
        for e in range(n - 1):
            if rec["score"][int(nodes[e])] == rec["score"][int(nodes[e + 1])] \
                    and snap["log_counts"][off + e] \
                    == snap["log_counts"][off + e + 1] > 0:
                return off + e
    raise AssertionError("case has no tied neighbours in any log")


def test_comparator_accepts_identical_and_rejects_swapped_tie():
    _, snap, records, _ = _oracle("fused-R5W1")
    kc.compare_results(snap, _copy(snap))
    bad = _copy(snap)
    e = _tied_pair(snap, records)
    bad["log_nodes"][[e, e + 1]] = bad["log_nodes"][[e + 1, e]]
    # same multiset of (node, count), same usage: only the order differs
    with pytest.raises(AssertionError, match="log_nodes"):
        kc.compare_results(snap, bad)


def test_comparator_rejects_count_off_by_one():
    _, snap, _, _ = _oracle("fused-R5W1")
    bad = _copy(snap)
    e = int(np.flatnonzero(snap["log_counts"] > 0)[0])
    bad["log_counts"][e] += 1
    with pytest.raises(AssertionError, match="log_counts"):
        kc.compare_results(snap, bad)


def test_comparator_rejects_state_and_flag_differences():
    _, snap, _, _ = _oracle("fused-R5W1")
    for key in ("used", "queue_alloc", "class_placed", "job_placed",
                "log_len"):
        bad = _copy(snap)
        bad[key].flat[0] += 1
        with pytest.raises(AssertionError):
            kc.compare_results(snap, bad)
    multi = next(j for j, (b, e) in enumerate(snap["jobs"]) if e - b > 1)
    bad = _copy(snap)
    bad["job_flag"][multi] ^= 1
    with pytest.raises(AssertionError, match="flag"):
        kc.compare_results(snap, bad)
