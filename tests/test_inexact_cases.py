"""CPU checks of the inexact input family and of the float64 validator.

* the error bounds recorded in ``_kernel_cases`` (f32 oracle and a numpy
  replay of the kernel's operation order, fused and unfused, each against
  the float64 formula) are what this run measures;
* every inexact plan case is non-vacuous on the oracle alone, has tied and
  forced neighbours in its logs and next to no ambiguous ones;
* ``validate_plan`` accepts the oracle's result of every case, exact and
  inexact, and rejects six corruptions;
* the byte-scale inputs of the discard tests leave a residue under plain
  f32 add-then-subtract.
"""

import functools

import numpy as np
import pytest
import torch

import _kernel_cases as kc

CASES = kc.inexact_plan_cases()
DYADIC = kc.plan_cases()

# tied / forced / ambiguous neighbours per case at tol = 2 * KERNEL_ERR, as
# the seeds in _kernel_cases give them on the oracle's logs: between 25 and
# 369 pairs per case, every case has tied and forced ones, and two cases
# have one ambiguous pair each (1 of 66 and 1 of 130; the cap is 2 %)
AMBIGUOUS_CAP = 0.02


@functools.lru_cache(maxsize=None)
def _oracle(name):
    case = CASES[name][0]()
    snap, records, plan = kc.run_oracle(case)
    return case, snap, records, plan


@functools.lru_cache(maxsize=None)
def _dyadic(name):
    case = DYADIC[name][0]()
    snap, _, _ = kc.run_oracle(case)
    return case, snap


def _errors(st, feas, s32, **kw):
    """|s - float64 formula| maxima over ``feas`` for the f32 oracle score
    ``s32`` and the two kernel-order replays."""
    want = kc.score_f64(st, **kw)
    out = [float(np.abs(s32.double().numpy() - want)[feas].max())]
    for fused in (False, True):
        got = kc.kernel_replay_f32(st, fused=fused, **kw)
        out.append(float(np.abs(got.astype(np.float64) - want)[feas].max()))
    return out


@functools.lru_cache(maxsize=None)
def _case_errors(name):
    case, _, records, plan = _oracle(name)
    worst = [0.0, 0.0, 0.0]
    for c, rec in enumerate(records):
        cp = plan.classes[c]
        feas = (rec["score"] > kc.NEG_INF).numpy()
        if not feas.any():
            continue
        st = dict(case.state, used=rec["used"])
        err = _errors(st, feas, rec["score"], req=torch.from_numpy(cp.req),
                      w_least=cp.w_least, w_most=cp.w_most, w_bal=cp.w_bal,
                      bias=kc.class_bias(case, c))
        worst = [max(a, b) for a, b in zip(worst, err)]
    return worst


def test_inexact_inputs_are_inexact():
    st = kc.dyadic_state(1000, 5, 1, 3, inexact=True)
    ex = kc.dyadic_state(1000, 5, 1, 3)
    a = st["alloc"].numpy()
    assert not (np.log2(a) == np.round(np.log2(a))).any()
    assert set(np.unique(ex["alloc"].numpy() - a)) == {1.0, 3.0}
    w = st["dim_w"].numpy()
    assert set(w.tolist()) <= {1.0, 2.0, 3.0}
    assert np.log2(w.sum()) != np.round(np.log2(w.sum()))
    for k in ("used", "extra", "req"):
        assert np.array_equal(st[k].numpy(), np.round(st[k].numpy()))
    for k in ("ready", "taints", "planes", "req"):
        assert torch.equal(st[k], ex[k])
    # the shapes that must still place something keep dim 0
    one = kc.dyadic_state(600, 5, 1, 3, cap_one=True, inexact=True)
    assert set(one["alloc"][:, 0].tolist()) == {16.0}
    assert set(one["used"][:, 0].tolist()) == {15.0}
    # and the oracle's score is really not the float64 one any more
    s, _ = kc.oracle_score_cap(st, tolerated=-1, w_bal=1.0, bias=st["bias"])
    want = kc.score_f64(st, w_bal=1.0, bias=st["bias"])
    feas = (s > kc.NEG_INF).numpy()
    assert (s.double().numpy()[feas] != want[feas]).mean() > 0.5


def test_every_inexact_class_has_the_balanced_term():
    for name in sorted(CASES):
        _, _, _, plan = _oracle(name)
        assert {cp.w_bal for cp in plan.classes} == {1.0}, name
    for name in sorted(DYADIC):
        case, _ = _dyadic(name)
        assert case.w_bal == 0.0


def test_recorded_error_bounds_are_the_measured_ones():
    worst = [0.0, 0.0, 0.0]
    for name in sorted(CASES):
        worst = [max(a, b) for a, b in zip(worst, _case_errors(name))]
    print("oracle / unfused / fused error vs float64:", worst)
    for got, rec in zip(worst, (kc.SCORE_ERR_F32, kc.REPLAY_ERR_UNFUSED,
                                kc.REPLAY_ERR_FUSED)):
        # the recorded figure is what was measured, not a loose cap
        assert 0.5 * rec < got <= rec, worst
    assert kc.KERNEL_ERR == 2 * max(kc.SCORE_ERR_F32, kc.REPLAY_ERR_UNFUSED,
                                    kc.REPLAY_ERR_FUSED)


def test_rand_state_error_bound_is_the_measured_one():
    """test_ops_gpu.test_score_cap_matches_oracle holds the kernel to
    RAND_KERNEL_ERR of the float64 formula on these inputs."""
    import test_ops_gpu as tg
    worst = 0.0
    for N, R in kc.RAND_SCORE_SHAPES:
        for seed in kc.RAND_SCORE_SEEDS:
            st, kw, mask = kc.rand_score_case(tg.rand_state, N, R, seed)
            s, _ = kc.oracle_score_cap(st, **kw, **mask)
            feas = (s > kc.NEG_INF).numpy()
            worst = max(worst, *_errors(st, feas, s, **kw))
    print("rand_state error vs float64:", worst)
    assert 0.5 * kc.RAND_KERNEL_ERR / 2 < worst <= kc.RAND_KERNEL_ERR / 2, \
        worst


@pytest.mark.parametrize("name", sorted(CASES))
def test_inexact_case_is_non_vacuous(name):
    case, snap, records, _ = _oracle(name)
    _, base, chunks = CASES[name]
    cond = kc.plan_conditions(case, snap, records)
    for key in base:
        assert cond[key], f"{name}: oracle run shows no {key}"
    for chunk, key in chunks:
        cond = kc.plan_conditions(case, snap, records, chunk=chunk)
        assert cond[key], f"{name}: chunk {chunk} shows no {key}"
    assert {c["use_future"] for c in case.classes} == {True, False}
    assert any(c["bias_row"] is not None for c in case.classes)
    assert {c["queue_idx"] for c in case.classes} == {0, 1, 2}
    # single-class discards are what part of the GPU suite is about
    assert any(e - b == 1 and snap["job_flag"][j] == 0
               for j, (b, e, _, _) in enumerate(case.jobs))


@pytest.mark.parametrize("name", sorted(CASES))
def test_validator_accepts_oracle_and_pairs_are_decided(name):
    case, snap, _, _ = _oracle(name)
    stats = kc.validate_plan(case, snap)
    pairs = sum(stats.values())
    print(name, stats)
    assert stats["tied"] >= 1 and stats["forced"] >= 1, stats
    assert stats["ambiguous"] <= AMBIGUOUS_CAP * pairs, stats


@pytest.mark.parametrize("name", sorted(DYADIC))
def test_validator_accepts_oracle_on_exact_cases(name):
    case, snap = _dyadic(name)
    kc.validate_plan(case, snap)


def _copy(snap):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v)
            for k, v in snap.items()}


def _pair(case, snap, want):
    """Log position of the first consecutive pair of kind ``want`` with
    equal counts (so a swap changes nothing but the order)."""
    tol = 2 * kc.KERNEL_ERR
    used = case.state["used"].clone()
    for j, (b, e, _, _) in enumerate(case.jobs):
        for c in range(b, e):
            d = case.classes[c]
            off, n = int(snap["log_off"][c]), int(snap["log_len"][c])
            nodes = snap["log_nodes"][off:off + n]
            counts = snap["log_counts"][off:off + n]
            bias = kc.class_bias(case, c)
            s64 = kc.score_f64(dict(case.state, used=used),
                               req=torch.from_numpy(d["req"]),
                               w_least=d["w_least"], w_most=d["w_most"],
                               w_bal=case.w_bal, bias=bias)
            # only the last entry can be cut by the budget: leave it out
            for k in range(n - 2):
                x, y = int(nodes[k]), int(nodes[k + 1])
                if not counts[k] == counts[k + 1] > 0:
                    continue
                same = all(torch.equal(case.state[f][x], case.state[f][y])
                           for f in ("alloc", "extra")) \
                    and torch.equal(used[x], used[y]) and bias[x] == bias[y]
                if want == "tied" and same:
                    return off + k
                if want == "forced" and not same and s64[x] - s64[y] > tol:
                    return off + k
            used.index_add_(0, torch.from_numpy(nodes).long(),
                            torch.from_numpy(counts).float()[:, None]
                            * torch.from_numpy(d["req"])[None, :])
    raise AssertionError(f"no {want} pair")


@pytest.mark.parametrize("name", ["fused-R5W1", "mega-N1000-R64W4",
                                  "chain-wide-N600-R5W1"])
def test_validator_rejects_corruptions(name):
    case, snap, _, _ = _oracle(name)
    kc.validate_plan(case, _copy(snap))

    def rejected(bad, match):
        with pytest.raises(kc.PlanInvalid, match=match):
            kc.validate_plan(case, bad)

    for kind, match in (("forced", "beats"), ("tied", "index order")):
        bad = _copy(snap)
        e = _pair(case, snap, kind)
        bad["log_nodes"][[e, e + 1]] = bad["log_nodes"][[e + 1, e]]
        rejected(bad, match)

    e = int(np.flatnonzero(snap["log_counts"] > 0)[0])
    bad = _copy(snap)
    bad["log_counts"][e] += 1
    rejected(bad, "counts")
    bad = _copy(snap)
    bad["log_counts"][e] -= 1
    rejected(bad, "counts|infeasible|budget")

    # the last entry of a committed class that filled its budget
    c = next(c for c in range(len(case.classes))
             if snap["class_placed"][c] > 0 and snap["log_len"][c] > 1)
    bad = _copy(snap)
    bad["log_len"][c] -= 1
    bad["log_counts"][int(snap["log_off"][c]) + int(snap["log_len"][c]) - 1] = 0
    rejected(bad, "not logged|counts|class_placed")

    committed = [j for j, (b, e) in enumerate(snap["jobs"])
                 if snap["job_flag"][j] == 1 and snap["job_placed"][j] > 0]
    multi = [j for j in committed
             if snap["jobs"][j][1] - snap["jobs"][j][0] > 1]
    bad = _copy(snap)
    bad["job_flag"][(multi or committed)[0]] = 0
    rejected(bad, "flag")
    failed_multi = [j for j, (b, e) in enumerate(snap["jobs"])
                    if e - b > 1 and snap["job_flag"][j] == 0]
    if failed_multi:
        bad = _copy(snap)
        bad["job_flag"][failed_multi[0]] = 1
        rejected(bad, "flag")

    bad = _copy(snap)
    node = int(snap["log_nodes"][e])
    bad["used"][node, 0] += 1.0
    rejected(bad, "final used")
    bad = _copy(snap)
    bad["queue_alloc"][0, 0] -= 1.0
    rejected(bad, "queue_alloc")


# --------------------------------------------------------------------------
# byte-scale inputs of the discard tests
# --------------------------------------------------------------------------

@pytest.mark.parametrize("N,R,seed", kc.BYTE_SELECT_SHAPES)
def test_byte_select_inputs_leave_a_residue(N, R, seed):
    """Precondition of tests/test_inexact_ops_gpu.py: on the nodes a
    discarded class touched, u + c*r - c*r is not u in f32 — whether the
    product rounds on its own or is folded into the adds."""
    inp = kc.byte_select_inputs(N, R, seed)
    for ntasks in kc.BYTE_SELECT_TASKS:
        nodes, counts, placed = kc.select_log(inp, ntasks)
        assert placed == min(ntasks, inp["room"]) and len(nodes) > 1
        unfused, fused = kc.select_residues(inp["used"], inp["req"], nodes,
                                            counts)
        print(N, R, ntasks, "residues:", unfused, fused, "of", len(nodes))
        assert unfused >= 1 and fused >= 1


def test_issue_example_of_a_residue():
    u, r, c = 112200000000.0, 1.5e9, 14
    two = kc.residue_f32(u, c, r, fused=False)
    one = kc.residue_f32(u, c, r, fused=True)
    assert float(two) - float(np.float32(u)) == 8192.0
    assert float(one) == float(np.float32(u))
    assert float(kc.ulp_f32(u)) == 8192.0


BYTES = kc.byte_plan_cases()


@functools.lru_cache(maxsize=None)
def _bytes(name):
    case = BYTES[name][0]()
    snap, records, _ = kc.run_oracle(case)
    return case, snap, records


@pytest.mark.parametrize("name", sorted(BYTES))
def test_byte_plan_case_discards_would_leave_residues(name):
    case, snap, records = _bytes(name)
    cond = kc.plan_conditions(case, snap, records)
    for key in BYTES[name][1]:
        assert cond[key], f"{name}: oracle run shows no {key}"
    drop = kc.discarded_single_jobs(case, snap)
    assert drop
    total = [0, 0]
    for j in drop:
        c = case.jobs[j][0]
        rec = records[c]
        off, n = int(snap["log_off"][c]), int(snap["log_len"][c])
        nodes = snap["log_nodes"][off:off + n]
        left, counts = min(rec["ntasks"], rec["quota"]), []
        for node in nodes:                # the discard zeroed the log's
            counts.append(min(int(rec["cap"][node]), left))
            left -= counts[-1]
        res = kc.select_residues(rec["used"],
                                 torch.from_numpy(case.classes[c]["req"]),
                                 nodes, np.array(counts))
        total = [a + b for a, b in zip(total, res)]
    print(name, "residues (unfused, fused):", total)
    assert total[0] >= 1 and total[1] >= 1


@pytest.mark.parametrize("name", sorted(BYTES))
def test_oracle_discard_leaves_no_trace(name):
    """run_plan_torch: the plan without its discarded single-class jobs
    ends in bit-equal usage and queue allocation."""
    case, snap, _ = _bytes(name)
    drop = set(kc.discarded_single_jobs(case, snap))
    pruned, _, _ = kc.run_oracle(kc.without_jobs(case, drop))
    kc.same_trace(snap, pruned, case, drop)
