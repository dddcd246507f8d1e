"""The domain-rule selects (``spread_select``, ``domain_mask`` ->
``select_commit`` -> ``domain_count_add``) against the sequential oracles on
signed, denormal and near-tied scores, against the plain select where the
rule cannot bind, and behind ``score_cap_kernel`` on inexact scores that
straddle zero.  Bit for bit everywhere: no tolerance, no allowance.

The cases are those of ``_domain_score_cases``; ``test_domain_scores.py``
shows on the CPU that they catch every wrong variant of the integer key."""

import contextlib
import functools

import numpy as np
import pytest
import torch

import _affinity_cases as ac
import _domain_score_cases as dc
import _kernel_cases as kc
import _spread_cases as sc
import test_affinity_gpu as tag
import test_spread_gpu as tsg

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODES = {"default": {}, "megacycle": {"VAMD_MEGACYCLE": 1},
         "chain4": {"VAMD_CHAIN_CHUNK": 4}}


@pytest.fixture(scope="module", autouse=True)
def _library():
    from volcano_amd.ops import hip
    hip._load()


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32),
                          np.ascontiguousarray(b).view(np.int32))


def run_rule(case, **kw):
    if dc.rule_of(case) == dc.SPREAD:
        return tsg.run_hip(case)
    got = tag.run_hip(case, **kw)
    tag.check_mask(case, got["masked"])
    if case.mode == dc.ANTI:
        check_heads(case, got["masked"])
    return got


def check_heads(case, masked):
    """The kept nodes are exactly the open domains' heads: per domain the
    placeable node with the largest key."""
    key = dc.spread_key(case.score)
    dom = case.dom_of
    ok = (case.score > dc.NEG_INF) & (case.cap > 0) & (dom >= 0)
    ok &= case.dom_count[np.where(dom >= 0, dom, 0)] == 0
    heads = {}
    for n in np.flatnonzero(ok):
        if dom[n] not in heads or key[n] > key[heads[dom[n]]]:
            heads[dom[n]] = n
    kept = np.flatnonzero(masked[0] > dc.NEG_INF)
    assert kept.tolist() == sorted(heads.values())


def run_select(case, cap):
    """The serial ``select_commit`` kernel on the case's score and ``cap``
    in the form score_cap leaves them: cap 0 where the score is -inf and
    score -inf where cap is 0 (the serial kernel logs an empty entry for a
    finite score without capacity; the domain kernels mask such nodes)."""
    from volcano_amd.ops import hip
    cap = np.where(case.score > dc.NEG_INF, cap, 0).astype(np.int32)
    score = np.where(cap > 0, case.score, np.float32(dc.NEG_INF))
    used_t = _d(case.used.T.copy())
    qa = _d(case.queue_alloc.copy())
    ln = torch.zeros(case.K, dtype=torch.int32, device=DEV)
    lc = torch.zeros(case.K, dtype=torch.int32, device=DEV)
    ll = torch.zeros(1, dtype=torch.int32, device=DEV)
    placed = torch.zeros(1, dtype=torch.int32, device=DEV)
    jp = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    hip.select_commit(_d(score), _d(cap), _d(case.req),
                      case.ntasks, used_t, qa, _d(case.queue_limit), ln, lc,
                      ll, placed, jp, -1, None)
    torch.cuda.synchronize()
    return dict(log_nodes=ln.cpu().numpy(), log_counts=lc.cpu().numpy(),
                log_len=int(ll), placed=int(placed), job_placed=int(jp),
                used=used_t.t().cpu().numpy(), queue_alloc=qa.cpu().numpy())


def same_fill(want, got):
    """``compare`` without the domain counts (the plain select has none)."""
    n = want["log_len"]
    assert got["log_len"] == n
    assert got["log_nodes"][:n].tolist() == want["log_nodes"][:n].tolist()
    assert got["log_counts"][:n].tolist() == want["log_counts"][:n].tolist()
    assert got["placed"] == want["placed"]
    assert got["job_placed"] == want["job_placed"]
    assert same_bits(got["used"], want["used"]), "used differs"
    assert same_bits(got["queue_alloc"], want["queue_alloc"]), \
        "queue_alloc differs"


# --------------------------------------------------------------------------
# section 3: kernels against the oracles
# --------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(dc.SPREAD_CASES))
def test_spread(name):
    case, want = dc.oracle(name)
    got = run_rule(case)
    tsg.compare(want, got)
    if name.endswith("gang-revert"):
        assert want["reverted"] and want["before"]["placed"] > 0
        assert got["dom_count"].tolist() == case.dom_count.tolist()
        assert same_bits(got["used"], case.used)
        assert same_bits(got["queue_alloc"], case.queue_alloc)
        assert not got["log_counts"].any()


@pytest.mark.parametrize("name", list(dc.AFFINITY_CASES))
def test_affinity_and_anti(name):
    """Anti-affinity runs twice, with sort scratch (600 instances: the
    sort-based select when N >= 512) and without (serial): both equal the
    oracle and each other."""
    case, want = dc.oracle(name)
    got = run_rule(case)
    tag.compare(want, got)
    if case.mode == dc.ANTI:
        serial = run_rule(case, bulk_scratch=False)
        tag.compare(want, serial)
        tag.compare(serial, got)
        assert same_bits(serial["masked"][0], got["masked"][0])


@pytest.mark.parametrize("name", [n for n in dc.RELATION_CASES
                                  if not n.endswith("N257")])
def test_rule_that_cannot_bind_is_the_plain_select_kernel(name):
    """Kernel against kernel: unbounded skew, one domain per node with unit
    caps, one hosting domain."""
    case, want = dc.oracle(name)
    got = run_rule(case, bulk_scratch=False) \
        if dc.rule_of(case) != dc.SPREAD else run_rule(case)
    cap = np.minimum(case.cap, 1) if name.startswith("anti") else case.cap
    plain = run_select(case, cap)
    same_fill(plain, got)
    same_fill(got, plain)
    (tsg if dc.rule_of(case) == dc.SPREAD else tag).compare(want, got)


# --------------------------------------------------------------------------
# section 4: behind the score kernel
# --------------------------------------------------------------------------

def kernel_score_cap(st, *, w_least, w_most, w_bal, bias, req=None,
                     tolerated=0, require=None, forbid=None):
    from volcano_amd.ops import hip
    N, R = st["alloc"].shape
    zw = torch.zeros(st["planes"].shape[1], dtype=torch.int64)
    score = torch.empty(N, device=DEV)
    cap = torch.empty(N, dtype=torch.int32, device=DEV)
    t = lambda x: x.t().contiguous().to(DEV)
    hip.score_cap(t(st["alloc"]), t(st["used"]), t(st["extra"]),
                  st["ready"].to(torch.uint8).to(DEV), st["taints"].to(DEV),
                  t(st["planes"]),
                  (st["req"] if req is None else req).to(DEV), tolerated,
                  (zw if require is None else require).to(DEV),
                  (zw if forbid is None else forbid).to(DEV),
                  w_least, w_most, w_bal, st["dim_w"].to(DEV),
                  None if bias is None else bias.to(DEV), score, cap)
    torch.cuda.synchronize()
    return score.cpu().numpy(), cap.cpu().numpy()


@functools.lru_cache(maxsize=None)
def kernel_scores(name):
    """score_cap_kernel on a state of section 4, read back: once per
    state."""
    st, kw = dc.scored_state(name)
    score, cap = kernel_score_cap(st, **kw)
    want, want_cap = kc.oracle_score_cap(st, **kw)
    # what the select sees: the same feasible set as the oracle's, scores
    # on both sides of zero
    feas = score > dc.NEG_INF
    assert np.array_equal(feas, want.numpy() > dc.NEG_INF)
    assert np.array_equal(cap, want_cap.numpy())
    neg = float((score[feas] < 0).mean())
    assert 0.2 <= neg <= 0.8, neg
    return score, cap


SCORED = [(name, D) for name, v in dc.SCORED_STATES.items()
          for N, D in dc.SCORED_SHAPES if N == v[0]]


@pytest.mark.parametrize("name,D", SCORED,
                         ids=[f"{n}-D{D}" for n, D in SCORED])
def test_rules_on_the_score_kernels_output(name, D):
    """score_cap_kernel -> read back -> the rule's kernels on those bits
    against the rule's oracle on the same bits.  The oracle never sees a
    score of its own, so how the two score implementations round cannot
    matter."""
    score, cap = kernel_scores(name)
    for skew in (1, 2):
        case = dc.scored_case(name, score, cap, dc.SPREAD, D, skew)
        want = sc.run_oracle(case)
        assert want["placed"] > 0
        tsg.compare(want, run_rule(case))
    for rule in ("aff-empty", "aff-hosting", "anti"):
        case = dc.scored_case(name, score, cap, rule, D)
        want = ac.run_oracle(case)
        assert want["placed"] > 0
        tag.compare(want, run_rule(case))


# --------------------------------------------------------------------------
# whole plans: every select of the oracle is the sequential reference, only
# the score comes from the kernel
# --------------------------------------------------------------------------

@contextlib.contextmanager
def scores_from_the_kernel():
    from volcano_amd.scheduler import plan as planmod
    real = planmod.ref.score_cap

    def score_cap(alloc, used, extra, ready, taints, planes, req, tolerated,
                  require, forbid, w_least, w_most, w_bal, dim_w, bias,
                  score_out, cap_out):
        st = dict(alloc=alloc, used=used, extra=extra, ready=ready,
                  taints=taints, planes=planes, dim_w=dim_w)
        score, cap = kernel_score_cap(
            st, w_least=w_least, w_most=w_most, w_bal=w_bal, bias=bias,
            req=req, tolerated=tolerated, require=require, forbid=forbid)
        score_out.copy_(torch.from_numpy(score))
        cap_out.copy_(torch.from_numpy(cap))

    planmod.ref.score_cap = score_cap
    try:
        yield
    finally:
        planmod.ref.score_cap = real


def run_modes(monkeypatch, run):
    out = {}
    for mode, env in MODES.items():
        tsg.set_mode(monkeypatch, **env)
        out[mode] = run()
    return out


def test_spread_twin_plan(monkeypatch):
    case = dc.spread_twin()
    with scores_from_the_kernel():
        want, records = sc.run_plan_oracle(case)
    r = case.roles
    assert any(rec["placed"] > 0 for rec in records)
    assert any(b for rec in records for n, b, _ in rec["steps"]
               if n is not None), "no instance blocked by skew"
    assert want["class_placed"][r["host_revert"]] == 0
    assert want["log_len"][r["host_revert"]] > 0
    j = [b for b, _ in want["jobs"]].index(r["gang_spread"])
    assert want["jobs"][j] == (r["gang_spread"], r["gang_spread"] + 2)
    assert want["job_flag"][j] == 0
    got = run_modes(monkeypatch, lambda: tsg.run_plan(case))
    for mode, snap in got.items():
        sc.compare_spread(want, snap)
    sc.compare_spread(got["default"], got["megacycle"])
    sc.compare_spread(got["default"], got["chain4"])
    sc.compare_spread(got["megacycle"], got["chain4"])


@pytest.mark.parametrize("N", list(dc.AFFINITY_TWINS))
def test_affinity_twin_plan(monkeypatch, N):
    case = dc.affinity_twin(N)
    with scores_from_the_kernel():
        want, records = ac.run_plan_oracle(case)
    dc.affinity_plan_conditions(case, want, records, exact=False)
    got = run_modes(monkeypatch, lambda: tag.run_plan(case))
    for mode, snap in got.items():
        ac.compare_plans(want, snap)
    ac.compare_plans(got["default"], got["megacycle"])
    ac.compare_plans(got["default"], got["chain4"])
    ac.compare_plans(got["megacycle"], got["chain4"])
