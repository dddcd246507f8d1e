"""``vamd_spread_select`` and the spread routing of ``vamd_run_cycle``
against the oracle: logs entry for entry and in order, per-domain counts,
usage, queue allocation and the counters, bit for bit.

Inputs are exact in f32 (``_spread_cases``), scores take four values, so
tie groups are large.  Before any GPU comparison the oracle's own results
are checked for non-vacuity."""

import functools

import numpy as np
import pytest
import torch

import _spread_cases as sc

pytestmark = pytest.mark.gpu

DEV = "cuda"
NS = (1, 63, 64, 65, 1025, 2049)
DS = (1, 2, 3, 64, 65, "N")
RS = (1, 5, 64)
MODE_VARS = ("VAMD_MEGACYCLE", "VAMD_CHAIN_CHUNK", "VAMD_NO_CHAIN")


def shape_cases():
    """Every N x D (D clipped to N), both skews; R walks through RS."""
    out, seen = {}, set()
    for i, N in enumerate(NS):
        for j, D in enumerate(DS):
            d = N if D == "N" else min(D, N)
            if (N, d) in seen:
                continue
            seen.add((N, d))
            for skew in (1, 2):
                R = RS[(i + j + skew) % 3]
                name = f"N{N}-D{d}-s{skew}-R{R}"
                out[name] = functools.partial(
                    sc.random_case, name, N, d, skew, R,
                    seed=100 * i + 10 * j + skew,
                    unbalanced=(i + j) % 2 == 0)
    return out


def feature_cases():
    f = sc.random_case
    return {
        "dead-domain": functools.partial(f, "dead", 257, 3, 1, 5, 7,
                                         dead_domain=True, ntasks=60),
        "unbalanced": functools.partial(f, "unb", 300, 5, 1, 5, 8,
                                        unbalanced=True, ntasks=80),
        "quota": functools.partial(f, "quota", 300, 4, 2, 5, 9, quota=11,
                                   ntasks=50),
        "over-capacity": functools.partial(f, "over", 130, 3, 2, 1, 10,
                                           ntasks=4000, cap_hi=2),
        "over-capacity-host": functools.partial(f, "overh", 65, 65, 1, 5, 11,
                                                ntasks=500),
        "gang-revert": functools.partial(f, "rev", 200, 3, 1, 5, 12,
                                         dead_domain=True, ntasks=40,
                                         fuse_min=40),
        "gang-revert-host": functools.partial(f, "revh", 1025, 1025, 1, 64,
                                              13, ntasks=30, fuse_min=2000),
        "gang-kept": functools.partial(f, "kept", 200, 3, 2, 5, 14,
                                       ntasks=20, fuse_min=1),
        "no-unlabeled-all-tie": functools.partial(
            f, "tie", 2049, 64, 1, 1, 15, unlabeled=0.0, infeasible=0.0,
            ntasks=96),
    }


SHAPES = shape_cases()
FEATURES = feature_cases()
R_SWEEP = {f"R{R}-s{s}": functools.partial(sc.random_case, f"R{R}s{s}", 129,
                                           3, s, R, 40 + R + s)
           for R in RS for s in (1, 2)}
ALL = {**SHAPES, **FEATURES, **R_SWEEP}


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Case + oracle result: computed once, never modified."""
    case = ALL[name]()
    return case, sc.run_oracle(case)


@pytest.fixture(scope="module", autouse=True)
def _library_and_non_vacuity():
    from volcano_amd.ops import hip
    hip._load()
    seen = dict(placed=0, blocked=0, tie=0, stopped=0, reverted=0,
                multi_count=0, unlabeled=0, quota=0)
    for name in ALL:
        case, want = oracle(name)
        seq, _, steps = sc.model_of(case)
        seen["placed"] += bool(seq)
        seen["blocked"] += any(b for n, b, _ in steps if n is not None)
        seen["tie"] += any(t >= 3 for _, _, t in steps)
        seen["stopped"] += steps[-1][0] is None and steps[-1][1]
        seen["reverted"] += want["reverted"] and want["before"]["placed"] > 0
        seen["multi_count"] += bool((want["before"]["log_counts"] > 1).any())
        seen["unlabeled"] += bool(((case.dom_of < 0)
                                   & (case.score > sc.NEG_INF)
                                   & (case.cap > 0)).any())
        seen["quota"] += sc.quota_of(case) < case.ntasks and \
            len(seq) == sc.quota_of(case)
    assert all(v >= 1 for v in seen.values()), seen
    assert seen["blocked"] >= 10 and seen["tie"] >= 10, seen


def run_hip(case):
    from volcano_amd.ops import hip
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    score, cap, req = d(case.score.copy()), d(case.cap.copy()), d(case.req)
    used_t = d(case.used.T.copy())
    qa, ql = d(case.queue_alloc.copy()), d(case.queue_limit)
    ln = torch.zeros(case.K, dtype=torch.int32, device=DEV)
    lc = torch.zeros(case.K, dtype=torch.int32, device=DEV)
    ll = torch.zeros(1, dtype=torch.int32, device=DEV)
    placed = torch.zeros(1, dtype=torch.int32, device=DEV)
    jp = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    dom_of, cnt = d(case.dom_of), d(case.dom_count.copy())
    hip.spread_select(score, cap, req, case.ntasks, used_t, qa, ql, ln, lc,
                      ll, placed, jp, dom_of, cnt, case.max_skew,
                      case.fuse_min)
    torch.cuda.synchronize()
    return dict(log_nodes=ln.cpu().numpy(), log_counts=lc.cpu().numpy(),
                log_len=int(ll), placed=int(placed), job_placed=int(jp),
                used=used_t.t().cpu().numpy(), queue_alloc=qa.cpu().numpy(),
                dom_count=cnt.cpu().numpy())


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int32),
                          np.ascontiguousarray(b).view(np.int32))


def compare(want, got):
    n = want["log_len"]
    assert got["log_len"] == n
    assert got["log_nodes"][:n].tolist() == want["log_nodes"][:n].tolist()
    assert got["log_counts"][:n].tolist() == want["log_counts"][:n].tolist()
    assert got["placed"] == want["placed"]
    assert got["job_placed"] == want["job_placed"]
    assert got["dom_count"].tolist() == want["dom_count"].tolist()
    assert same_bits(got["used"], want["used"]), "used differs"
    assert same_bits(got["queue_alloc"], want["queue_alloc"]), \
        "queue_alloc differs"


@pytest.mark.parametrize("name", list(SHAPES))
def test_shapes(name):
    case, want = oracle(name)
    compare(want, run_hip(case))


@pytest.mark.parametrize("name", list(R_SWEEP))
def test_resource_dims(name):
    case, want = oracle(name)
    compare(want, run_hip(case))


@pytest.mark.parametrize("name", list(FEATURES))
def test_features(name):
    case, want = oracle(name)
    if name.startswith("gang-revert"):
        assert want["reverted"] and want["before"]["placed"] > 0
        assert want["dom_count"].tolist() == case.dom_count.tolist()
    if name == "gang-kept":
        assert not want["reverted"] and want["placed"] > 0
    if name == "dead-domain":
        assert want["placed"] < case.ntasks        # stopped by the skew
    if name.startswith("over-capacity"):
        assert 0 < want["placed"] < case.ntasks
    if name == "quota":
        assert want["placed"] == sc.quota_of(case) < case.ntasks
    compare(want, run_hip(case))


def test_spread_revert_kernel():
    """vamd_spread_revert: flag 0 undoes a kept placement, flag 1 does not."""
    from volcano_amd.ops import hip
    case, _ = oracle("unbalanced")
    kept = sc.run_oracle(case, revert=False)
    undone = sc.run_oracle(case, revert=True)
    assert kept["placed"] > 0
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    for flag, want in ((1, kept), (0, undone)):
        used_t = d(kept["used"].T.copy())
        qa, cnt = d(kept["queue_alloc"].copy()), d(kept["dom_count"].copy())
        ln, lc = d(kept["log_nodes"].copy()), d(kept["log_counts"].copy())
        ll = torch.tensor([kept["log_len"]], dtype=torch.int32, device=DEV)
        placed = torch.tensor([kept["placed"]], dtype=torch.int32,
                              device=DEV)
        jp = torch.tensor([kept["job_placed"]], dtype=torch.int32,
                          device=DEV)
        hip.spread_revert(torch.tensor([flag], dtype=torch.uint8, device=DEV),
                          ln, lc, ll, d(case.req), used_t, qa, placed, jp,
                          d(case.dom_of), cnt)
        torch.cuda.synchronize()
        compare(want, dict(
            log_nodes=ln.cpu().numpy(), log_counts=lc.cpu().numpy(),
            log_len=int(ll), placed=int(placed), job_placed=int(jp),
            used=used_t.t().cpu().numpy(), queue_alloc=qa.cpu().numpy(),
            dom_count=cnt.cpu().numpy()))


# --------------------------------------------------------------------------
# run_plan_hip vs run_plan_torch on plans with spread classes
# --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def plan_oracle(bulk):
    case = sc.spread_plan_case(bulk=bulk)
    snap, records = sc.run_plan_oracle(case)
    return case, snap, records


def plan_non_vacuous(bulk, oracle=plan_oracle):
    case, snap, records = oracle(bulk)
    r = case.roles
    assert len(records) == len(case.spread)
    assert any(rec["placed"] > 0 for rec in records), "no spread placements"
    assert any(b for rec in records for n, b, _ in rec["steps"]
               if n is not None), "no instance blocked by skew"
    assert any(t >= 3 for rec in records for _, _, t in rec["steps"]), \
        "no tie broken"
    # the two-role gang reverted after its spread role had placed
    j = int(np.searchsorted([b for b, _ in snap["jobs"]],
                            r["gang_spread"]))
    assert snap["jobs"][j] == (r["gang_spread"], r["gang_spread"] + 2)
    assert snap["job_flag"][j] == 0
    assert snap["log_len"][r["gang_spread"]] > 0
    assert snap["class_placed"][r["gang_spread"]] == 0
    # ... and the later class of the same group started from the restored
    # counts
    later = [rec for rec in records if rec["skew"] == 2][0]
    assert later["count"] == case.groups[0][1].tolist()
    assert snap["class_placed"][r["spread"]] > 0
    assert snap["class_placed"][r["host_revert"]] == 0
    assert snap["log_len"][r["host_revert"]] > 0
    assert snap["class_placed"][r["host"]] > 0
    if bulk:
        assert case.base.classes[r["bulk"]]["ntasks"] >= 512
        assert case.base.N >= 512
        assert snap["class_placed"][r["bulk"]] >= 512
        # a bulk-sized spread class, placed one per node (D = N, skew 1)
        assert case.base.classes[r["host"]]["ntasks"] >= 512
        assert snap["log_len"][r["host"]] == \
            snap["class_placed"][r["host"]] >= 512
    plain =[c for c in range(len(case.base.classes))
             if c not in case.spread]
    assert sum(snap["class_placed"][c] > 0 for c in plain) >= 20
    return case, snap


def run_plan(case):
    from volcano_amd.scheduler.plan import run_plan_hip
    plan = sc.build_spread_plan(case, DEV)
    res = run_plan_hip(plan)
    torch.cuda.synchronize()
    return sc.spread_snapshot(plan, res)


def set_mode(monkeypatch, **env):
    for var in MODE_VARS:
        monkeypatch.delenv(var, raising=False)
    for var, val in env.items():
        monkeypatch.setenv(var, str(val))


@pytest.mark.parametrize("mode", [{}, {"VAMD_MEGACYCLE": 1},
                                  {"VAMD_CHAIN_CHUNK": 4}],
                         ids=["default", "megacycle", "chain4"])
def test_plan_with_spread_classes(monkeypatch, mode):
    """Bulk class + reverting gang with a spread role + chain run + spread
    jobs of two groups, under every dispatch mode."""
    case, want = plan_non_vacuous(True)
    set_mode(monkeypatch, **mode)
    sc.compare_spread(want, run_plan(case))


def test_megacycle_yields_to_spread(monkeypatch):
    """No bulk class, >= 32 small classes: VAMD_MEGACYCLE=1 would take the
    one-launch kernel, which has no spread select — the plan must run per
    class instead."""
    case, want = plan_non_vacuous(False)
    assert len(case.base.classes) >= 32
    assert max(c["ntasks"] for c in case.base.classes) < 512
    set_mode(monkeypatch, VAMD_MEGACYCLE=1)
    sc.compare_spread(want, run_plan(case))
