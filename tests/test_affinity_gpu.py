"""``domain_mask`` → ``select_commit`` → ``domain_count_add`` and the routing
of ``vamd_run_cycle`` by its ``class_mode`` column against the oracle: logs
entry for entry and in order, per-domain counts, usage, queue allocation
and the counters, bit for bit.  Inputs are exact in f32
(``_affinity_cases``)."""

import functools

import numpy as np
import pytest
import torch

import _affinity_cases as ac

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODE_VARS = ("VAMD_MEGACYCLE", "VAMD_CHAIN_CHUNK", "VAMD_NO_CHAIN")
ALL = {**{f"aff-{k}": v for k, v in ac.AFFINITY_CASES.items()},
       **{f"anti-{k}": v for k, v in ac.ANTI_CASES.items()}}


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Case + oracle result: computed once, never modified."""
    case = ALL[name]()
    return case, ac.run_oracle(case)


@pytest.fixture(scope="module", autouse=True)
def _library():
    from volcano_amd.ops import hip
    hip._load()


def _d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run_hip(case, *, bulk_scratch=True):
    """The composition the cycle runner launches for such a class."""
    from volcano_amd.ops import hip
    score, cap, req = _d(case.score.copy()), _d(case.cap.copy()), _d(case.req)
    used_t = _d(case.used.T.copy())
    qa, ql = _d(case.queue_alloc.copy()), _d(case.queue_limit)
    ln = torch.zeros(case.K, dtype=torch.int32, device=DEV)
    lc = torch.zeros(case.K, dtype=torch.int32, device=DEV)
    ll = torch.zeros(1, dtype=torch.int32, device=DEV)
    placed = torch.zeros(1, dtype=torch.int32, device=DEV)
    jp = torch.full((1,), 7, dtype=torch.int32, device=DEV)
    dom_of, cnt = _d(case.dom_of), _d(case.dom_count.copy())
    sort_scratch = torch.empty(4 * case.N, dtype=torch.int32, device=DEV) \
        if bulk_scratch else None
    hip.domain_mask(score, cap, dom_of, cnt, case.mode)
    masked = (score.cpu().numpy().copy(), cap.cpu().numpy().copy())
    hip.select_commit(score, cap, req, case.ntasks, used_t, qa, ql, ln, lc,
                      ll, placed, jp, case.fuse_min, sort_scratch)
    hip.domain_count_add(ln, lc, ll, dom_of, cnt)
    torch.cuda.synchronize()
    return dict(log_nodes=ln.cpu().numpy(), log_counts=lc.cpu().numpy(),
                log_len=int(ll), placed=int(placed), job_placed=int(jp),
                used=used_t.t().cpu().numpy(), queue_alloc=qa.cpu().numpy(),
                dom_count=cnt.cpu().numpy(), masked=masked)


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


def check_mask(case, masked):
    """Kept nodes are placeable and labelled; masked ones carry -inf AND
    cap 0 (the serial select would otherwise log empty entries)."""
    score, cap = masked
    kept = score > ac.NEG_INF
    assert ((cap > 0) == kept).all()
    assert (case.dom_of[kept] >= 0).all()
    assert (case.cap[kept] > 0).all() and \
        (case.score[kept] > ac.NEG_INF).all()
    assert same_bits(score[kept], case.score[kept])
    if case.mode == ac.ANTI:
        assert (cap[kept] == 1).all()
        doms = case.dom_of[kept]
        assert len(set(doms.tolist())) == len(doms)
        assert (case.dom_count[doms] == 0).all()
    else:
        assert (cap[kept] == case.cap[kept]).all()


@pytest.mark.parametrize("name", list(ALL))
def test_composition_equals_oracle(name):
    case, want = oracle(name)
    got = run_hip(case)
    check_mask(case, got["masked"])
    compare(want, got)


@pytest.mark.parametrize("name", ["aff-bulk-hosting", "anti-bulk-identity",
                                  "aff-two-of-three"])
def test_serial_select_gives_the_same(name):
    """Without sort scratch every size takes the serial select."""
    case, want = oracle(name)
    compare(want, run_hip(case, bulk_scratch=False))


def test_bulk_cases_take_the_bulk_select():
    for name in ("aff-bulk-empty", "aff-bulk-hosting", "anti-bulk",
                 "anti-bulk-identity"):
        case, _ = oracle(name)
        assert case.ntasks >= 512 and case.N >= 512


def test_argument_checks():
    from volcano_amd.ops import hip
    case, _ = oracle("aff-anchor-best")
    score, cap = _d(case.score.copy()), _d(case.cap.copy())
    dom_of, cnt = _d(case.dom_of), _d(case.dom_count.copy())
    with pytest.raises(ValueError):
        hip.domain_mask(score, cap, dom_of, cnt, 0)
    with pytest.raises(ValueError):
        hip.domain_mask(score, cap, dom_of[:-1], cnt, 1)
    with pytest.raises(ValueError):
        hip.domain_mask(score, cap, dom_of,
                        torch.zeros(case.N + 1, dtype=torch.int32,
                                    device=DEV), 1)
    with pytest.raises(ValueError):
        hip.domain_mask(score, cap, dom_of, cnt, 2,
                        scratch=torch.zeros(2, dtype=torch.int32,
                                            device=DEV))
    ln = torch.zeros(4, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError):
        hip.domain_count_add(ln, ln[:3], ln[:1], dom_of, cnt)


def test_two_class_job_reverts_through_spread_revert():
    """A kept affinity placement of a two-class job, then the job's flag:
    0 undoes it (counts included), 1 does not."""
    from volcano_amd.ops import hip
    case, _ = oracle("aff-two-of-three")
    kept = ac.run_oracle(case, revert=False)
    undone = ac.run_oracle(case, revert=True)
    assert kept["placed"] > 0
    assert kept["dom_count"].tolist() != case.dom_count.tolist()
    assert undone["dom_count"].tolist() == case.dom_count.tolist()
    first = run_hip(case)
    compare(kept, first)
    for flag, want in ((1, kept), (0, undone)):
        used_t = _d(first["used"].T.copy())
        qa, cnt = _d(first["queue_alloc"].copy()), \
            _d(first["dom_count"].copy())
        ln, lc = _d(first["log_nodes"].copy()), _d(first["log_counts"].copy())
        ll = torch.tensor([first["log_len"]], dtype=torch.int32, device=DEV)
        placed = torch.tensor([first["placed"]], dtype=torch.int32,
                              device=DEV)
        jp = torch.tensor([first["job_placed"]], dtype=torch.int32,
                          device=DEV)
        hip.spread_revert(torch.tensor([flag], dtype=torch.uint8, device=DEV),
                          ln, lc, ll, _d(case.req), used_t, qa, placed, jp,
                          _d(case.dom_of), cnt)
        torch.cuda.synchronize()
        compare(want, dict(
            log_nodes=ln.cpu().numpy(), log_counts=lc.cpu().numpy(),
            log_len=int(ll), placed=int(placed), job_placed=int(jp),
            used=used_t.t().cpu().numpy(), queue_alloc=qa.cpu().numpy(),
            dom_count=cnt.cpu().numpy()))


# --------------------------------------------------------------------------
# run_plan_hip vs run_plan_torch on plans with affinity classes
# --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def plan_oracle(N, rules=True):
    case = ac.affinity_plan_case(N=N)
    snap, records = ac.run_plan_oracle(case, rules=rules)
    return case, snap, records


def run_plan(case, *, rules=True, calls=None):
    from volcano_amd.ops import hip
    from volcano_amd.scheduler.plan import run_plan_hip
    plan = ac.build_affinity_plan(case, DEV, rules=rules)
    real = hip.run_cycle

    def spy(*args, spread=None, **kw):
        if calls is not None:
            calls.append(spread)
        return real(*args, spread=spread, **kw)

    hip.run_cycle = spy
    try:
        res = run_plan_hip(plan)
    finally:
        hip.run_cycle = real
    torch.cuda.synchronize()
    return ac.plan_snapshot(plan, res)


def set_mode(monkeypatch, **env):
    for var in MODE_VARS:
        monkeypatch.delenv(var, raising=False)
    for var, val in env.items():
        monkeypatch.setenv(var, str(val))


@pytest.mark.parametrize("N", [65, 1500])
@pytest.mark.parametrize("mode", [{}, {"VAMD_MEGACYCLE": 1},
                                  {"VAMD_CHAIN_CHUNK": 4}],
                         ids=["default", "megacycle", "chain4"])
def test_plan_with_affinity_classes(monkeypatch, mode, N):
    """Affinity, anti-affinity, spread and plain classes of shared groups,
    in-select and multi-class reverts, a chain run, under every dispatch
    mode: the domain classes still run per class, with identical results."""
    case, want, records = plan_oracle(N)
    assert any(r["placed"] > 0 and r["mode"] == ac.AFFINITY for r in records)
    assert any(r["placed"] > 0 and r["mode"] == ac.ANTI for r in records)
    assert (want["job_flag"] == 0).any()
    assert len(case.base.classes) >= 32
    set_mode(monkeypatch, **mode)
    calls = []
    got = run_plan(case, calls=calls)
    ac.compare_plans(want, got)
    # one runner call for the whole plan, with one mode entry per class
    # (the launches themselves: test_launch_sequence_is_constant_in_ntasks)
    assert len(calls) == 1
    cm = calls[0]["class_mode"]
    assert cm.shape == (len(case.base.classes),)
    for c, (_, m) in case.affinity.items():
        assert cm[c] == m
    for c in case.spread:
        assert cm[c] == 0 and calls[0]["class_group"][c] >= 0


def _vamd_launches(case):
    """Names of the library's kernels one run_plan_hip launches, in start
    order (kernel trace of the torch profiler)."""
    from torch.profiler import ProfilerActivity, profile
    from volcano_amd.scheduler.plan import run_plan_hip
    plan = ac.build_affinity_plan(case, DEV)
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        res = run_plan_hip(plan)
        torch.cuda.synchronize()
    evs = [e for e in prof.events() if e.name.startswith("vamd::")]
    evs.sort(key=lambda e: e.time_range.start)
    names = [e.name.split("(")[0].replace("vamd::", "") for e in evs]
    return names, ac.plan_snapshot(plan, res)


@pytest.mark.parametrize("N", [65, 1500])
def test_launch_sequence_is_constant_in_ntasks(N):
    """Every affinity / anti class is score_cap -> domain_mask -> ONE select
    -> domain_count_add, whether it has 2 instances or 700: the same plan
    is traced with all such classes small and with all of them large."""
    import copy
    base = ac.affinity_plan_case(N=N)
    selects = ("select_commit_kernel", "bulk_select_kernel")
    traces = {}
    for ntasks in (2, 700):
        case = copy.deepcopy(base)
        for c in case.affinity:
            case.base.classes[c]["ntasks"] = ntasks
        want, _ = ac.run_plan_oracle(case)
        names, got = _vamd_launches(case)
        ac.compare_plans(want, got)
        masks = [i for i, n in enumerate(names) if n == "domain_mask_kernel"]
        assert len(masks) == len(case.affinity)
        assert names.count("domain_count_add_kernel") == len(case.affinity)
        for i in masks:
            assert names[i - 1] == "score_cap_kernel"
            assert names[i + 1] in selects
            assert names[i + 2] == "domain_count_add_kernel"
        bulk = ntasks >= 512 and N >= 512
        assert all((names[i + 1] == "bulk_select_kernel") == bulk
                   for i in masks)
        traces[ntasks] = [n if n not in selects else "select" for n in names]
    assert traces[2] == traces[700]


@pytest.mark.parametrize("N", [65, 1500])
def test_plan_without_domain_classes_takes_the_old_entry_point(N):
    case, want, _ = plan_oracle(N, rules=False)
    calls = []
    got = run_plan(case, rules=False, calls=calls)
    assert calls == [None]                  # no domain block at all
    ac.compare_plans(want, got)


def test_spread_only_plan_keeps_its_entry_point():
    import _spread_cases as sc
    from volcano_amd.ops import hip
    from volcano_amd.scheduler.plan import run_plan_hip
    case = sc.spread_plan_case(N=300, bulk=False)
    want, _ = sc.run_plan_oracle(case)
    plan = sc.build_spread_plan(case, DEV)
    calls, real = [], hip.run_cycle

    def spy(*args, spread=None, **kw):
        calls.append(spread)
        return real(*args, spread=spread, **kw)

    hip.run_cycle = spy
    try:
        res = run_plan_hip(plan)
    finally:
        hip.run_cycle = real
    torch.cuda.synchronize()
    assert len(calls) == 1 and "class_mode" not in calls[0]
    sc.compare_spread(want, sc.spread_snapshot(plan, res))


# --------------------------------------------------------------------------
# through the scheduler, HIP decision plane
# --------------------------------------------------------------------------

def _schedule(device):
    """Zone affinity (6), keyed anti-affinity (5) and zone affinity with
    hostname anti-affinity (5) in one cycle -> {pod: node}, zones."""
    from volcano_amd.scheduler import (FakeBinder, Scheduler, SchedulerCache,
                                       default_config)
    from volcano_amd.scheduler.config import PluginOption, Tier
    from volcano_amd.store import ObjectStore
    from volcano_amd.utils import synth
    GI = 1024 ** 3
    store, binder = ObjectStore(), FakeBinder()
    config = default_config()
    if device == "cuda":
        config.use_hip = True
        config.device = "cuda"
    config.tiers = [
        Tier(plugins=[PluginOption(n)
                      for n in ("priority", "gang", "conformance")]),
        Tier(plugins=[PluginOption(n) for n in (
            "overcommit", "drf", "predicates", "nodeorder", "binpack")]
            + [PluginOption("interpodaffinity",
                            arguments={"exact": True})])]
    cache = SchedulerCache(store=store, binder=binder, device=device)
    sched = Scheduler(cache, config)
    zones = {}
    for i in range(12):
        zones[f"n{i:02d}"] = "abc"[i % 3]
        store.create("Node", synth.make_node(
            f"n{i:02d}", cpu_milli=1000, mem=256 * GI,
            labels={"zone": zones[f"n{i:02d}"]}))
    store.create("Queue", synth.make_queue("default"))

    def job(name, n, affinity, priority):
        store.create("PodGroup", synth.make_podgroup(name, min_member=1))
        for i in range(n):
            p = synth.make_pod(f"{name}-w-{i}", name, cpu_milli=300, mem=GI,
                               role="w", priority=priority)
            p.affinity = affinity
            store.create("Pod", p)

    job("aff", 6, {"podAffinity": {"group": "g1", "topologyKey": "zone"}}, 9)
    job("anti", 5, {"podAntiAffinity": {"group": "g2",
                                        "topologyKey": "zone"}}, 5)
    job("both", 5, {"podAffinity": {"group": "g3", "topologyKey": "zone"},
                    "podAntiAffinity": {"group": "g3h"}}, 1)
    sched.run_once()
    return dict(binder.binds), zones


def test_scheduler_on_the_hip_plane_matches_the_torch_runner():
    want, zones = _schedule("cpu")
    got, _ = _schedule("cuda")
    assert got == want
    zone_of = lambda prefix: [zones[n] for k, n in sorted(got.items())
                              if k.startswith(f"default/{prefix}-")]
    assert len(zone_of("aff")) == 6 and len(set(zone_of("aff"))) == 1
    assert sorted(zone_of("anti")) == ["a", "b", "c"]
    both = zone_of("both")
    assert len(both) == 4 and len(set(both)) == 1     # one per node of a zone
