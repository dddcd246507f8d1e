"""The cases of ``test_predicate_compile`` on the device: ``score_cap`` over
a session's device planes with the rows the real compiler built, and whole
cycles on the HIP decision plane under every dispatch mode.  Each test
synchronizes once and compares on the host."""

import functools

import pytest
import torch

import _predicate_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODE_VARS = ("VAMD_MEGACYCLE", "VAMD_CHAIN_CHUNK", "VAMD_NO_CHAIN")


@pytest.fixture(scope="module", autouse=True)
def _library():
    from volcano_amd.ops import hip
    hip._load()


@functools.lru_cache(maxsize=None)
def world(name):
    if name == "hostnames":
        return pc.hostname_world()
    return pc.WORLDS[name]()


def device_masks(nt, classes):
    """One score_cap launch per class into its own row, one sync."""
    from volcano_amd.ops import hip
    N, R, W = nt.n, nt.r, nt.planes_t.shape[0]
    assert nt.alloc_t.shape == nt.used_t.shape == (R, N)
    assert nt.planes_t.shape == (W, N) and nt.planes_t.is_contiguous()
    assert nt.ready.shape == nt.taint_mask.shape == (N,)
    assert nt.planes_t.device.type == DEV
    C = len(classes)
    score = torch.zeros(C, N, dtype=torch.float32, device=DEV)
    cap = torch.zeros(C, N, dtype=torch.int32, device=DEV)
    dim_w = torch.ones(R, dtype=torch.float32, device=DEV)
    keep = []
    for i, c in enumerate(classes):
        req = torch.from_numpy(nt.req_vector(c.task)).to(DEV)
        require = torch.from_numpy(c.require).to(DEV)
        forbid = torch.from_numpy(c.forbid).to(DEV)
        assert req.shape == (R,) and require.shape == forbid.shape == (W,)
        keep.append((req, require, forbid))
        hip.score_cap(nt.alloc_t, nt.used_t, None, nt.ready, nt.taint_mask,
                      nt.planes_t, req, c.tolerated, require, forbid,
                      1.0, 0.0, 0.0, dim_w, None, score[i], cap[i])
    torch.cuda.synchronize()
    return (score.cpu() > float("-inf")).tolist()


@pytest.mark.parametrize("name", ["f64-s0", "f128-s0", "taints64",
                                  "hostnames"])
def test_device_masks_equal_the_evaluator(name):
    w = world(name)
    _, _, sched = pc.build(w, DEV)
    ssn = sched.open_session()
    try:
        classes = pc.compiled(ssn)
    finally:
        sched.close_session(ssn)
    nt = ssn.node_tensors
    assert len(classes) == len(w.pods)
    assert nt.names == [n.meta.name for n in w.nodes]
    if name != "hostnames":
        assert nt.planes_t.shape[0] > 1
    got = device_masks(nt, classes)
    for c, mask in zip(classes, got):
        want = pc.mask(c.pod, w.nodes)
        assert mask == want, pc.first_difference(w, c, mask, want)
        host = pc.reference_mask(nt, c)
        assert mask == host, pc.first_difference(w, c, mask, host)


# --------------------------------------------------------------------------
# through the scheduler, HIP decision plane
# --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cycle_world():
    return pc.make_world(3, filler=64, n_nodes=130, n_pods=64)


@functools.lru_cache(maxsize=None)
def torch_binds():
    _, binder, sched = pc.build(cycle_world(), "cpu")
    sched.run_once()
    return dict(binder.binds)


@pytest.mark.parametrize("mode", [{}, {"VAMD_MEGACYCLE": 1},
                                  {"VAMD_CHAIN_CHUNK": 8}],
                         ids=["default", "megacycle", "chain8"])
def test_cycle_on_the_hip_plane(monkeypatch, mode):
    """Per-class tolerated / require / forbid rows from the real compiler,
    two words wide and distinct per class, in the [C, W] tables of the
    per-class, megacycle and chain paths."""
    from volcano_amd.scheduler.actions import allocate
    w = cycle_world()
    assert len(w.nodes) == 130 and len(w.pods) >= 40
    assert pc.static_pairs(w.nodes) == 64
    for var in MODE_VARS:
        monkeypatch.delenv(var, raising=False)
    for var, val in mode.items():
        monkeypatch.setenv(var, str(val))
    plans, real = [], allocate.run_plan_hip

    def spy(plan):
        plans.append(plan)
        return real(plan)

    monkeypatch.setattr(allocate, "run_plan_hip", spy)
    _, binder, sched = pc.build(w, DEV)
    sched.run_once()
    torch.cuda.synchronize()
    binds = dict(binder.binds)

    # what the megacycle and chain paths need to be taken at all
    assert len(plans) == 1
    plan = plans[0]
    single = [jp for jp in plan.jobs if jp.class_end - jp.class_begin == 1]
    assert len(single) >= 32 and len(single) == len(plan.jobs)
    assert all(cp.ntasks < 512 for cp in plan.classes)
    assert all(cp.spread is None and cp.affinity is None
               for cp in plan.classes)
    assert not plan.spread_groups
    W = plan.nt.planes_t.shape[0]
    assert W == 2
    rows = {(cp.tolerated, cp.require.tobytes(), cp.forbid.tobytes())
            for cp in plan.classes}
    assert all(len(cp.require) == W == len(cp.forbid) for cp in plan.classes)
    assert len(rows) >= 32
    assert any(cp.require[1] for cp in plan.classes)
    assert any(cp.forbid[1] for cp in plan.classes)

    assert 0 < len(binds) < len(w.pods)
    pc.check_binds(w, binds)
    assert binds == torch_binds()
