"""The coherence scenarios of ``_coherence_cases`` on the HIP path.

Every plan goes through ``run_plan_hip`` (the recording wrapper of the world
refuses a plan that reaches the other runner).  After every action the
device tensors, the ledger and the per-task truth must be equal, and the
binds (task -> node) must be those of the torch-runner world built from the
same scenario: the inputs are exact, so this is decision equality.
"""

import functools

import pytest
import torch

import _coherence_cases as cc

pytestmark = pytest.mark.gpu

DEV = "cuda"
MODE_VARS = ("VAMD_MEGACYCLE", "VAMD_CHAIN_CHUNK", "VAMD_NO_CHAIN")


@pytest.fixture(scope="module", autouse=True)
def _library():
    from volcano_amd.ops import hip
    hip._load()      # the HIP library must be there: no silent fallback


@functools.lru_cache(maxsize=None)
def cpu_binds(name):
    """Binds of the torch-runner world: computed once, never modified."""
    world = cc.World(cc.SCENARIOS[name], "cpu")
    world.run()
    assert all(world.conditions().values())
    return world.binds()


def set_mode(monkeypatch, **env):
    # the runner reads these per cycle
    for var in MODE_VARS:
        monkeypatch.delenv(var, raising=False)
    for var, val in env.items():
        monkeypatch.setenv(var, str(val))


def run_on_gpu(name, monkeypatch, native="1"):
    monkeypatch.setenv("VAMD_NATIVE_APPLY", native)
    want = cpu_binds(name)
    world = cc.World(cc.SCENARIOS[name], DEV)
    world.run()
    torch.cuda.synchronize()
    sc = world.scenario
    assert world.cache.node_tensors.used_t.is_cuda
    assert [r.action for r in world.reports] == sc.actions * sc.cycles
    for rep in world.reports:
        cc.assert_coherent(rep)
    got = world.binds()
    assert got == want, (
        f"{name}: {len(got)} binds on the HIP path, {len(want)} on the "
        f"torch runner; first difference "
        f"{sorted(set(got.items()) ^ set(want.items()))[:4]}")
    return world


@pytest.mark.parametrize("name", list(cc.SCENARIOS))
def test_scenario_is_coherent_after_every_action(monkeypatch, name):
    set_mode(monkeypatch)
    world = run_on_gpu(name, monkeypatch)
    if name != "preempt_nominated":
        assert world.runs, "no plan reached run_plan_hip"


@pytest.mark.parametrize("mode", [{"VAMD_MEGACYCLE": 1},
                                  {"VAMD_CHAIN_CHUNK": 8}],
                         ids=["megacycle", "chain8"])
def test_small_gangs_under_the_other_dispatch_modes(monkeypatch, mode):
    set_mode(monkeypatch, **mode)
    world = run_on_gpu("small_gangs", monkeypatch)
    plan = cc.allocate_runs(world)[0].plan
    assert len(plan.jobs) >= 32
    assert all(jp.class_end - jp.class_begin == 1 for jp in plan.jobs)
    assert max(cp.ntasks for cp in plan.classes) < 512


@pytest.mark.parametrize("native", ["1", "0"])
@pytest.mark.parametrize("name", cc.BUNDLE_SCENARIOS)
def test_bundles_with_native_apply_on_and_off(monkeypatch, name, native):
    set_mode(monkeypatch)
    world = run_on_gpu(name, monkeypatch, native)
    stats = getattr(world.allocate, "last_walk_stats", None)
    assert (stats is not None) == (native == "1")
    assert any(r.bundle for r in world.reverts)
    if name == "bundle_short":
        big = [cp for cp in cc.allocate_runs(world)[0].plan.classes
               if cp.bundle is not None and cp.ntasks >= 512]
        assert len(big) == 1 and world.cache.node_tensors.n >= 512
