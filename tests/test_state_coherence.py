"""Device usage and queue rows against the host truth after every action,
on the torch runner (``_coherence_cases``).

Each scenario first proves that the path it exists for was taken (its
*conditions*), then every report of every action has to be coherent: the
ledger's ``USED`` plane, ``nt.used_t`` and the per-task truth are equal, and
so are ``ssn.queue_alloc`` and the per-task queue rows.  The mutation tests
show that the comparison is not vacuous: with the host give-back disabled,
or with only the partial first piece of an unclaimed tail lost, the same run
fails it.
"""

import numpy as np
import pytest

import _coherence_cases as cc
from volcano_amd.scheduler.actions.allocate import AllocateAction

NATIVE = ["1", "0"]


def run_world(scenario, monkeypatch, native):
    monkeypatch.setenv("VAMD_NATIVE_APPLY", native)
    world = cc.World(scenario, "cpu")
    world.run()
    walked_native = getattr(world.allocate, "last_walk_stats", None)
    assert (walked_native is not None) == (native == "1")
    return world


def assert_conditions(world):
    cond = world.conditions()
    assert cond, "scenario records no condition"
    missed = [k for k, ok in cond.items() if not ok]
    assert not missed, f"{world.scenario.name}: not reached: {missed}"


def assert_all_coherent(world):
    assert world.reports
    for rep in world.reports:
        cc.assert_coherent(rep)


@pytest.mark.parametrize("native", NATIVE)
@pytest.mark.parametrize("name", list(cc.SCENARIOS))
def test_scenario_is_coherent_after_every_action(monkeypatch, name, native):
    world = run_world(cc.SCENARIOS[name], monkeypatch, native)
    sc = world.scenario
    assert world.cache.node_tensors.n == sc.n_nodes <= 1024
    assert [r.action for r in world.reports] == sc.actions * sc.cycles
    assert_conditions(world)
    assert_all_coherent(world)


@pytest.mark.parametrize("native", NATIVE)
@pytest.mark.parametrize("name", cc.GIVE_BACK)
def test_without_the_give_back_the_check_fails(monkeypatch, name, native):
    """Mutant: ``_revert_pieces`` gives nothing back."""
    monkeypatch.setattr(AllocateAction, "_revert_pieces",
                        staticmethod(cc.revert_nothing))
    world = run_world(cc.SCENARIOS[name], monkeypatch, native)
    assert world.reverts, "the run asked for no give-back"
    with pytest.raises(AssertionError, match="used_t != truth"):
        assert_all_coherent(world)


@pytest.mark.parametrize("native", NATIVE)
def test_losing_the_partial_first_piece_fails(monkeypatch, native):
    """Mutant: only the partial first piece of the unclaimed tail is lost;
    every whole entry of the tail is still given back."""
    ref = [None]
    monkeypatch.setattr(AllocateAction, "_revert_pieces",
                        staticmethod(cc.make_drop_partial_first(ref)))
    monkeypatch.setenv("VAMD_NATIVE_APPLY", native)
    world = ref[0] = cc.World(cc.SCENARIOS["bundle_short"], "cpu")
    world.run()
    assert_conditions(world)        # the spy still saw the partial piece
    reps = [r for r in world.reports if r.action == "allocate"]
    off = np.argwhere(reps[0].used_t != reps[0].truth_used)
    # one node, every dim of the request, nothing else
    assert len(set(off[:, 0].tolist())) == 1 and len(off) == 3
    with pytest.raises(AssertionError, match="used_t != truth"):
        assert_all_coherent(world)


def test_mutants_are_gone_afterwards():
    assert AllocateAction.__dict__["_revert_pieces"].__func__.__name__ \
        == "_revert_pieces"


@pytest.mark.parametrize("native", NATIVE)
def test_byte_scale_bundle_stays_within_the_derived_bound(monkeypatch,
                                                          native, capsys):
    """Memory ``1500M``: 3 * 1.5e9 is no f32 value, so commit and give-back
    round.  ``|used_t - truth| <= (3 k + 1) / 2 * ulp_f32(alloc)`` per
    element (``cc.byte_bound``); the ledger, summed in f64, stays exact."""
    world = run_world(cc.BUNDLE_SHORT_BYTES, monkeypatch, native)
    assert_conditions(world)
    bound = cc.byte_bound(world)
    mem = world.cache.node_tensors.dims.index["memory"]
    worst = 0.0
    for rep in world.reports:
        assert np.array_equal(rep.ledger_used, rep.truth_used)
        err = np.abs(rep.used_t - rep.truth_used)
        at = np.unravel_index(np.argmax(err), err.shape)
        with capsys.disabled():
            print(f"\n[bytes native={native}] after {rep.action}: "
                  f"max |used_t - truth| = {err.max():.0f} B at {at}, "
                  f"bound there {bound[at]:.0f} B")
        worst = max(worst, float(err.max()))
        assert (err <= bound).all(), \
            f"after {rep.action}: {err.max()} over the bound at {at}"
        # the other dims are still whole numbers
        exact = np.delete(err, mem, axis=1)
        assert not exact.any()
    assert worst > 0.0, "nothing rounded: the twin is not byte-scale"
