"""Every dispatch path of ``vamd_run_cycle`` on inexact inputs.

``test_plan_paths_gpu.py`` pins the paths bit for bit against the torch
oracle on inputs where no f32 operation rounds, with ``w_bal`` = 0.  Here
``alloc`` is no power of two, the dim weights do not sum to one, the bias
is a multiple of 0.3 and every class carries the balanced-allocation term
(``w_bal`` = 1, the production default), so every operation of the score
rounds.  Nothing is compared with the f32 oracle:

* each path's result must pass ``_kernel_cases.validate_plan``, a float64
  replay that accepts an order only within the measured ``KERNEL_ERR`` and
  holds exact twins to index order with no tolerance;
* the paths must agree with each other bit for bit (same
  ``node_score_one`` on the same inputs): logs in order, counters, usage;
* with decimal byte-scale memory in one dim, a discarded single-class gang
  must leave no trace: the plan without the discarded jobs ends in
  bit-equal usage.
"""

import functools
import hashlib

import pytest
import torch

import _kernel_cases as kc

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = kc.inexact_plan_cases()
BYTES = kc.byte_plan_cases()
TAGS = [f"R{R}W{W}" for R, W in kc.SHAPES]
MODE_VARS = ("VAMD_MEGACYCLE", "VAMD_CHAIN_CHUNK", "VAMD_NO_CHAIN")


@pytest.fixture(scope="module", autouse=True)
def _library():
    from volcano_amd.ops import hip
    hip._load()


@functools.lru_cache(maxsize=None)
def case_of(name):
    return (CASES.get(name) or BYTES[name])[0]()


def run_hip(case, monkeypatch, **env):
    from volcano_amd.scheduler.plan import run_plan_hip
    # the runner reads these per cycle
    for var in MODE_VARS:
        monkeypatch.delenv(var, raising=False)
    for var, val in env.items():
        monkeypatch.setenv(var, str(val))
    plan = kc.build_plan(case, DEV)
    res = run_plan_hip(plan)
    torch.cuda.synchronize()
    return kc.snapshot(plan, res)


_VALID = {}


def validate(name, case, snap):
    """kc.validate_plan(case, snap).  It is a pure function of what it
    reads from the snapshot, so a result whose every such byte equals an
    accepted one's is accepted without a second replay (the modes are
    meant to be bit-identical; the replay of a 300-class plan at R = 64
    takes seconds)."""
    h = hashlib.sha1()
    for c, (off, n) in enumerate(zip(snap["log_off"], snap["log_len"])):
        for key in ("log_nodes", "log_counts"):
            h.update(snap[key][int(off):int(off) + int(n)].tobytes())
    for key in ("log_len", "class_placed", "job_placed", "job_flag", "used",
                "queue_alloc"):
        h.update(snap[key].tobytes())
    if _VALID.get(name) != h.digest():
        kc.validate_plan(case, snap)
        _VALID[name] = h.digest()


def small_classes_only(case):
    return max(c["ntasks"] for c in case.classes) < 512


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("shape", ["fused", "split", "bulk-single",
                                   "bulk-multi"])
def test_per_class_paths_are_valid(monkeypatch, shape, tag):
    """Default mode: fused launch (N <= 4096), score + select (N > 4096),
    and the sort-based select for the 600-task class."""
    name = f"{shape}-{tag}"
    case = case_of(name)
    assert (case.N <= 4096) == (shape in ("fused", "bulk-single"))
    assert small_classes_only(case) == (not shape.startswith("bulk"))
    validate(name, case, run_hip(case, monkeypatch))


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("N", [1000, 4097])
def test_megacycle_is_valid_and_equals_per_class(monkeypatch, N, tag):
    """40 classes, multi-class jobs among them, in one launch; the same
    plan per class (fused at N = 1000, score + select at N = 4097)."""
    name = f"mega-N{N}-{tag}"
    case = case_of(name)
    assert len(case.classes) >= 32 and small_classes_only(case)
    assert any(e - b > 1 for b, e, _, _ in case.jobs)
    mega = run_hip(case, monkeypatch, VAMD_MEGACYCLE=1)
    validate(name, case, mega)
    plain = run_hip(case, monkeypatch)
    validate(name, case, plain)
    kc.compare_results(plain, mega)


CHAIN_N = {"ragged": (1000, 4097), "hot": (1000, 4097), "wide": (600, 4097)}


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("big", [0, 1])
@pytest.mark.parametrize("shape", ["ragged", "wide", "hot"])
def test_chain_is_valid_and_equals_every_other_path(monkeypatch, shape, big,
                                                    tag):
    """Runs of single-class jobs through the chain at chunk 8 and 512,
    with the chain switched off, per class and through the megacycle: all
    valid, all bit-identical."""
    name = f"chain-{shape}-N{CHAIN_N[shape][big]}-{tag}"
    case = case_of(name)
    assert len(case.jobs) >= 32 and small_classes_only(case)
    assert all(e - b == 1 for b, e, _, _ in case.jobs)
    plain = run_hip(case, monkeypatch)
    validate(name, case, plain)
    for env in (dict(VAMD_CHAIN_CHUNK=8), dict(VAMD_CHAIN_CHUNK=512),
                dict(VAMD_CHAIN_CHUNK=8, VAMD_NO_CHAIN=1),
                dict(VAMD_MEGACYCLE=1)):
        got = run_hip(case, monkeypatch, **env)
        validate(name, case, got)
        kc.compare_results(plain, got)


BYTE_MODES = {
    "fused-bytes": (dict(),),
    "mega-bytes": (dict(), dict(VAMD_MEGACYCLE=1)),
    "chain-bytes": (dict(), dict(VAMD_MEGACYCLE=1), dict(VAMD_CHAIN_CHUNK=8),
                    dict(VAMD_CHAIN_CHUNK=512)),
}


@pytest.mark.parametrize("name", sorted(BYTES))
def test_discarded_single_class_gang_leaves_no_trace(monkeypatch, name):
    """Byte-scale memory in one dim (tests/test_inexact_cases.py shows the
    discarded logs of these plans leave residues under f32 add-then-
    subtract).  Every mode gives the same result, and the plan without its
    discarded single-class jobs ends bit-equal."""
    case = case_of(name)
    plain = run_hip(case, monkeypatch)
    drop = set(kc.discarded_single_jobs(case, plain))
    assert drop
    pruned = run_hip(kc.without_jobs(case, drop), monkeypatch)
    for env in BYTE_MODES[name]:
        got = run_hip(case, monkeypatch, **env)
        kc.compare_results(plain, got)
        kc.same_trace(got, pruned, case, drop)
