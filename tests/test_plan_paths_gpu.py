"""Every dispatch path of ``vamd_run_cycle`` against ``run_plan_torch``.

Plans are built straight from arrays (``_kernel_cases``: no scheduler, no
store, no synthetic cluster) on exact-arithmetic inputs with large tie
groups, three queues with one binding limit, per-class bias rows and a
plan-wide bias, future-idle scoring on and off, R in {5, 64}, W in {1, 4}.
The same plan runs through the torch oracle on the CPU and through the
HIP runner under each dispatch mode; logs (entry for entry, in order),
counters, final usage and final queue allocation must be identical.

Before any GPU comparison the oracle's own result is checked for
non-vacuity: a case cannot pass by placing nothing, never reverting,
never hitting a quota or never breaking a tie.
"""

import functools

import pytest
import torch

import _kernel_cases as kc

pytestmark = pytest.mark.gpu

DEV = "cuda"
CASES = kc.plan_cases()
TAGS = [f"R{R}W{W}" for R, W in kc.SHAPES]
MODE_VARS = ("VAMD_MEGACYCLE", "VAMD_CHAIN_CHUNK", "VAMD_NO_CHAIN")


@pytest.fixture(scope="module", autouse=True)
def _library():
    from volcano_amd.ops import hip
    hip._load()


@functools.lru_cache(maxsize=None)
def oracle(name):
    """The CPU reference of a case: computed once, never modified."""
    case = CASES[name][0]()
    snap, records, _ = kc.run_oracle(case)
    return case, snap, records


def run_hip(case):
    from volcano_amd.scheduler.plan import run_plan_hip
    plan = kc.build_plan(case, DEV)
    res = run_plan_hip(plan)
    if DEV == "cuda":
        torch.cuda.synchronize()
    return kc.snapshot(plan, res)


def set_mode(monkeypatch, **env):
    # the runner reads these per cycle
    for var in MODE_VARS:
        monkeypatch.delenv(var, raising=False)
    for var, val in env.items():
        monkeypatch.setenv(var, str(val))


def non_vacuous(name, chunk=None):
    case, snap, records = oracle(name)
    _, base, chunks = CASES[name]
    cond = kc.plan_conditions(case, snap, records)
    for key in base:
        assert cond[key], f"{name}: oracle run shows no {key}"
    for ch, key in chunks:
        if ch == chunk:
            cond = kc.plan_conditions(case, snap, records, chunk=ch)
            assert cond[key], f"{name}: chunk {ch} shows no {key}"
    return case, snap


def small_classes_only(case):
    return max(c["ntasks"] for c in case.classes) < 512


@pytest.mark.parametrize("tag", TAGS)
def test_fused_path(monkeypatch, tag):
    """N <= 4096, every class small: one fused launch per class."""
    case, want = non_vacuous(f"fused-{tag}")
    assert case.N <= 4096 and small_classes_only(case)
    set_mode(monkeypatch)
    kc.compare_results(want, run_hip(case))


@pytest.mark.parametrize("tag", TAGS)
def test_split_path(monkeypatch, tag):
    """N > 4096: grid-stride score kernel + serial select per class."""
    case, want = non_vacuous(f"split-{tag}")
    assert case.N > 4096 and small_classes_only(case)
    set_mode(monkeypatch)
    kc.compare_results(want, run_hip(case))


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("kind", ["single", "multi"])
def test_bulk_class_in_plan(monkeypatch, kind, tag):
    """A 600-task class takes the sort-based select; as one role of a gang
    that fails, its bulk log is undone by cond_revert."""
    case, want = non_vacuous(f"bulk-{kind}-{tag}")
    assert case.classes[0]["ntasks"] == 600 and case.N >= 512
    if kind == "multi":
        assert case.jobs[0][:2] == (0, 2)
        assert want["job_flag"][0] == 0 and want["log_len"][0] > 0
        assert want["class_placed"][0] == 0
    else:
        assert want["class_placed"][0] >= 512
    set_mode(monkeypatch)
    kc.compare_results(want, run_hip(case))


@pytest.mark.parametrize("tag", TAGS)
def test_megacycle_path(monkeypatch, tag):
    """VAMD_MEGACYCLE=1: 40 classes, multi-class jobs among them, in one
    launch — and the same plan through the default per-class path."""
    case, want = non_vacuous(f"mega-{tag}")
    assert len(case.classes) >= 32 and small_classes_only(case)
    assert any(e - b > 1 for b, e, _, _ in case.jobs)
    set_mode(monkeypatch, VAMD_MEGACYCLE=1)
    kc.compare_results(want, run_hip(case))
    set_mode(monkeypatch)
    kc.compare_results(want, run_hip(case))


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("chunk", [8, 512])
@pytest.mark.parametrize("shape", ["ragged", "wide", "hot"])
def test_chain_path(monkeypatch, shape, chunk, tag):
    """VAMD_CHAIN_CHUNK: batch score + top-k + select chain per chunk.
    "ragged": 70 jobs = several chunks and a ragged last one; "wide": one
    chunk touches more than 256 nodes; "hot": candidate lists are used up
    and the fallback scan runs.  VAMD_NO_CHAIN=1 must change nothing."""
    case, want = non_vacuous(f"chain-{shape}-{tag}", chunk=chunk)
    # the chain needs a run of >= 32 single-class small jobs
    assert len(case.jobs) >= 32 and small_classes_only(case)
    assert all(e - b == 1 for b, e, _, _ in case.jobs)
    set_mode(monkeypatch, VAMD_CHAIN_CHUNK=chunk)
    chained = run_hip(case)
    kc.compare_results(want, chained)
    set_mode(monkeypatch, VAMD_CHAIN_CHUNK=chunk, VAMD_NO_CHAIN=1)
    plain = run_hip(case)
    kc.compare_results(want, plain)
    kc.compare_results(chained, plain)
