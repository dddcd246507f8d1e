"""Differential tests of the host-native per-job loops against their Python
loops: the JobTable column scan, the fused-run bundle entries, the bulk
pod-group phase store, and a whole cycle with ``VAMD_NATIVE_JOBS`` on and
off.  Inventories are built by hand so every edge is in plain sight."""

import random
import types

import numpy as np
import pytest

from volcano_amd.api.info import JobInfo, TaskInfo
from volcano_amd.api.objects import PodGroup
from volcano_amd.api.resource import Resource
from volcano_amd.api.types import PodGroupPhase, TaskStatus
from volcano_amd.ops import host
from volcano_amd.scheduler import (FakeBinder, Scheduler, SchedulerCache,
                                   default_config)
from volcano_amd.scheduler.actions.allocate import AllocateAction
from volcano_amd.scheduler.jobtable import (_PHASE_MAP, PH_INQUEUE, PH_OTHER,
                                            PH_PENDING, PH_RUNNING, JobTable)
from volcano_amd.scheduler.plan import BundleEntry
from volcano_amd.store import ObjectStore
from volcano_amd.utils import synth

P, F, B = TaskStatus.PENDING, TaskStatus.FAILED, TaskStatus.BOUND
INQ = PodGroupPhase.INQUEUE.value
RUN = PodGroupPhase.RUNNING.value


@pytest.fixture(autouse=True)
def _native_on(monkeypatch):
    monkeypatch.setenv("VAMD_NATIVE_JOBS", "1")
    assert host.native_jobs_enabled()


def mk_job(name, statuses, phase=INQ, podgroup=True, gated_first=False):
    """A JobInfo with one task per entry of ``statuses``."""
    pg = None
    if podgroup:
        pg = PodGroup()
        pg.status.phase = phase
    job = JobInfo(f"default/{name}", pg)
    for t, st in enumerate(statuses):
        job.add_task(TaskInfo(
            uid=f"{name}-{t}", name=f"{name}-{t}", namespace="default",
            job_key=job.key, role="worker", request=Resource(),
            status=st, gated=gated_first and t == 0))
    return job


# -- column scan --------------------------------------------------------------

def scan_inventory():
    jobs = [
        mk_job("plain", [P, P, P]),
        mk_job("nopg", [P], podgroup=False),
        mk_job("odd-phase", [P, P], phase="Completed"),
        mk_job("empty-pending", [B, B], phase=RUN),
        mk_job("no-pending-key", [B], phase=RUN),
        mk_job("failed-2", [F, F, P], phase=RUN),
        mk_job("pending-phase", [P], phase=PodGroupPhase.PENDING.value),
    ]
    jobs[3].task_status_index[P] = {}          # empty dict, key present
    assert P not in jobs[4].task_status_index  # key missing
    assert jobs[3]._occ == 2                   # non-zero occupancy
    return jobs


def table_of(jobs):
    jt = JobTable()
    jt.jobs = jobs
    jt._vers = np.array([j._tver for j in jobs], dtype=np.int64)
    return jt


def columns(jt):
    return [jt.occ.tolist(), jt.npend.tolist(), jt.nfailed.tolist(),
            jt.phase.tolist()]


@pytest.mark.parametrize("J", [0, 1, 7])
def test_scan_matches_refresh_dynamic(J):
    jobs = scan_inventory()[:J]
    jt = table_of(jobs)
    dirty = jt._scan_native()
    got = columns(jt)
    assert [a.dtype for a in (jt.occ, jt.npend, jt.nfailed, jt.phase)] == \
        [np.int64, np.int64, np.int64, np.int8]
    jt._refresh_dynamic()
    assert got == columns(jt)
    assert dirty == []
    if J == 7:
        assert got == [[0, 0, 0, 2, 1, 0, 0],
                       [3, 1, 2, 0, 0, 1, 1],
                       [0, 0, 0, 0, 0, 2, 0],
                       [PH_INQUEUE, PH_PENDING, PH_OTHER, PH_RUNNING,
                        PH_RUNNING, PH_RUNNING, PH_PENDING]]


def test_scan_returns_only_the_bumped_row():
    jobs = scan_inventory()
    jt = table_of(jobs)
    jobs[5]._tver += 1
    assert jt._scan_native() == [5]
    assert [k for k, j in enumerate(jobs) if j._tver != jt._vers[k]] == [5]


def test_scan_rejects_wrong_columns():
    jobs = scan_inventory()
    vers = np.zeros(7, dtype=np.int64)

    def call(vers=vers, occ=None, phase=None):
        col = lambda: np.zeros(7, dtype=np.int64)    # noqa: E731
        return host.load().scan_jobs(
            jobs, P, F, _PHASE_MAP, PH_PENDING, PH_OTHER, vers,
            col() if occ is None else occ, col(), col(),
            np.zeros(7, dtype=np.int8) if phase is None else phase)

    call()
    for bad in (dict(occ=np.zeros(6, dtype=np.int64)),       # short
                dict(vers=np.zeros(8, dtype=np.int64)),      # long
                dict(occ=np.zeros(7, dtype=np.int32)),       # narrow
                dict(occ=np.zeros(7, dtype=np.float64)),     # not integer
                dict(phase=np.zeros(7, dtype=np.int64))):    # wide
        with pytest.raises((ValueError, TypeError)):
            call(**bad)
    ro = np.zeros(7, dtype=np.int64)
    ro.setflags(write=False)
    with pytest.raises((ValueError, TypeError, BufferError)):
        call(occ=ro)


def test_scan_propagates_attribute_errors():
    jobs = scan_inventory()
    del jobs[2]._occ
    with pytest.raises(AttributeError):
        table_of(jobs)._scan_native()


# -- bundle entries -----------------------------------------------------------

def entries_both(jobs_l, i, j, gm_l):
    nat = host.load().bundle_entries(jobs_l, i, j, gm_l, P, BundleEntry)
    ref = AllocateAction._run_entries_py(jobs_l, i, j, gm_l, P, BundleEntry)
    assert len(nat[0]) == len(ref[0])
    for a, b in zip(nat[0], ref[0]):
        assert type(a) is BundleEntry
        assert a.job_key == b.job_key
        assert a.tasks == b.tasks and all(
            x is y for x, y in zip(a.tasks, b.tasks))
        assert (a.ntasks, a.min_needed) == (b.ntasks, b.min_needed)
        assert a.job is b.job
        assert a == b
    assert nat[1:] == ref[1:]
    return nat


def test_entries_smallest_run():
    jobs_l = [mk_job("a", [P, P]), mk_job("b", [P, P, P])]
    entries, total, mn = entries_both(jobs_l, 0, 2, [2, 3])
    assert [e.job for e in entries] == jobs_l
    assert (total, mn) == (5, 2)
    assert [t.key for t in entries[1].tasks] == \
        list(jobs_l[1].task_status_index[P])        # dict order


def test_entries_skip_empty_and_gated_inside_a_window():
    jobs_l = [mk_job("pre", [P]),                       # outside: i > 0
              mk_job("r0", [P, P]), mk_job("r1", [P, P], gated_first=True),
              mk_job("r2", [B, B]), mk_job("r3", [P, P, P]),
              mk_job("r4", [P]),
              mk_job("post", [P])]                      # outside: j < L
    jobs_l[3].task_status_index[P] = {}                 # middle job: empty
    gm_l = [9, 2, 1, 1, 3, 1, 9]
    entries, total, mn = entries_both(jobs_l, 1, 6, gm_l)
    assert [e.job.key for e in entries] == \
        ["default/r0", "default/r3", "default/r4"]
    assert (total, mn) == (6, 1)
    # the skipped gated job carried the smallest minimum of its neighbours
    entries, total, mn = entries_both(jobs_l, 1, 5, gm_l)
    assert (total, mn) == (5, 2)


def test_entries_every_job_skipped():
    jobs_l = [mk_job("g", [P], gated_first=True), mk_job("b", [B])]
    assert entries_both(jobs_l, 0, 2, [1, 1]) == ([], 0, 1 << 60)
    assert entries_both(jobs_l, 1, 1, [1, 1]) == ([], 0, 1 << 60)


def test_entries_other_entry_types_and_bad_windows():
    jobs_l = [mk_job("a", [P, P]), mk_job("b", [P])]

    class Loose:                       # no slots: built by calling the type
        def __init__(self, job_key, tasks, ntasks, min_needed, job):
            self.args = (job_key, tasks, ntasks, min_needed, job)

    entries, total, mn = host.load().bundle_entries(
        jobs_l, 0, 2, [2, 1], P, Loose)
    assert [e.args[0] for e in entries] == ["default/a", "default/b"]
    assert entries[0].args[2:] == (2, 2, jobs_l[0])
    for i, j in ((-1, 1), (1, 0), (0, 3)):
        with pytest.raises(IndexError):
            host.load().bundle_entries(jobs_l, i, j, [2, 1], P, BundleEntry)
    with pytest.raises(IndexError):
        host.load().bundle_entries(jobs_l, 0, 2, [2], P, BundleEntry)


# -- phase helper -------------------------------------------------------------

def test_phase_helper_changed_and_gated():
    jobs = [mk_job("pend", [P], phase="Pending"),
            mk_job("nopg", [P], podgroup=False),
            mk_job("already", [P], phase=INQ),
            mk_job("gated", [P, P], phase="Pending", gated_first=True),
            mk_job("gated-nopg", [P], podgroup=False, gated_first=True)]
    changed, gated = host.load().set_podgroup_phase(jobs, INQ, True)
    assert changed == [jobs[0], jobs[3]]
    assert gated == [jobs[3], jobs[4]]
    assert [j.phase for j in jobs] == [INQ, "Pending", INQ, INQ, "Pending"]
    assert jobs[1].podgroup is None
    # nothing left to change; the gated list is only built on request
    assert host.load().set_podgroup_phase(jobs, INQ) == ([], [])
    assert host.load().set_podgroup_phase([], RUN, True) == ([], [])


# -- whole cycle --------------------------------------------------------------

class Recorder:
    def __init__(self):
        self.calls = []

    def on_allocate(self, tclass, node_ids, counts, tasks):
        self.calls.append((list(node_ids), list(counts),
                           [t.key for t in tasks]))


def populate_random(store, rng, roomy):
    for n in synth.make_nodes(40, cpu_milli=64000 if roomy else 8000,
                              mem=256 * 1024 ** 3):
        store.create("Node", n)
    store.create("Queue", synth.make_queue("default"))
    store.create("Queue", synth.make_queue("other"))
    for j in range(30):
        shape = rng.choice(["gang4", "gang4", "gang4", "big", "loose", "one"])
        queue = "other" if rng.random() < 0.25 else "default"
        if shape == "gang4":        # identical gangs: fused runs
            synth.make_gang(store, f"job-{j:02d}", replicas=4, queue=queue,
                            cpu_milli=1000, mem=1024 ** 3)
        elif shape == "big":        # may not fit: gang miss
            synth.make_gang(store, f"job-{j:02d}", replicas=rng.randint(8, 40),
                            queue=queue, cpu_milli=4000, mem=1024 ** 3)
        elif shape == "loose":      # partial placement allowed
            synth.make_gang(store, f"job-{j:02d}", replicas=6, queue=queue,
                            cpu_milli=2000, mem=1024 ** 3, min_member=2)
        else:
            synth.make_gang(store, f"job-{j:02d}", replicas=1, queue=queue,
                            cpu_milli=500, mem=1024 ** 3)


def populate_partial(store):
    """Room for one whole gang and half of a loose job: the commit set
    mixes whole-gang jobs with a partly placed one."""
    for n in synth.make_nodes(2, cpu_milli=8000, mem=32 * 1024 ** 3):
        store.create("Node", n)
    store.create("Queue", synth.make_queue("default"))
    synth.make_gang(store, "job-00", replicas=4, cpu_milli=1000,
                    mem=1024 ** 3, priority=10)
    synth.make_gang(store, "job-01", replicas=6, cpu_milli=3000,
                    mem=1024 ** 3, min_member=2, priority=5)
    synth.make_gang(store, "job-02", replicas=2, cpu_milli=500,
                    mem=1024 ** 3, priority=1)


def run_cycle(seed, handler, monkeypatch, roomy=False):
    """One ``run_once`` over 40 nodes and 30 mixed jobs.  A tight cluster
    leaves gangs unplaced and makes enqueue vote job by job; a roomy one
    admits each queue in bulk and places everything."""
    store = ObjectStore()
    if seed == "partial":
        populate_partial(store)
    else:
        populate_random(store, random.Random(seed), roomy)
    binder = FakeBinder()
    cache = SchedulerCache(store=store, binder=binder, device="cpu")
    sched = Scheduler(cache, default_config())
    recorder = Recorder() if handler else None
    if recorder is not None:
        opened = sched.open_session

        def open_with_handler():
            ssn = opened()
            ssn.event_handlers.append(recorder)
            return ssn
        monkeypatch.setattr(sched, "open_session", open_with_handler)
    rv0 = store.resource_version
    sched.run_once()
    jt = cache.job_table
    return {
        "tasks": {t.key: (t.node_name, int(t.status))
                  for job in cache.jobs.values()
                  for t in job.tasks.values()},
        "phases": {k: job.phase for k, job in cache.jobs.items()},
        "binds": list(binder.binds.items()),
        "nodes": {ni.name: list(ni.tasks) for ni in cache.nodes.values()},
        # the store sees update_podgroup calls in call order
        "journal": [(e[1], e[2], e[3]["meta"]["name"],
                     e[3].get("status", {}).get("phase"))
                    for e in store.journal_since(rv0)],
        "table": [c.tolist() for c in (
            jt.occ, jt.npend, jt.nfailed, jt.phase, jt.minav, jt.ntasks,
            jt.qi, jt.sigid, jt.gangmin)],
        "events": recorder.calls if recorder else None,
    }


@pytest.mark.parametrize(
    "seed,handler,roomy",
    [(s, False, False) for s in range(4)] + [(4, False, True),
                                             (5, False, True),
                                             (100, True, False),
                                             (101, True, True)])
def test_whole_cycle_matches_python_loops(seed, handler, roomy, monkeypatch):
    calls = counting_module(monkeypatch)
    native = run_cycle(seed, handler, monkeypatch, roomy)
    assert calls["scan_jobs"] and calls["bundle_entries"] and \
        calls["set_podgroup_phase"], calls
    if roomy:       # enqueue's bulk admit (one per queue) and apply's flip
        assert calls["set_podgroup_phase"] >= 3, calls
    monkeypatch.setenv("VAMD_NATIVE_JOBS", "0")
    oracle = run_cycle(seed, handler, monkeypatch, roomy)
    for k in oracle:
        assert native[k] == oracle[k], k
    n_bound = sum(1 for _, st in native["tasks"].values() if st == int(B))
    assert n_bound == len(native["tasks"]) if roomy else \
        20 < n_bound < len(native["tasks"])
    assert any(ph == RUN for ph in native["phases"].values())
    assert any(e[1] == "PodGroup" for e in native["journal"])
    if handler:
        assert native["events"]


# -- switch -------------------------------------------------------------------

def counting_module(monkeypatch):
    real = host.load()
    calls = {}

    def wrap(name):
        fn = getattr(real, name)

        def counted(*a, **kw):
            calls[name] += 1
            return fn(*a, **kw)
        calls[name] = 0
        return counted

    names = [n for n in dir(real) if not n.startswith("_")]
    monkeypatch.setattr(host, "_mod", types.SimpleNamespace(
        **{n: wrap(n) for n in names}))
    return calls


def test_switch_off_takes_the_python_loops(monkeypatch):
    calls = counting_module(monkeypatch)
    monkeypatch.setenv("VAMD_NATIVE_JOBS", "0")
    assert not host.native_jobs_enabled()
    run_cycle(0, False, monkeypatch)
    assert calls["apply_walk"] >= 1            # its own switch is still on
    assert calls["scan_jobs"] == calls["bundle_entries"] == \
        calls["set_podgroup_phase"] == 0


def test_module_without_the_functions_disables_the_switch(monkeypatch):
    real = host.load()
    monkeypatch.setattr(host, "_mod", types.SimpleNamespace(
        apply_walk=real.apply_walk, finish_binds=real.finish_binds))
    assert host.native_apply_enabled()
    assert not host.native_jobs_enabled()


def test_whole_cycle_with_whole_and_partial_gangs(monkeypatch):
    native = run_cycle("partial", False, monkeypatch)
    monkeypatch.setenv("VAMD_NATIVE_JOBS", "0")
    oracle = run_cycle("partial", False, monkeypatch)
    for k in oracle:
        assert native[k] == oracle[k], k
    bound = {}
    for key, (_, st) in native["tasks"].items():
        bound.setdefault(key.split("-worker-")[0], []).append(
            st == int(B))
    assert all(bound["default/job-00"]) and all(bound["default/job-02"])
    assert any(bound["default/job-01"]) and not all(bound["default/job-01"])
    assert [e[2] for e in native["journal"] if e[3] == RUN] == \
        ["job-00", "job-01", "job-02"]
