"""Reference-count and collector hygiene of the host-native per-job loops:
repeated calls leak nothing, the task lists they build stay out of the
cyclic collector's sight, and reference counting alone frees the plan."""

import gc
import sys
import weakref

import numpy as np
import pytest

from volcano_amd.api.info import JobInfo, TaskInfo
from volcano_amd.api.objects import PodGroup
from volcano_amd.api.resource import Resource
from volcano_amd.api.types import PodGroupPhase, TaskStatus
from volcano_amd.ops import host
from volcano_amd.scheduler.jobtable import (_PHASE_MAP, PH_OTHER, PH_PENDING)
from volcano_amd.scheduler.plan import BundleEntry

P, F = TaskStatus.PENDING, TaskStatus.FAILED
INQ = PodGroupPhase.INQUEUE.value
RUN = PodGroupPhase.RUNNING.value
N_CALLS = 200


@pytest.fixture(autouse=True)
def _native_on(monkeypatch):
    monkeypatch.setenv("VAMD_NATIVE_JOBS", "1")
    assert host.native_jobs_enabled()


def inventory():
    jobs = []
    for j, (n, phase) in enumerate([(3, INQ), (2, RUN), (4, "Pending"),
                                    (1, None)]):
        pg = None
        if phase is not None:
            pg = PodGroup()
            pg.status.phase = phase
        job = JobInfo(f"default/job-{j}", pg)
        for t in range(n):
            job.add_task(TaskInfo(
                uid=f"j{j}-{t}", name=f"j{j}-{t}", namespace="default",
                job_key=job.key, role="worker", request=Resource()))
        jobs.append(job)
    return jobs


def sampled(jobs, phases):
    tasks = [t for job in jobs for t in job.tasks.values()]
    return jobs + tasks + [P, F] + phases


def counts(objs):
    return [sys.getrefcount(o) for o in objs]


def test_scan_jobs_leaks_nothing():
    jobs = inventory()
    vers = np.array([j._tver for j in jobs], dtype=np.int64)
    vers[1] -= 1                               # one dirty row per call
    cols = [np.zeros(4, dtype=np.int64) for _ in range(3)] + \
        [np.zeros(4, dtype=np.int8)]
    objs = sampled(jobs, [INQ, RUN, jobs[2].podgroup.status.phase]) + \
        cols + [vers, _PHASE_MAP]
    before = counts(objs)
    for _ in range(N_CALLS):
        dirty = host.load().scan_jobs(jobs, P, F, _PHASE_MAP, PH_PENDING,
                                      PH_OTHER, vers, *cols)
    assert dirty == [1]
    del dirty
    assert counts(objs) == before              # buffers released as well


def test_bundle_entries_leaks_nothing():
    jobs = inventory()
    gm_l = [3000, 2000, 4000, 1000]        # above the shared small ints
    objs = sampled(jobs, []) + gm_l
    before = counts(objs)
    for _ in range(N_CALLS):
        out = host.load().bundle_entries(jobs, 0, 4, gm_l, P, BundleEntry)
    assert len(out[0]) == 4 and out[1:] == (10, 1000)
    del out
    assert counts(objs) == before


def test_set_podgroup_phase_leaks_nothing():
    jobs = inventory()
    jobs[0]._gated = 1
    phases = [INQ, RUN]
    objs = sampled(jobs, phases)
    first = [j.podgroup.status.phase for j in jobs[:3]]
    before = counts(objs)
    for k in range(N_CALLS):
        out = host.load().set_podgroup_phase(jobs, phases[k % 2], True)
    assert out == (jobs[:3], jobs[:1])         # INQ -> RUN on the last call
    del out
    assert [j.podgroup.status.phase for j in jobs[:3]] == [RUN] * 3
    for j, ph in zip(jobs, first):             # back to the first state
        j.podgroup.status.phase = ph
    del j, ph
    assert counts(objs) == before


def test_entry_task_lists_are_untracked_and_entries_tracked():
    jobs = inventory()
    entries, _, _ = host.load().bundle_entries(jobs, 0, 4, [3, 2, 4, 1], P,
                                               BundleEntry)
    assert all(not gc.is_tracked(e.tasks) for e in entries)
    assert all(gc.is_tracked(e) for e in entries)
    assert [len(e.tasks) for e in entries] == [3, 2, 4, 1]


class WeakEntry(BundleEntry):
    """BundleEntry is slotted without ``__weakref__``; this subclass keeps
    its five slots at the same offsets and adds the weak-reference one."""
    __slots__ = ("__weakref__",)


def test_refcount_alone_frees_the_entries():
    jobs = inventory()
    task = next(iter(jobs[0].tasks.values()))
    base = sys.getrefcount(task)
    gc.collect()
    gc.disable()
    try:
        entries, _, _ = host.load().bundle_entries(
            jobs, 0, 4, [3, 2, 4, 1], P, WeakEntry)
        assert type(entries[0]) is WeakEntry
        assert entries[0].job is jobs[0] and entries[0].ntasks == 3
        assert sys.getrefcount(task) == base + 1
        refs = [weakref.ref(e) for e in entries]
        plan = {"bundle": entries}
        del entries
        assert all(r() is not None for r in refs)
        del plan
        assert all(r() is None for r in refs)
        assert sys.getrefcount(task) == base
    finally:
        gc.enable()


def test_apply_walk_bind_lists_untracked_handler_lists_tracked(monkeypatch):
    from test_native_apply import World

    monkeypatch.setenv("VAMD_NATIVE_APPLY", "1")
    seen = {}
    real = host.load()

    class Spy:
        def __getattr__(self, name):
            return getattr(real, name)

        def apply_walk(self, *a):
            out = real.apply_walk(*a)
            seen["bind_by_job"], seen["events"] = out[3], out[6]
            return out

    monkeypatch.setattr(host, "_mod", Spy())
    world = World({"nodes": 4, "jobs": [(3, 3), (2, 2)], "handler": True,
                   "classes": [{"kind": "bundle", "jobs": [0, 1],
                                "log": [(0, 2), (1, 3)]}]})
    world.apply()
    binds = seen["bind_by_job"]
    assert sorted(len(v) for v in binds.values()) == [2, 3]
    assert all(not gc.is_tracked(v) for v in binds.values())
    # the per-piece slices appended to the nodes' batches are untracked too
    batches = [b for ni in world.cache.nodes_sorted for b in ni._batches]
    assert batches and all(not gc.is_tracked(b) for b in batches)
    fired = [ev for ev in seen["events"] if ev[0] == "f"]
    assert fired
    for ev in fired:                   # plugin code may keep these
        assert all(gc.is_tracked(arg) for arg in ev[2:5])
