"""The block lookahead of the host-native per-job loops changes no result.

Every loop runs with ``VAMD_HOST_PREFETCH`` on and off and against its
Python oracle, at job counts around the block size B (0, 1, B-1, B, B+1,
2B+1) and with the elements the lookahead has to skip placed inside and at
the edges of a block.  Reference counts and a whole cycle over several
blocks are compared the same way."""

import collections
import collections.abc
import sys

import numpy as np
import pytest

import test_native_jobs as tnj
from test_native_apply import World, run_both
from test_native_jobs import INQ, RUN, B as BOUND, F, P, mk_job, table_of
from volcano_amd.api.info import JobInfo
from volcano_amd.api.objects import PodGroup
from volcano_amd.ops import host
from volcano_amd.scheduler.actions.allocate import AllocateAction
from volcano_amd.scheduler.plan import BundleEntry
from volcano_amd.utils import synth

BLK = host.load().PREFETCH_BLOCK
SIZES = [0, 1, BLK - 1, BLK, BLK + 1, 2 * BLK + 1]
MODES = ("1", "0")                     # lookahead on, off


@pytest.fixture(autouse=True)
def _native_on(monkeypatch):
    monkeypatch.setenv("VAMD_NATIVE_JOBS", "1")
    monkeypatch.setenv("VAMD_NATIVE_APPLY", "1")
    monkeypatch.delenv("VAMD_HOST_PREFETCH_BLOCK", raising=False)
    assert host.native_jobs_enabled()
    assert BLK == 64


def in_modes(monkeypatch, fn):
    """fn() once per mode, each on whatever fresh state fn builds."""
    out = []
    for mode in MODES:
        monkeypatch.setenv("VAMD_HOST_PREFETCH", mode)
        out.append(fn())
    return out


def job_state(job):
    pg = job.podgroup
    return (job.key, None if pg is None else pg.status.phase,
            {int(s): list(b) for s, b in job.task_status_index.items()},
            job._occ, job._tver, job._alloc_vec,
            [(t.key, t.node_name, int(t.status)) for t in job.tasks.values()])


SHAPES = [([P], INQ), ([P, P], "Pending"), ([P, P, P], INQ), ([BOUND, P], RUN),
          ([F, P, P], RUN), ([P, BOUND, BOUND], "Completed")]


def inventory(J, tag="j"):
    """J jobs of 1-3 tasks, every one with a non-empty pending bucket."""
    return [mk_job(f"{tag}{k:03d}", *SHAPES[k % len(SHAPES)])
            for k in range(J)]


def columns(jt):
    return [c.tolist() for c in (jt.occ, jt.npend, jt.nfailed, jt.phase)]


def phase_py(jobs, phase):
    changed = []
    for job in jobs:
        pg = job.podgroup
        if pg is not None and pg.status.phase != phase:
            pg.status.phase = phase
            changed.append(job)
    return changed


# -- block edges --------------------------------------------------------------

@pytest.mark.parametrize("J", SIZES)
def test_scan_block_edges(J, monkeypatch):
    def run():
        jobs = inventory(J)
        if J:
            jobs[-1]._tver += 1        # the last row of the last block
        jt = table_of(jobs)
        if J:
            jt._vers[-1] -= 1
        dirty = jt._scan_native()
        got = columns(jt)
        jt._refresh_dynamic()
        assert got == columns(jt)
        assert dirty == ([J - 1] if J else [])
        return dirty, got
    on, off = in_modes(monkeypatch, run)
    assert on == off


@pytest.mark.parametrize("i", [0, 3, BLK - 1])
@pytest.mark.parametrize("J", SIZES)
def test_entries_block_edges(J, i, monkeypatch):
    def run():
        jobs_l = inventory(i + J + 2)
        gm_l = [1 + k % 3 for k in range(len(jobs_l))]
        entries, total, mn = tnj.entries_both(jobs_l, i, i + J, gm_l)
        assert [e.job for e in entries] == jobs_l[i:i + J]
        return [(e.job_key, [t.key for t in e.tasks], e.ntasks,
                 e.min_needed) for e in entries], total, mn
    on, off = in_modes(monkeypatch, run)
    assert on == off


@pytest.mark.parametrize("J", SIZES)
def test_phase_block_edges(J, monkeypatch):
    def run():
        jobs, ref = inventory(J), inventory(J)
        changed, gated = host.load().set_podgroup_phase(jobs, INQ, True)
        expect = phase_py(ref, INQ)
        assert [j.key for j in changed] == [j.key for j in expect]
        assert gated == []
        assert [job_state(j) for j in jobs] == [job_state(j) for j in ref]
        return [j.key for j in changed], [job_state(j) for j in jobs]
    on, off = in_modes(monkeypatch, run)
    assert on == off


def bind_batches(jobs):
    """by_job for finish_binds: whole pending buckets (the gang case) and,
    for every third job, all but one task; tasks get BOUND first, as the
    walk leaves them."""
    by_job = {}
    for k, job in enumerate(jobs):
        ts = list(job.task_status_index[P].values())
        if k % 3 == 2 and len(ts) > 1:
            ts = ts[:-1]
        for t in ts:
            t.status = BOUND
        by_job[job.key] = ts
    return by_job


@pytest.mark.parametrize("J", SIZES)
def test_finish_binds_block_edges(J, monkeypatch):
    def run():
        jobs, ref = inventory(J), inventory(J)
        table = {j.key: j for j in jobs}
        table["default/absent"] = None
        by_job = bind_batches(jobs)
        host.load().finish_binds(by_job, table, P, BOUND)
        for job, ts in zip(ref, bind_batches(ref).values()):
            job.finish_bind(ts)
        assert [job_state(j) for j in jobs] == [job_state(j) for j in ref]
        return [job_state(j) for j in jobs]
    on, off = in_modes(monkeypatch, run)
    assert on == off


def walk_spec(J, handler=False):
    jobs = [(1 + k % 3, 1 + k % 3) for k in range(J)]
    total = sum(n for n, _ in jobs)
    nodes = max(2, (total + 3) // 4)
    log = [(n, 4) for n in range(nodes)]       # four tasks per node
    return {"nodes": nodes, "jobs": jobs, "handler": handler,
            "classes": [{"kind": "bundle", "jobs": list(range(J)),
                         "log": log}]}


@pytest.mark.parametrize("J", SIZES)
def test_apply_walk_cycle_block_edges(J, monkeypatch):
    if J == 0:      # a plan without classes: the walk itself, called bare
        def run():
            z = np.zeros(0, dtype=np.int32)
            return host.load().apply_walk(
                [], {}, {}, [], np.zeros(0, dtype=np.uint8), z, z, z, z,
                None, BOUND, False)
        on, off = in_modes(monkeypatch, run)
        assert on == off
        assert on[3:8] == ({}, {}, set(), [], (0, 0, 0, 0))
        return

    def run():
        world, state = run_both(walk_spec(J, handler=J == BLK + 1),
                                monkeypatch)
        assert tnj_bound(state) == sum(n for n, _ in world.spec["jobs"])
        return state
    on, off = in_modes(monkeypatch, run)
    for k in ("tasks", "jobs", "nodes", "binds", "bound_count", "events"):
        assert on[k] == off[k], k
    assert np.array_equal(on["used_t"], off["used_t"])


def tnj_bound(state):
    return sum(1 for _, st in state["tasks"].values() if st == int(BOUND))


# -- elements the lookahead must skip -----------------------------------------

class DictSub(dict):
    pass


class Bucket(collections.abc.Mapping):
    """A status bucket that is no dict."""

    def __init__(self, d):
        self._d = dict(d)

    def __getitem__(self, k):
        return self._d[k]

    def __iter__(self):
        return iter(self._d)

    def __len__(self):
        return len(self._d)


class SlottedJob:
    __slots__ = ("key", "podgroup", "tasks", "task_status_index", "_occ",
                 "_tver", "_alloc_vec")

    def __init__(self, src):
        self.key, self.podgroup, self.tasks = src.key, src.podgroup, src.tasks
        self.task_status_index = src.task_status_index
        self._occ, self._tver, self._alloc_vec = src._occ, src._tver, None


class PropertyJob(JobInfo):
    def __init__(self, key, podgroup=None):
        super().__init__(key, None)
        self._pg = podgroup

    @property
    def podgroup(self):
        return self._pg

    @podgroup.setter
    def podgroup(self, v):
        self._pg = v


class ForeignTask:
    """Dict-backed: none of TaskInfo's slots."""

    def __init__(self, key, gated=False):
        self.key, self.gated = key, gated
        self.status, self.node_name = P, ""


def special(kind, k):
    name = f"{kind}{k:03d}"
    if kind == "nopg":
        return mk_job(name, [P, P], podgroup=False)
    if kind == "nobucket":
        job = mk_job(name, [BOUND], phase=RUN)
        assert P not in job.task_status_index
        return job
    if kind == "emptybucket":
        job = mk_job(name, [BOUND, BOUND], phase=RUN)
        job.task_status_index[P] = {}
        return job
    if kind == "gated":
        return mk_job(name, [P, P], gated_first=True)
    if kind == "idxsub":
        job = mk_job(name, [P, P, F])
        job.task_status_index = DictSub(job.task_status_index)
        return job
    if kind == "bucket":
        job = mk_job(name, [P, P, F])
        job.task_status_index[P] = Bucket(job.task_status_index[P])
        return job
    if kind == "slotted":
        return SlottedJob(mk_job(name, [P, P]))
    if kind == "property":
        src = mk_job(name, [P, P, P])
        job = PropertyJob(src.key, src.podgroup)
        for t in src.tasks.values():
            job.add_task(t)
        return job
    if kind == "foreign":
        job = mk_job(name, [P])
        job.task_status_index[P] = {
            f"default/{name}-x{i}": ForeignTask(f"default/{name}-x{i}")
            for i in range(2)}
        return job
    raise AssertionError(kind)


KINDS = ["nopg", "nobucket", "emptybucket", "gated", "idxsub", "bucket",
         "slotted", "property", "foreign"]
# first, inside, last of block 0; first, second, inside of block 1; the
# lone element of block 2
SPOTS = [0, 5, BLK - 1, BLK, BLK + 1, BLK + 9, 2 * BLK]


def spiked(kind):
    jobs = inventory(2 * BLK + 1)
    for k in SPOTS:
        jobs[k] = special(kind, k)
    return jobs


def plain_state(job):
    pg = job.podgroup
    return (job.key, None if pg is None else pg.status.phase, job._occ,
            job._tver,
            {int(s): list(b) for s, b in job.task_status_index.items()})


@pytest.mark.parametrize("kind", KINDS)
def test_skipped_elements_scan_and_phase(kind, monkeypatch):
    def run():
        jobs, ref = spiked(kind), spiked(kind)
        jt = table_of(jobs)
        dirty = jt._scan_native()
        got = columns(jt)
        jt._refresh_dynamic()
        assert got == columns(jt) and dirty == []
        changed, _ = host.load().set_podgroup_phase(jobs, RUN)
        expect = phase_py(ref, RUN)
        assert [j.key for j in changed] == [j.key for j in expect]
        assert [plain_state(j) for j in jobs] == [plain_state(j) for j in ref]
        return got, [j.key for j in changed], [plain_state(j) for j in jobs]
    on, off = in_modes(monkeypatch, run)
    assert on == off


@pytest.mark.parametrize("kind", KINDS)
def test_skipped_elements_entries(kind, monkeypatch):
    def run():
        jobs_l = spiked(kind)
        gm_l = [1 + k % 3 for k in range(len(jobs_l))]
        out = []
        for i, j in ((0, len(jobs_l)), (3, BLK + 3 + 2)):
            nat = host.load().bundle_entries(jobs_l, i, j, gm_l, P,
                                             BundleEntry)
            ref = AllocateAction._run_entries_py(jobs_l, i, j, gm_l, P,
                                                 BundleEntry)
            flat = [[(e.job_key, [t.key for t in e.tasks], e.ntasks,
                      e.min_needed, id(e.job)) for e in r[0]] + list(r[1:])
                    for r in (nat, ref)]
            assert flat[0] == flat[1]
            out.append([x[:4] if isinstance(x, tuple) else x
                        for x in flat[0]])
        return out
    on, off = in_modes(monkeypatch, run)
    assert on == off
    skipped = {"nobucket", "emptybucket", "gated"}
    assert len(on[0]) - 2 == 2 * BLK + 1 - (len(SPOTS) if kind in skipped
                                            else 0)


def test_skipped_foreign_and_subclass_in_finish_binds(monkeypatch):
    def run():
        out = []
        for kind in ("idxsub", "foreign", "property"):
            jobs, ref = spiked(kind), spiked(kind)
            table = {j.key: j for j in jobs}
            host.load().finish_binds(bind_batches(jobs), table, P, BOUND)
            for job, ts in zip(ref, bind_batches(ref).values()):
                job.finish_bind(ts)
            assert [plain_state(j) for j in jobs] == \
                [plain_state(j) for j in ref]
            out.append([plain_state(j) for j in jobs])
        return out
    on, off = in_modes(monkeypatch, run)
    assert on == off


class Boom(Exception):
    pass


class RaisingPG:
    @property
    def status(self):
        raise Boom("status")


@pytest.mark.parametrize("at", [0, 5, BLK - 1, BLK, BLK + 9])
def test_raising_status_propagates(at, monkeypatch):
    def run():
        jobs = inventory(2 * BLK + 1)
        jobs[at].podgroup = RaisingPG()
        with pytest.raises(Boom):
            table_of(jobs)._scan_native()
        with pytest.raises(Boom):
            host.load().set_podgroup_phase(jobs, RUN)
        # stores up to the raising job happened, none after it
        phases = [None if k == at else j.podgroup.status.phase
                  for k, j in enumerate(jobs)]
        fresh = inventory(2 * BLK + 1)
        assert phases[:at] == [RUN] * at
        assert phases[at + 1:] == [j.podgroup.status.phase
                                   for j in fresh[at + 1:]]
        return phases
    on, off = in_modes(monkeypatch, run)
    assert on == off


class ShrinkingPG:
    def __init__(self, jobs):
        self.jobs = jobs
        self.real = PodGroup().status

    @property
    def status(self):
        del self.jobs[-1]
        return self.real


@pytest.mark.parametrize("at", [0, 5, BLK - 1, BLK])
def test_shrinking_job_list_still_raises(at, monkeypatch):
    def run():
        jobs = inventory(2 * BLK + 1)
        jobs[at].podgroup = ShrinkingPG(jobs)
        jt = table_of(jobs)
        with pytest.raises(RuntimeError, match="job list changed size"):
            jt._scan_native()
        assert len(jobs) == 2 * BLK
        # the phase store follows the live length instead
        jobs[at].podgroup = ShrinkingPG(jobs)
        changed, _ = host.load().set_podgroup_phase(jobs, "Unknown")
        assert len(jobs) == 2 * BLK - 1 and len(changed) == len(jobs)
        return [j.key for j in changed]
    on, off = in_modes(monkeypatch, run)
    assert on == off


class Rebinding(str):
    """A phase whose != rebinds the pod group of a later job."""
    hook = None

    def __ne__(self, other):
        if Rebinding.hook is not None:
            hook, Rebinding.hook = Rebinding.hook, None
            hook()
        return str.__ne__(self, other)

    __hash__ = str.__hash__


@pytest.mark.parametrize("at,later", [(0, 1), (3, BLK - 1), (BLK, BLK + 5),
                                      (BLK - 1, BLK)])
def test_rebound_podgroup_is_seen_by_the_later_job(at, later, monkeypatch):
    def run():
        jobs = inventory(2 * BLK + 1)
        jobs[at].podgroup.status.phase = Rebinding("Pending")
        old = jobs[later].podgroup
        old_phase = old.status.phase
        new = PodGroup()
        new.status.phase = "Pending"

        def rebind():
            jobs[later].podgroup = new
        Rebinding.hook = rebind
        changed, _ = host.load().set_podgroup_phase(jobs, RUN)
        assert Rebinding.hook is None
        assert jobs[later].podgroup is new and new.status.phase == RUN
        assert old.status.phase == old_phase       # never touched
        assert jobs[later] in changed
        return [j.key for j in changed]
    on, off = in_modes(monkeypatch, run)
    assert on == off


# -- reference counts ---------------------------------------------------------

def counts(objs):
    return [sys.getrefcount(o) for o in objs]


def sampled(jobs):
    objs = list(jobs)
    for job in jobs:
        objs += list(job.tasks.values())
        objs += list(job.task_status_index.values())
        if job.podgroup is not None:
            objs += [job.podgroup, job.podgroup.status]
    return objs


def test_reference_counts_match_with_lookahead_off(monkeypatch):
    J = 2 * BLK + 1

    def run():
        jobs = inventory(J)
        objs = sampled(jobs) + [P, F, BOUND]
        gm_l = [3000 + k for k in range(J)]    # above the shared small ints
        vers = np.array([j._tver for j in jobs], dtype=np.int64)
        cols = [np.zeros(J, dtype=np.int64) for _ in range(3)] + \
            [np.zeros(J, dtype=np.int8)]
        deltas = []
        before = counts(objs)
        host.load().scan_jobs(jobs, P, F, tnj._PHASE_MAP, tnj.PH_PENDING,
                              tnj.PH_OTHER, vers, *cols)
        deltas.append([a - b for a, b in zip(counts(objs), before)])
        assert not any(deltas[-1])
        out = host.load().bundle_entries(jobs, 1, J, gm_l, P, BundleEntry)
        deltas.append([a - b for a, b in zip(counts(objs), before)])
        assert sum(deltas[-1]) == J - 1 + out[1]   # entry.job, entry.tasks
        del out
        assert counts(objs) == before
        out = host.load().set_podgroup_phase(jobs, "Unknown", True)
        assert len(out[0]) == J
        del out
        deltas.append([a - b for a, b in zip(counts(objs), before)])
        assert not any(deltas[-1])
        table = {j.key: j for j in jobs}
        by_job = bind_batches(jobs)
        # the wholesale move re-homes buckets: sample them again
        objs = list(jobs) + [t for j in jobs for t in j.tasks.values()] + \
            [P, F, BOUND]
        before = counts(objs)
        host.load().finish_binds(by_job, table, P, BOUND)
        deltas.append([a - b for a, b in zip(counts(objs), before)])
        return deltas
    on, off = in_modes(monkeypatch, run)
    assert on == off


def test_apply_walk_reference_counts_match_with_lookahead_off(monkeypatch):
    def run():
        world = World(walk_spec(2 * BLK + 1))
        objs = list(world.cache.nodes_sorted) + world.jobs + \
            [t for j in world.jobs for t in j.tasks.values()] + \
            [e for cp in world.plan.classes for e in cp.bundle] + \
            [e.tasks for cp in world.plan.classes for e in cp.bundle]
        before = counts(objs)
        world.apply()
        assert world.action.last_walk_stats is not None
        return [a - b for a, b in zip(counts(objs), before)]
    on, off = in_modes(monkeypatch, run)
    assert on == off


# -- whole cycle over several blocks ------------------------------------------

def populate_150(store, rng, roomy):
    """About 150 jobs on 40 nodes: 70 identical gangs first (one fused run
    longer than a block), then a seeded mix of whole gangs, gangs too big
    to fit, jobs that may place in part and singles."""
    for n in synth.make_nodes(40, cpu_milli=64000 if roomy else 16000,
                              mem=256 * 1024 ** 3):
        store.create("Node", n)
    store.create("Queue", synth.make_queue("default"))
    store.create("Queue", synth.make_queue("other"))
    for j in range(150):
        shape = "gang4" if j < 70 else rng.choice(
            ["gang4", "gang4", "big", "loose", "loose", "one"])
        queue = "other" if j >= 70 and rng.random() < 0.25 else "default"
        if shape == "gang4":
            synth.make_gang(store, f"job-{j:03d}", replicas=4, queue=queue,
                            cpu_milli=1000, mem=1024 ** 3)
        elif shape == "big":
            synth.make_gang(store, f"job-{j:03d}",
                            replicas=rng.randint(8, 40), queue=queue,
                            cpu_milli=4000, mem=1024 ** 3)
        elif shape == "loose":
            synth.make_gang(store, f"job-{j:03d}", replicas=6, queue=queue,
                            cpu_milli=2000, mem=1024 ** 3, min_member=2)
        else:
            synth.make_gang(store, f"job-{j:03d}", replicas=1, queue=queue,
                            cpu_milli=500, mem=1024 ** 3)


@pytest.mark.parametrize("seed,handler,roomy", [(16, False, False),
                                                (8, True, False),
                                                (9, True, True),
                                                (10, False, True)])
def test_whole_cycle_of_several_blocks(seed, handler, roomy, monkeypatch):
    monkeypatch.setattr(tnj, "populate_random", populate_150)
    calls = tnj.counting_module(monkeypatch)
    monkeypatch.setenv("VAMD_HOST_PREFETCH", "1")
    on = tnj.run_cycle(seed, handler, monkeypatch, roomy)
    assert calls["scan_jobs"] and calls["bundle_entries"] and \
        calls["set_podgroup_phase"] and calls["apply_walk"] and \
        calls["finish_binds"], calls
    monkeypatch.setenv("VAMD_HOST_PREFETCH", "0")
    off = tnj.run_cycle(seed, handler, monkeypatch, roomy)
    monkeypatch.setenv("VAMD_NATIVE_JOBS", "0")
    monkeypatch.setenv("VAMD_NATIVE_APPLY", "0")
    oracle = tnj.run_cycle(seed, handler, monkeypatch, roomy)
    for k in oracle:
        assert on[k] == off[k], k
        assert on[k] == oracle[k], k
    assert len(on["phases"]) == 150
    n_bound = sum(1 for _, st in on["tasks"].values() if st == int(BOUND))
    if roomy:
        assert n_bound == len(on["tasks"])
    else:       # whole gangs, gang misses and partly placed jobs
        assert 280 < n_bound < len(on["tasks"])
        per_job = collections.defaultdict(list)
        for key, (_, st) in on["tasks"].items():
            per_job[key.split("-worker-")[0]].append(st == int(BOUND))
        assert any(all(v) for v in per_job.values())
        assert any(not any(v) for v in per_job.values())
        assert any(any(v) and not all(v) for v in per_job.values())
    if handler:
        assert on["events"]
