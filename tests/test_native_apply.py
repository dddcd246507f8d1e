"""Differential test of the host-native apply walk against the Python walk.

Each case builds two identical, independent worlds from one spec (store →
cache → open session → hand-built ``CyclePlan`` / ``CycleResult`` arrays),
runs ``AllocateAction._apply`` once with the native walk and once with
``VAMD_NATIVE_APPLY=0``, and compares every piece of state the apply
touches.  The worlds are rebuilt from the spec rather than deep-copied:
sessions hold plugin closures and tensors that ``copy.deepcopy`` does not
separate, and a rebuild from the same seed is the same state.
"""

import random

import numpy as np
import pytest
import torch

from volcano_amd.api.info import TaskClass
from volcano_amd.api.types import TaskStatus
from volcano_amd.ops import host
from volcano_amd.scheduler import (FakeBinder, Scheduler, SchedulerCache,
                                   default_config)
from volcano_amd.scheduler.actions.allocate import AllocateAction
from volcano_amd.scheduler.plan import (BundleEntry, ClassPlan, CyclePlan,
                                        CycleResult, JobPlan)
from volcano_amd.store import ObjectStore
from volcano_amd.utils import synth

# -- spec -------------------------------------------------------------------
# {"nodes": N,
#  "jobs": [(ntasks, min_member), ...],
#  "classes": [{"kind": "bundle", "jobs": [j, ...], "log": [(nid, cnt), ...],
#               "flag": 1, "len": None, "lookup": set_of_j_without_job_ref},
#              {"kind": "plain", "job": j, "take": k, "alias": bool, ...}],
#  "bad": [nid, ...], "handler": bool}

class Recorder:
    def __init__(self):
        self.calls = []

    def on_allocate(self, tclass, node_ids, counts, tasks):
        self.calls.append((tclass.tasks[0].key if tclass.tasks else None,
                           list(node_ids), list(counts),
                           [t.key for t in tasks]))


class World:
    def __init__(self, spec):
        self.spec = spec
        store = ObjectStore()
        for n in synth.make_nodes(spec["nodes"], cpu_milli=64000,
                                  mem=256 * 1024 ** 3):
            store.create("Node", n)
        store.create("Queue", synth.make_queue("default"))
        for j, (ntasks, min_member) in enumerate(spec["jobs"]):
            synth.make_gang(store, f"job-{j:03d}", replicas=ntasks,
                            cpu_milli=1000, mem=1024 ** 3,
                            min_member=min_member)
        self.binder = FakeBinder()
        self.cache = SchedulerCache(store=store, binder=self.binder,
                                    device="cpu")
        self.sched = Scheduler(self.cache, default_config())
        self.ssn = ssn = self.sched.open_session()
        self.recorder = None
        if spec.get("handler"):
            self.recorder = Recorder()
            ssn.event_handlers.append(self.recorder)
        nt = ssn.node_tensors
        Q = max(len(ssn.queue_index), 1)
        self.qi = qi = ssn.queue_index.get("default", 0)
        self.plan = plan = CyclePlan(
            nt, torch.full((Q, nt.r), 1.0e18, dtype=torch.float32),
            torch.zeros((Q, nt.r), dtype=torch.float32))
        jobs = [ssn.jobs[f"default/job-{j:03d}"]
                for j in range(len(spec["jobs"]))]
        self.jobs = jobs
        W = max(nt.labels.words, 1)
        zeros = np.zeros(W, dtype=np.int64)
        logs = []
        for ci, cs in enumerate(spec["classes"]):
            if cs["kind"] == "bundle":
                members = [jobs[j] for j in cs["jobs"]]
                entries = []
                for j, jb in zip(cs["jobs"], members):
                    tasks = list(jb.task_status_index[
                        TaskStatus.PENDING].values())
                    entries.append(BundleEntry(
                        jb.key, tasks, len(tasks), jb.min_available,
                        None if j in cs.get("lookup", ()) else jb))
                first = entries[0].tasks[0]
                tc = TaskClass(signature=first.class_signature(),
                               role=first.role, request=first.request,
                               tasks=entries[0].tasks,
                               priority=first.priority)
                cp = ClassPlan(tclass=tc, job_key=entries[0].job_key,
                               queue_idx=qi, req=nt.req_vector(first),
                               tolerated=-1, require=zeros, forbid=zeros,
                               min_needed=min(e.min_needed for e in entries))
                cp.ntasks_override = sum(e.ntasks for e in entries)
                cp.bundle = entries
                key = entries[0].job_key
            else:
                jb = jobs[cs["job"]]
                tasks = list(jb.task_status_index[
                    TaskStatus.PENDING].values())[
                        cs.get("from", 0):cs.get("from", 0) + cs["take"]]
                first = tasks[0]
                tc = TaskClass(signature=first.class_signature(),
                               role=first.role, request=first.request,
                               tasks=tasks, priority=first.priority)
                key = jb.key
                if cs.get("alias"):
                    key = f"{jb.key}#sg0:{ci}"
                    if not hasattr(plan, "job_alias"):
                        plan.job_alias = {}
                    plan.job_alias[key] = jb.key
                cp = ClassPlan(tclass=tc, job_key=key, queue_idx=qi,
                               req=nt.req_vector(first), tolerated=-1,
                               require=zeros, forbid=zeros, min_needed=1)
            plan.jobs.append(JobPlan(job_key=key, class_begin=len(plan.classes),
                                     class_end=len(plan.classes) + 1,
                                     occupied=0, min_available=1))
            plan.classes.append(cp)
            logs.append(list(cs["log"]))
        plan.finalize()
        # hand-built logs decide the slot layout (zero-count entries make
        # a log longer than the planner's own cap)
        off = 0
        ln, lc, ll, jf = [], [], [], []
        for cp, cs, log in zip(plan.classes, spec["classes"], logs):
            cp.log_off = off
            cp.log_cap = max(1, len(log))
            pad = cp.log_cap - len(log)
            ln += [n for n, _ in log] + [0] * pad
            lc += [c for _, c in log] + [0] * pad
            ll.append(len(log) if cs.get("len") is None else cs["len"])
            jf.append(cs.get("flag", 1))
            off += cp.log_cap
        plan.log_total = off
        C = len(plan.classes)
        self.result = CycleResult(
            plan, np.asarray(ln, dtype=np.int32), np.asarray(lc, dtype=np.int32),
            np.asarray(ll, dtype=np.int32), np.zeros(C, dtype=np.int32),
            np.zeros(C, dtype=np.int32), np.asarray(jf, dtype=np.uint8))
        # stage what the decision plane would have left on the device
        for c, cp in enumerate(plan.classes):
            if not jf[c]:
                continue
            req = torch.from_numpy(cp.req)
            for e in range(cp.log_off, cp.log_off + ll[c]):
                if lc[e] > 0:
                    nt.used_t[:, ln[e]] += req * float(lc[e])
                    plan.queue_alloc[qi] += req * float(lc[e])

    def apply(self):
        self.action = AllocateAction()
        self.action._apply(self.ssn, self.plan, self.result,
                           bad_nodes=frozenset(self.spec.get("bad", ())))

    def state(self):
        ssn = self.ssn
        tasks = {}
        jobs = {}
        for key, job in ssn.jobs.items():
            for t in job.tasks.values():
                tasks[t.key] = (t.node_name, int(t.status))
            jobs[key] = (
                {int(s): list(b) for s, b in job.task_status_index.items()
                 if b},
                job.occupied_count, job.phase)
        nodes = {}
        for ni in self.cache.nodes_sorted:
            nodes[ni.name] = (list(ni.tasks), sorted(ni.used.q.items()))
        return {
            "tasks": tasks, "jobs": jobs, "nodes": nodes,
            "binds": list(self.binder.binds.items()),
            "bound_count": self.binder.bound_count,
            "used_t": ssn.node_tensors.used_t.cpu().numpy().copy(),
            "queue_alloc": self.plan.queue_alloc.cpu().numpy().copy(),
            "events": self.recorder.calls if self.recorder else None,
        }


def run_both(spec, monkeypatch):
    monkeypatch.setenv("VAMD_NATIVE_APPLY", "1")
    native = World(spec)
    native.apply()
    assert getattr(native.action, "last_walk_stats", None) is not None, \
        "native walk did not run"
    monkeypatch.setenv("VAMD_NATIVE_APPLY", "0")
    oracle = World(spec)
    oracle.apply()
    assert getattr(oracle.action, "last_walk_stats", None) is None
    a, b = native.state(), oracle.state()
    for k in ("tasks", "jobs", "nodes", "binds", "bound_count", "events"):
        assert a[k] == b[k], k
    for k in ("used_t", "queue_alloc"):
        assert np.array_equal(a[k], b[k]), k
    return native, a


def n_bound(state):
    return sum(1 for _, st in state["tasks"].values()
               if st == int(TaskStatus.BOUND))


# -- fixed cases --------------------------------------------------------------

def test_gang_miss_then_smaller_entry_places_from_recycled_slots(monkeypatch):
    # 3 slots: job 0 (4 tasks, gang 4) misses, job 1 (3 tasks) takes them
    spec = {"nodes": 8, "jobs": [(4, 4), (3, 3)],
            "classes": [{"kind": "bundle", "jobs": [0, 1],
                         "log": [(2, 2), (5, 1)]}]}
    w, st = run_both(spec, monkeypatch)
    assert w.action.last_walk_stats == (1, 1, 0, 0)
    assert n_bound(st) == 3
    assert st["jobs"]["default/job-000"][1] == 0
    assert st["jobs"]["default/job-001"][1] == 3
    assert st["jobs"]["default/job-001"][2] == "Running"


def test_unclaimed_tail_begins_mid_entry(monkeypatch):
    # job 0 takes 2 of the first entry's 5; the rest reverts: (1,3),(4,2)
    spec = {"nodes": 8, "jobs": [(2, 2)],
            "classes": [{"kind": "bundle", "jobs": [0],
                         "log": [(1, 5), (4, 2)]}]}
    w, st = run_both(spec, monkeypatch)
    assert w.action.last_walk_stats == (1, 0, 0, 2)
    assert n_bound(st) == 2
    req = w.plan.classes[0].req
    # staged 7, kept 2
    assert np.allclose(st["queue_alloc"][w.qi], 2 * req)


def test_zero_count_entries_in_bundle_and_plain(monkeypatch):
    spec = {"nodes": 8, "jobs": [(3, 3), (2, 1), (3, 1)],
            "classes": [{"kind": "bundle", "jobs": [0, 1],
                         "log": [(0, 1), (3, 0), (6, 2), (7, 0), (1, 2)]},
                        {"kind": "plain", "job": 2, "take": 3,
                         "log": [(2, 0), (5, 2), (6, 0), (0, 1)]}]}
    w, st = run_both(spec, monkeypatch)
    assert n_bound(st) == 8
    assert w.action.last_walk_stats[:3] == (3, 0, 0)


def test_lost_node_hits_bundle_entry(monkeypatch):
    # job 0 lands on nodes 1,2 (2 is lost) → reverted; job 1 commits on 3
    spec = {"nodes": 8, "jobs": [(3, 3), (2, 2)], "bad": [2],
            "classes": [{"kind": "bundle", "jobs": [0, 1],
                         "log": [(1, 2), (2, 1), (3, 2)]}]}
    w, st = run_both(spec, monkeypatch)
    assert w.action.last_walk_stats == (1, 0, 1, 0)
    assert n_bound(st) == 2
    assert st["jobs"]["default/job-000"][1] == 0


def test_lost_node_hits_plain_class(monkeypatch):
    spec = {"nodes": 8, "jobs": [(4, 1), (2, 1)], "bad": [6],
            "classes": [{"kind": "plain", "job": 0, "take": 4,
                         "log": [(1, 2), (6, 2)]},
                        {"kind": "plain", "job": 1, "take": 2,
                         "log": [(0, 2)]}]}
    w, st = run_both(spec, monkeypatch)
    assert w.action.last_walk_stats == (1, 0, 1, 0)
    assert n_bound(st) == 2
    assert np.allclose(st["queue_alloc"][w.qi], 2 * w.plan.classes[0].req)


def test_flag_zero_and_empty_log_classes_are_skipped(monkeypatch):
    spec = {"nodes": 8, "jobs": [(2, 2), (2, 2), (2, 2)],
            "classes": [{"kind": "bundle", "jobs": [0], "flag": 0,
                         "log": [(1, 2)]},
                        {"kind": "plain", "job": 1, "take": 2, "len": 0,
                         "log": [(2, 2)]},
                        {"kind": "bundle", "jobs": [2],
                         "log": [(3, 2)]}]}
    w, st = run_both(spec, monkeypatch)
    assert w.action.last_walk_stats == (1, 0, 0, 0)
    assert n_bound(st) == 2
    assert st["jobs"]["default/job-002"][1] == 2


def test_class_reached_through_job_alias(monkeypatch):
    # two subgroup classes of one real job, keyed by synthetic names
    spec = {"nodes": 8, "jobs": [(6, 2)],
            "classes": [{"kind": "plain", "job": 0, "take": 2,
                         "alias": True, "log": [(4, 2)]},
                        {"kind": "plain", "job": 0, "take": 1, "from": 2,
                         "alias": True, "log": [(5, 1)]}]}
    w, st = run_both(spec, monkeypatch)
    assert st["jobs"]["default/job-000"][2] == "Running"
    assert w.action.last_walk_stats[0] == 2


def test_event_handler_receives_the_same_arguments(monkeypatch):
    spec = {"nodes": 8, "jobs": [(3, 3), (4, 2), (2, 2), (3, 1)],
            "handler": True, "bad": [7],
            "classes": [{"kind": "bundle", "jobs": [0, 1, 2],
                         "lookup": {1},
                         "log": [(0, 2), (1, 0), (2, 3), (3, 1), (7, 2),
                                 (4, 1)]},
                        {"kind": "plain", "job": 3, "take": 3,
                         "log": [(5, 1), (6, 2)]}]}
    w, st = run_both(spec, monkeypatch)
    assert st["events"], "handler saw no allocation"
    assert sum(len(ev[3]) for ev in st["events"]) == n_bound(st)
    for _, nids, cnts, keys in st["events"]:
        assert len(nids) == len(cnts)
        assert sum(cnts) == len(keys)


# -- seeded sweep ---------------------------------------------------------------

def random_spec(rng):
    n_nodes = rng.randint(8, 64)
    n_jobs = rng.randint(2, 40)
    jobs = []
    for _ in range(n_jobs):
        nt = rng.randint(1, 6)
        jobs.append((nt, rng.randint(1, nt)))
    classes = []
    j = 0
    while j < n_jobs:
        flag = 0 if rng.random() < 0.1 else 1
        if rng.random() < 0.3:
            nt = jobs[j][0]
            take = rng.randint(1, nt)
            left, log = take, []
            while left > 0 and rng.random() < 0.9:
                if rng.random() < 0.15:
                    log.append((rng.randrange(n_nodes), 0))
                    continue
                c = rng.randint(1, left)
                log.append((rng.randrange(n_nodes), c))
                left -= c
            cs = {"kind": "plain", "job": j, "take": take, "log": log,
                  "alias": rng.random() < 0.3, "flag": flag}
            j += 1
        else:
            k = min(rng.randint(1, 8), n_jobs - j)
            members = list(range(j, j + k))
            total = sum(jobs[m][0] for m in members)
            # under-, exactly- or over-provisioned placement stream
            slots = max(0, int(total * rng.choice((0.3, 0.7, 1.0, 1.4))))
            log = []
            while slots > 0:
                if rng.random() < 0.15:
                    log.append((rng.randrange(n_nodes), 0))
                    continue
                c = rng.randint(1, min(5, slots))
                log.append((rng.randrange(n_nodes), c))
                slots -= c
            cs = {"kind": "bundle", "jobs": members, "log": log, "flag": flag,
                  "lookup": {m for m in members if rng.random() < 0.3}}
            j += k
        if rng.random() < 0.05:
            cs["len"] = 0
        classes.append(cs)
    bad = [rng.randrange(n_nodes) for _ in range(rng.choice((0, 0, 1, 3)))]
    return {"nodes": n_nodes, "jobs": jobs, "classes": classes, "bad": bad,
            "handler": rng.random() < 0.3}


SWEEP_SEEDS = list(range(20))


def test_seeded_random_sweep(monkeypatch):
    committed = missed = lost = 0
    tails = 0
    for seed in SWEEP_SEEDS:
        spec = random_spec(random.Random(seed))
        w, _ = run_both(spec, monkeypatch)
        c, m, l, t = w.action.last_walk_stats
        committed += c
        missed += m
        lost += l
        tails += 1 if t else 0
    assert committed > 0
    assert missed > 0
    assert lost > 0
    assert tails > 0


# -- fallback and predicate --------------------------------------------------

def test_switch_forces_the_python_walk(monkeypatch):
    monkeypatch.setenv("VAMD_NATIVE_APPLY", "0")
    assert host.native_apply_loaded()
    assert not host.native_apply_enabled()
    monkeypatch.setenv("VAMD_NATIVE_APPLY", "1")
    assert host.native_apply_enabled()


def test_negative_count_raises(monkeypatch):
    monkeypatch.setenv("VAMD_NATIVE_APPLY", "1")
    spec = {"nodes": 8, "jobs": [(2, 2)],
            "classes": [{"kind": "bundle", "jobs": [0],
                         "log": [(1, -1), (2, 2)]}]}
    w = World(spec)
    with pytest.raises(ValueError):
        w.apply()
    assert all(t.status == TaskStatus.PENDING
               for t in w.jobs[0].tasks.values())
