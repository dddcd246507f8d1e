"""One cycle through the HIP decision plane with the host-native per-job
loops on and off: same placements and phases, and the loops are really
the native ones."""

import pytest

from volcano_amd.ops import host

pytestmark = pytest.mark.gpu


def _cycle():
    from volcano_amd.scheduler import (FakeBinder, Scheduler, SchedulerCache,
                                       default_config)
    from volcano_amd.store import ObjectStore
    from volcano_amd.utils import synth

    store = ObjectStore()
    for n in synth.make_nodes(64, cpu_milli=32000, mem=64 * 1024 ** 3):
        store.create("Node", n)
    store.create("Queue", synth.make_queue("default"))
    for j in range(8):
        synth.make_gang(store, f"gang-{j}", replicas=8, cpu_milli=1000,
                        mem=1024 ** 3)
    config = default_config()
    config.use_hip = True
    config.device = "cuda"
    binder = FakeBinder()
    cache = SchedulerCache(store=store, binder=binder, device="cuda")
    Scheduler(cache, config).run_once()
    tasks = {t.key: (t.node_name, int(t.status))
             for job in cache.jobs.values() for t in job.tasks.values()}
    nodes = {ni.name: sorted(ni.tasks) for ni in cache.nodes.values()}
    phases = {k: job.phase for k, job in cache.jobs.items()}
    jt = cache.job_table
    table = [c.tolist() for c in (jt.occ, jt.npend, jt.nfailed, jt.phase)]
    return dict(binder.binds), tasks, nodes, phases, table


def test_native_jobs_match_python_loops_on_hip_plane(monkeypatch):
    monkeypatch.setenv("VAMD_NATIVE_JOBS", "1")
    assert host.native_jobs_enabled()
    native = _cycle()
    monkeypatch.setenv("VAMD_NATIVE_JOBS", "0")
    assert not host.native_jobs_enabled()
    oracle = _cycle()
    assert len(native[0]) == 64
    assert set(native[3].values()) == {"Running"}
    assert native == oracle
