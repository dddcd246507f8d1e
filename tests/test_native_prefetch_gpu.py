"""One cycle of 130 gangs on 40 nodes through the HIP decision plane with
the block lookahead of the host-native loops on and off: the same
placements, phases and table columns."""

import pytest

from volcano_amd.ops import host

pytestmark = pytest.mark.gpu


def _cycle():
    from volcano_amd.scheduler import (FakeBinder, Scheduler, SchedulerCache,
                                       default_config)
    from volcano_amd.store import ObjectStore
    from volcano_amd.utils import synth

    store = ObjectStore()
    for n in synth.make_nodes(40, cpu_milli=32000, mem=64 * 1024 ** 3):
        store.create("Node", n)
    store.create("Queue", synth.make_queue("default"))
    for j in range(130):               # two blocks and two jobs
        synth.make_gang(store, f"gang-{j:03d}", replicas=1 + j % 3,
                        cpu_milli=1000, mem=1024 ** 3)
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


def test_lookahead_changes_no_placement_on_hip_plane(monkeypatch):
    monkeypatch.setenv("VAMD_NATIVE_JOBS", "1")
    monkeypatch.setenv("VAMD_NATIVE_APPLY", "1")
    assert host.native_jobs_enabled() and host.native_apply_enabled()
    assert host.load().PREFETCH_BLOCK == 64
    monkeypatch.setenv("VAMD_HOST_PREFETCH", "1")
    on = _cycle()
    monkeypatch.setenv("VAMD_HOST_PREFETCH", "0")
    off = _cycle()
    assert len(on[0]) == sum(1 + j % 3 for j in range(130))
    assert set(on[3].values()) == {"Running"}
    assert on == off
