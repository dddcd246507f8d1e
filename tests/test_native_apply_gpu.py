"""One cycle through the HIP decision plane with the host-native apply
walk on and off: same placements, and the extension is really loaded."""

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
    return dict(binder.binds), tasks, nodes, phases


def test_native_apply_matches_python_walk_on_hip_plane(monkeypatch):
    assert host.native_apply_loaded()
    monkeypatch.setenv("VAMD_NATIVE_APPLY", "1")
    native = _cycle()
    monkeypatch.setenv("VAMD_NATIVE_APPLY", "0")
    oracle = _cycle()
    assert len(native[0]) == 64
    assert native == oracle
