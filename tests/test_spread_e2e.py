"""Exact topology spread (``topologyspread`` with ``exact: true``) through the
scheduler on the torch runner: maxSkew holds per placement inside one
allocate cycle, across jobs of a group, and across a gang revert."""

from collections import Counter

import pytest

from volcano_amd.scheduler import (FakeBinder, Scheduler, SchedulerCache,
                                   default_config)
from volcano_amd.scheduler.config import PluginOption, Tier
from volcano_amd.store import ObjectStore
from volcano_amd.utils import synth

GI = 1024 ** 3


def mk(exact):
    store = ObjectStore()
    binder = FakeBinder()
    cache = SchedulerCache(store=store, binder=binder)
    config = default_config()
    args = {} if exact is None else {"exact": exact}
    config.tiers = [
        Tier(plugins=[PluginOption(n)
                      for n in ("priority", "gang", "conformance")]),
        Tier(plugins=[PluginOption(n) for n in (
            "overcommit", "drf", "predicates", "nodeorder", "binpack")]
            + [PluginOption("topologyspread", arguments=args)])]
    return store, binder, Scheduler(cache, config)


def inventory(store, sizes):
    """sizes: {node: (zone or None, cpu_milli)} -> {node: zone}."""
    zones = {}
    for name, (zone, cpu) in sizes.items():
        labels = {"zone": zone} if zone is not None else {}
        store.create("Node", synth.make_node(name, cpu_milli=cpu,
                                             mem=256 * GI, labels=labels))
        zones[name] = zone
    store.create("Queue", synth.make_queue("default"))
    return zones


# one node far larger than the rest: the least-requested score prefers it
# for every replica, so scoring alone piles the whole job into zone a
UNEVEN = {"big-a": ("a", 64000), "small-b": ("b", 8000),
          "small-c": ("c", 8000)}


def spread_job(store, name, replicas, min_member, *, group="web", skew=1,
               priority=0, cpu=500):
    store.create("PodGroup", synth.make_podgroup(name, min_member=min_member))
    for i in range(replicas):
        p = synth.make_pod(f"{name}-w-{i}", name, cpu_milli=cpu, mem=GI,
                           role="w", priority=priority)
        p.affinity = {"topologySpread": {"group": group,
                                         "topologyKey": "zone",
                                         "maxSkew": skew}}
        store.create("Pod", p)


def zone_counts(binder, zones, prefix=""):
    c = Counter({z: 0 for z in zones.values() if z is not None})
    for key, node in binder.binds.items():
        if key.startswith(f"default/{prefix}"):
            c[zones[node]] += 1
    return c


def test_seven_replicas_one_cycle():
    store, binder, sched = mk(exact=True)
    zones = inventory(store, UNEVEN)
    spread_job(store, "web", 7, 1)
    sched.run_once()
    c = zone_counts(binder, zones)
    assert sorted(c.values()) == [2, 2, 3], c


@pytest.mark.parametrize("exact", [None, False, "false"])
def test_control_without_exact_overshoots(exact):
    """The same inventory without ``exact``: the cycle-granular bit cannot
    hold the bound inside one class — this is what the feature fixes, and
    what shows the inventory discriminates."""
    store, binder, sched = mk(exact=exact)
    zones = inventory(store, UNEVEN)
    spread_job(store, "web", 7, 1)
    sched.run_once()
    c = zone_counts(binder, zones)
    assert sum(c.values()) == 7
    assert max(c.values()) - min(c.values()) > 1, c


def test_two_jobs_share_one_group():
    store, binder, sched = mk(exact="true")
    zones = inventory(store, UNEVEN)
    spread_job(store, "web-a", 4, 1)
    spread_job(store, "web-b", 3, 1)
    sched.run_once()
    assert sum(zone_counts(binder, zones, "web-a").values()) == 4
    assert sum(zone_counts(binder, zones, "web-b").values()) == 3
    c = zone_counts(binder, zones)
    assert sorted(c.values()) == [2, 2, 3], c


def test_gang_revert_restores_the_group_counts():
    """Zone c has no node the pods fit on, so with maxSkew 1 only two
    replicas can ever be placed (one in a, one in b).  The gang of 3
    reverts; the next job of the same group must then find the counts it
    would have found alone — with the gang's two placements still counted
    it could place nothing."""
    store, binder, sched = mk(exact=True)
    sizes = dict(UNEVEN)
    sizes["small-c"] = ("c", 100)
    zones = inventory(store, sizes)
    spread_job(store, "gang", 3, 3, priority=10)
    spread_job(store, "later", 2, 1, priority=0)
    sched.run_once()
    assert not any(k.startswith("default/gang") for k in binder.binds)
    c = zone_counts(binder, zones, "later")
    assert (c["a"], c["b"], c["c"]) == (1, 1, 0), c


def test_blocked_domain_stops_the_class():
    store, binder, sched = mk(exact=True)
    sizes = dict(UNEVEN)
    sizes["small-c"] = ("c", 100)
    zones = inventory(store, sizes)
    spread_job(store, "web", 7, 1)
    sched.run_once()
    c = zone_counts(binder, zones)
    assert (c["a"], c["b"], c["c"]) == (1, 1, 0), c


def test_unlabeled_nodes_stay_out():
    store, binder, sched = mk(exact=True)
    sizes = dict(UNEVEN)
    sizes["huge-nolabel"] = (None, 256000)
    zones = inventory(store, sizes)
    spread_job(store, "web", 6, 1)
    sched.run_once()
    assert "huge-nolabel" not in binder.binds.values()
    assert sorted(zone_counts(binder, zones).values()) == [2, 2, 2]


def test_saturated_zone_reopens_within_the_cycle():
    """Cycle 1 puts one pod into zone a.  At the next session open a is
    saturated (1 >= 0 + 1); the cycle-granular bit would keep it shut for
    the whole cycle, the exact path reopens it once b and c have caught
    up: 5 more replicas end at 2/2/2."""
    store, binder, sched = mk(exact=True)
    zones = inventory(store, UNEVEN)
    spread_job(store, "first", 1, 1)
    sched.run_once()
    assert zone_counts(binder, zones)["a"] == 1
    spread_job(store, "rest", 5, 1)
    sched.run_once()
    c = zone_counts(binder, zones)
    assert sorted(c.values()) == [2, 2, 2], c


def test_max_skew_two():
    store, binder, sched = mk(exact=True)
    zones = inventory(store, UNEVEN)
    spread_job(store, "web", 8, 1, skew=2)
    sched.run_once()
    c = zone_counts(binder, zones)
    assert sum(c.values()) == 8
    assert max(c.values()) - min(c.values()) <= 2
    # the big node still wins whenever its zone is eligible
    assert c["a"] == max(c.values())


@pytest.mark.parametrize("exact", [True, False])
def test_one_pod_per_cycle_alternates(exact):
    """The scenario of test_plugins_policy.test_topology_spread_across_zones
    gives the same 2/2 with and without ``exact``."""
    store, binder, sched = mk(exact=exact)
    zones = {}
    for i, zone in enumerate(["z1", "z1", "z2", "z2"]):
        store.create("Node", synth.make_node(
            f"n{i}", cpu_milli=8000, mem=32 * GI, labels={"zone": zone}))
        zones[f"n{i}"] = zone
    store.create("Queue", synth.make_queue("default"))
    placed = []
    for i in range(4):
        spread_job(store, f"sp{i}", 1, 1)
        sched.run_once()
        node = binder.binds.get(f"default/sp{i}-w-0")
        assert node is not None
        placed.append(zones[node])
    assert placed.count("z1") == 2 and placed.count("z2") == 2


def _plans_of(sched):
    """Run one cycle, returning the plans the torch runner was given."""
    from volcano_amd.scheduler import plan as planmod
    import volcano_amd.scheduler.actions.allocate as alloc
    seen = []
    real = planmod.run_plan_torch

    def spy(plan):
        seen.append(plan)
        return real(plan)

    orig = alloc.run_plan_torch
    alloc.run_plan_torch = spy
    try:
        sched.run_once()
    finally:
        alloc.run_plan_torch = orig
    return seen


def test_subgroup_policy_jobs_stay_cycle_granular():
    """Out of scope by design: a SubGroupPolicy job can lose placements
    after the select has counted them, so ``exact`` is ignored for it."""
    store, binder, sched = mk(exact=True)
    inventory(store, UNEVEN)
    pg = synth.make_podgroup("sg", min_member=1)
    pg.spec.sub_group_policy = [{"subGroupSize": 2, "minSubGroups": 0}]
    store.create("PodGroup", pg)
    for i in range(4):
        p = synth.make_pod(f"sg-w-{i}", "sg", cpu_milli=500, mem=GI,
                           role="w")
        p.affinity = {"topologySpread": {"group": "web",
                                         "topologyKey": "zone",
                                         "maxSkew": 1}}
        store.create("Pod", p)
    plans = _plans_of(sched)
    assert plans and plans[0].classes
    assert all(cp.spread is None for cp in plans[0].classes)
    assert plans[0].spread_groups == []
    assert len(binder.binds) == 4


def test_soft_shard_coordinator_stays_cycle_granular():
    """Under a coordinator the conflict reconcile may drop placements:
    the plan builder does not route through the exact select."""
    import torch

    class Coordinator:
        def stagger_bias(self, nt):
            return torch.zeros(nt.n, dtype=torch.float32)

        def find_conflicts(self, nt, used_before):
            return frozenset()

        def finalize(self, ssn, nt, used_before):
            pass

    store, binder, sched = mk(exact=True)
    inventory(store, UNEVEN)
    for action in sched._actions:
        if action.name == "allocate":
            action.coordinator = Coordinator()
    spread_job(store, "web", 7, 1)
    plans = _plans_of(sched)
    assert plans and all(cp.spread is None for cp in plans[0].classes)
    assert len(binder.binds) == 7


def test_exact_classes_carry_a_spread_descriptor():
    """Plan-level view: the class is routed (descriptor set, never bundled)
    and has lost the saturation bit but kept the unlabeled one."""
    store, binder, sched = mk(exact=True)
    sizes = dict(UNEVEN)
    sizes["nolabel"] = (None, 8000)
    inventory(store, sizes)
    spread_job(store, "first", 1, 1)
    sched.run_once()                       # zone a now saturated at open
    spread_job(store, "web-a", 2, 1)
    spread_job(store, "web-b", 2, 1)       # same signature: would bundle
    plan = _plans_of(sched)[0]
    assert len(plan.classes) == 2 and len(plan.spread_groups) == 1
    g = plan.spread_groups[0]
    assert g.count.tolist() == [1, 0, 0]
    assert sorted(g.dom_of.tolist()) == [-1, 0, 1, 2]
    for cp in plan.classes:
        assert cp.spread == (0, 1) and cp.bundle is None
    # constraint words: exactly one forbid bit left (the unlabeled set),
    # while the cycle-granular consumers still get both
    bits = sum(bin(int(w) & (2 ** 64 - 1)).count("1")
               for w in plan.classes[0].forbid)
    assert bits == 1
    assert len(binder.binds) == 5
