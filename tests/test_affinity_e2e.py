"""Exact inter-pod affinity (``interpodaffinity`` with ``exact: true``)
through the scheduler on the torch runner: the rule holds per placement
inside one allocate cycle, across jobs of a group and across a gang revert;
``topologyKey`` is honoured on the cycle-granular path too."""

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
            + [PluginOption("interpodaffinity", arguments=args)])]
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


# nine equal nodes of two pods each, zones interleaved in node order: the
# scores tie, the fill walks the nodes in index order and scatters a class
# of six over all three zones
SMALL = {f"n{i}": ("abc"[i % 3], 1000) for i in range(9)}
# one node far larger than the rest, one node per zone
UNEVEN = {"big-a": ("a", 64000), "small-b": ("b", 8000),
          "small-c": ("c", 8000)}
# a second node in zone a (and in zone b): the hostname unit dim alone lets
# two members into one zone, so only the keyed rule keeps them apart
ANTI4 = dict(UNEVEN, **{"big-a2": ("a", 64000)})
ANTI5 = dict(ANTI4, **{"small-b2": ("b", 8000)})
# nine equal nodes of four pods each: two jobs of two scatter over two nodes
FOUR = {f"n{i}": ("abc"[i % 3], 2000) for i in range(9)}
# ... of three pods each: a class of four spills onto a second node
THREE = {f"n{i}": ("abc"[i % 3], 1500) for i in range(9)}


def job(store, name, replicas, min_member, *, kind="podAffinity",
        group="web", key="zone", priority=0, cpu=500, extra=None):
    store.create("PodGroup", synth.make_podgroup(name, min_member=min_member))
    for i in range(replicas):
        p = synth.make_pod(f"{name}-w-{i}", name, cpu_milli=cpu, mem=GI,
                           role="w", priority=priority)
        spec = {"group": group}
        if key is not None:
            spec["topologyKey"] = key
        p.affinity = {kind: spec}
        if extra:
            p.affinity.update(extra)
        store.create("Pod", p)


def zone_counts(binder, zones, prefix=""):
    c = Counter()
    for key, node in binder.binds.items():
        if key.startswith(f"default/{prefix}"):
            c[zones[node]] += 1
    return c


def node_counts(binder, prefix=""):
    return Counter(node for key, node in binder.binds.items()
                   if key.startswith(f"default/{prefix}"))


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


def best_zone(store_sizes):
    """Zone of the node a single unconstrained pod lands on."""
    store, binder, sched = mk(exact=None)
    zones = inventory(store, store_sizes)
    store.create("PodGroup", synth.make_podgroup("probe", min_member=1))
    store.create("Pod", synth.make_pod("probe-w-0", "probe", cpu_milli=500,
                                       mem=GI, role="w"))
    sched.run_once()
    return zones[binder.binds["default/probe-w-0"]]


def test_six_zone_affine_replicas_one_cycle():
    store, binder, sched = mk(exact=True)
    zones = inventory(store, SMALL)
    job(store, "web", 6, 1)
    plans = _plans_of(sched)
    c = zone_counts(binder, zones)
    assert sum(c.values()) == 6
    assert len(c) == 1, c
    assert list(c) == [best_zone(SMALL)]
    assert len(node_counts(binder)) == 3      # the zone's three small nodes
    cp = plans[0].classes[0]
    assert cp.affinity == (0, 1) and cp.bundle is None and cp.spread is None


@pytest.mark.parametrize("exact", [None, False, "false"])
def test_control_without_exact_scatters(exact):
    """The same inventory without ``exact``: six replicas see an empty group
    six times — what the feature fixes, and what shows the inventory
    discriminates."""
    store, binder, sched = mk(exact=exact)
    zones = inventory(store, SMALL)
    job(store, "web", 6, 1)
    sched.run_once()
    c = zone_counts(binder, zones)
    assert sum(c.values()) == 6
    assert len(c) > 1, c


def _hostname_four(exact, key):
    """Two jobs of two replicas, one group, one cycle, nodes of four."""
    store, binder, sched = mk(exact=exact)
    inventory(store, FOUR)
    job(store, "web-a", 2, 2, key=key, priority=10)
    job(store, "web-b", 2, 2, key=key, priority=0, cpu=400)
    plans = _plans_of(sched)
    return node_counts(binder), plans[0]


@pytest.mark.parametrize("key", [None, "kubernetes.io/hostname"])
def test_hostname_affinity_packs_one_node(key):
    """Four replicas on one node; the identity map has D = N."""
    c, plan = _hostname_four(True, key)
    assert sum(c.values()) == 4 and len(c) == 1, c
    assert [cp.affinity for cp in plan.classes] == [(0, 1), (0, 1)]
    g = plan.spread_groups[0]
    assert g.dom_of.tolist() == list(range(len(FOUR)))
    assert g.count.shape == (len(FOUR),)


def test_hostname_affinity_control_scatters():
    """Without ``exact`` the second job sees an empty group as well."""
    c, plan = _hostname_four(None, None)
    assert sum(c.values()) == 4 and len(c) == 2, c
    assert all(cp.affinity is None for cp in plan.classes)


@pytest.mark.parametrize("exact,nodes,placed", [(True, 1, 3), (None, 2, 4)])
def test_hostname_affinity_stops_at_the_anchor_capacity(exact, nodes, placed):
    """A class of four on nodes of three: three on the anchor and no second
    anchor; without ``exact`` the fourth spills onto the next node."""
    store, binder, sched = mk(exact=exact)
    inventory(store, THREE)
    job(store, "web", 4, 1, key=None)
    sched.run_once()
    c = node_counts(binder)
    assert sum(c.values()) == placed and len(c) == nodes, c


def test_hostname_affinity_gang_too_big_for_one_node():
    """Every node holds two pods; four replicas on ONE node cannot be, and
    with minMember 4 nothing binds."""
    store, binder, sched = mk(exact=True)
    inventory(store, SMALL)
    job(store, "web", 4, 4, key=None)
    sched.run_once()
    assert not binder.binds


def test_second_job_follows_the_first():
    store, binder, sched = mk(exact="true")
    zones = inventory(store, SMALL)
    job(store, "web-a", 2, 1, priority=10)
    job(store, "web-b", 3, 1, priority=0, cpu=400)
    sched.run_once()
    a, b = zone_counts(binder, zones, "web-a"), \
        zone_counts(binder, zones, "web-b")
    assert sum(a.values()) == 2 and sum(b.values()) == 3
    assert len(a) == 1 and list(a) == list(b), (a, b)


def test_gang_revert_gives_the_domain_back():
    """A zone holds six pods: the gang of eight anchors, misses its minimum
    and reverts.  The next job of the group anchors where it would have
    alone, and the group's live counts hold its two pods only."""
    store, binder, sched = mk(exact=True)
    zones = inventory(store, SMALL)
    job(store, "gang", 8, 8, priority=10)
    job(store, "later", 2, 1, priority=0)
    plans = _plans_of(sched)
    assert not any(k.startswith("default/gang") for k in binder.binds)
    c = zone_counts(binder, zones, "later")
    assert c == Counter({best_zone(SMALL): 2}), c
    assert [cp.affinity for cp in plans[0].classes] == [(0, 1), (0, 1)]
    counts = plans[0].spread_counts[0].tolist()
    assert sorted(counts) == [0, 0, 2], counts


def test_member_of_an_earlier_cycle_is_followed():
    """Cycle 1 anchors one pod; the three of cycle 2 do not fit on its node
    and take the other nodes of ITS zone."""
    store, binder, sched = mk(exact=True)
    zones = inventory(store, SMALL)
    job(store, "first", 1, 1, cpu=900)
    sched.run_once()
    anchor = zones[binder.binds["default/first-w-0"]]
    job(store, "rest", 3, 1)
    sched.run_once()
    c = zone_counts(binder, zones, "rest")
    assert c == Counter({anchor: 3}), c
    assert binder.binds["default/first-w-0"] not in \
        node_counts(binder, "rest")


def _anti_after_one_cycle(exact):
    """One member bound in cycle 1, three more in cycle 2; two zones have two
    nodes, so whichever zone the first takes, a free zone has room for two
    as far as the hostname dim is concerned."""
    store, binder, sched = mk(exact=exact)
    zones = inventory(store, ANTI5)
    job(store, "first", 1, 1, kind="podAntiAffinity")
    sched.run_once()
    taken = zones[binder.binds["default/first-w-0"]]
    job(store, "rest", 3, 1, kind="podAntiAffinity")
    plans = _plans_of(sched)
    return taken, zone_counts(binder, zones, "rest"), plans[0]


def test_member_of_an_earlier_cycle_is_avoided():
    taken, c, plan = _anti_after_one_cycle(True)
    assert c == Counter({z: 1 for z in "abc" if z != taken}), c
    assert [cp.affinity for cp in plan.classes] == [(0, 2)]
    g = plan.spread_groups[0]
    assert g.count.tolist() == [int(z == taken) for z in "abc"]
    # the session-open forbid bit is off the class; the mask does its work
    assert not any(int(w) for w in plan.classes[0].forbid)


def test_member_of_an_earlier_cycle_control():
    """Cycle-granular: the taken zone is shut, but two of the three land in
    one of the free zones."""
    taken, c, plan = _anti_after_one_cycle(None)
    assert taken not in c and sum(c.values()) == 3, c
    assert max(c.values()) == 2, c
    assert all(cp.affinity is None for cp in plan.classes)


def test_keyed_anti_affinity_one_per_zone():
    store, binder, sched = mk(exact=True)
    zones = inventory(store, ANTI4)
    job(store, "web", 5, 1, kind="podAntiAffinity")
    plans = _plans_of(sched)
    c = zone_counts(binder, zones)
    assert c == Counter({"a": 1, "b": 1, "c": 1}), c
    cp = plans[0].classes[0]
    assert cp.affinity == (0, 2) and cp.bundle is None and cp.spread is None
    # zones a, b, c -> domains 0, 1, 2, whatever the node order is
    assert sorted(plans[0].spread_groups[0].dom_of.tolist()) == \
        sorted(ord(ANTI4[n][0]) - ord("a") for n in ANTI4)


@pytest.mark.parametrize("exact", [None, False])
def test_keyed_anti_affinity_control_overshoots(exact):
    """The same inventory and job without ``exact``."""
    store, binder, sched = mk(exact=exact)
    zones = inventory(store, ANTI4)
    job(store, "web", 5, 1, kind="podAntiAffinity")
    sched.run_once()
    c = zone_counts(binder, zones)
    assert c == Counter({"a": 2, "b": 1, "c": 1}), c


def test_affinity_wins_over_keyed_anti_affinity_on_one_class():
    """One domain rule per class: affinity is routed exactly, the keyed
    anti-affinity of the same class stays on its forbid bit."""
    store, binder, sched = mk(exact=True)
    inventory(store, ANTI4)
    job(store, "first", 1, 1, kind="podAntiAffinity", group="rack")
    sched.run_once()
    job(store, "web", 2, 1, extra={"podAntiAffinity": {
        "group": "rack", "topologyKey": "zone"}})
    plan = _plans_of(sched)[0]
    cp = plan.classes[0]
    assert cp.affinity is not None and cp.affinity[1] == 1
    assert any(int(w) for w in cp.forbid)


def test_unlabelled_nodes_take_no_member_of_a_keyed_rule():
    for kind in ("podAffinity", "podAntiAffinity"):
        for exact in (True, None):
            store, binder, sched = mk(exact=exact)
            sizes = dict(UNEVEN)
            sizes["huge-nolabel"] = (None, 256000)
            inventory(store, sizes)
            job(store, "web", 2, 1, kind=kind)
            sched.run_once()
            assert binder.binds
            assert "huge-nolabel" not in binder.binds.values(), (kind, exact)


def test_zone_affinity_with_hostname_anti_affinity():
    """All replicas in one zone, at most one per node."""
    store, binder, sched = mk(exact=True)
    zones = inventory(store, SMALL)
    job(store, "web", 5, 1,
        extra={"podAntiAffinity": {"group": "web-host"}})
    plans = _plans_of(sched)
    c = zone_counts(binder, zones)
    assert sum(c.values()) == 3 and len(c) == 1, c
    assert set(node_counts(binder).values()) == {1}
    assert plans[0].classes[0].affinity == (0, 1)


def test_cycle_granular_keyed_path_over_two_cycles():
    """Without ``exact``: the second-cycle pods may take ANY node of the
    hosting zone — the hosting node itself is full — and no other zone."""
    store, binder, sched = mk(exact=None)
    zones = inventory(store, SMALL)
    job(store, "first", 1, 1, cpu=900)
    sched.run_once()
    host = binder.binds["default/first-w-0"]
    job(store, "rest", 2, 1, cpu=900)
    sched.run_once()
    rest = node_counts(binder, "rest")
    assert sum(rest.values()) == 2 and host not in rest
    assert {zones[n] for n in rest} == {zones[host]}, rest


def test_subgroup_policy_jobs_stay_cycle_granular():
    store, binder, sched = mk(exact=True)
    inventory(store, UNEVEN)
    pg = synth.make_podgroup("sg", min_member=1)
    pg.spec.sub_group_policy = [{"subGroupSize": 2, "minSubGroups": 0}]
    store.create("PodGroup", pg)
    for i in range(4):
        p = synth.make_pod(f"sg-w-{i}", "sg", cpu_milli=500, mem=GI,
                           role="w")
        p.affinity = {"podAffinity": {"group": "web",
                                      "topologyKey": "zone"}}
        store.create("Pod", p)
    plans = _plans_of(sched)
    assert plans and plans[0].classes
    assert all(cp.affinity is None for cp in plans[0].classes)
    assert plans[0].spread_groups == []
    assert len(binder.binds) == 4


def test_exact_class_loses_the_session_open_bit():
    """Plan-level view: a follower class of a hosted group is routed
    (descriptor set, never bundled) and no longer carries the hosting
    require bit, while two same-signature jobs stay separate classes."""
    store, binder, sched = mk(exact=True)
    inventory(store, UNEVEN)
    job(store, "first", 1, 1)
    sched.run_once()
    job(store, "web-a", 2, 1)
    job(store, "web-b", 2, 1)              # same signature: would bundle
    plan = _plans_of(sched)[0]
    assert len(plan.classes) == 2 and len(plan.spread_groups) == 1
    assert plan.spread_groups[0].count.tolist() == [1, 0, 0]
    for cp in plan.classes:
        assert cp.affinity == (0, 1) and cp.bundle is None
        assert not any(int(w) for w in cp.require)
    assert len(binder.binds) == 5


def test_group_and_key_names_cannot_collide():
    """An un-keyed group literally named ``web:zone`` and group ``web``
    over key ``zone`` are different rules with different bits: the keyed
    followers may take any node of the hosting zone, the un-keyed ones only
    their own hosting node."""
    store, binder, sched = mk(exact=None)
    zones = inventory(store, SMALL)
    job(store, "keyed", 1, 1, cpu=900)                      # web over zone
    job(store, "plain", 1, 1, cpu=400, group="web:zone", key=None)
    sched.run_once()
    k_host = binder.binds["default/keyed-w-0"]
    p_host = binder.binds["default/plain-w-0"]
    job(store, "keyed2", 2, 1, cpu=900)
    job(store, "plain2", 1, 1, cpu=400, group="web:zone", key=None)
    sched.run_once()
    assert binder.binds["default/plain2-w-0"] == p_host
    rest = node_counts(binder, "keyed2")
    assert sum(rest.values()) == 2
    assert {zones[n] for n in rest} == {zones[k_host]}, rest
