"""The plans, binds and allocate events of a fixed set of small clusters,
as text, against ``tests/plan_fingerprint.expected``.

The expected file pins what the allocate plan builder emits: every field of
every ``JobPlan`` and ``ClassPlan``, the domain groups, the bundle entries
in order, what the binder bound and what ``on_allocate`` was told.  It is
recorded by running this module as a program (``python
tests/test_plan_fingerprint.py``) on a tree whose builder is trusted, and is
never rewritten to follow the code under test.

Tasks are named ``namespace/name``: the store draws a random uid per object,
the name is the identity that is the same in every run.

The scenarios come from the builders the other test modules already use; the
last test checks that together they reach every emission path of the builder
and every exact rule, so that none of them goes unpinned.
"""

import contextlib
import functools
import re
import sys
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

import _coherence_cases as cc
import _deviceshare_cases as dc
import _hypernode_cases as hc
import test_affinity_e2e as aff
import test_numa_exact as numa
import test_spread_e2e as spr
import test_task_topology_bucket as ttb
from _plan_spy import plans_of, spying
from volcano_amd.ops import host
from volcano_amd.scheduler.actions.allocate import AllocateAction
from volcano_amd.scheduler.session import Session
from volcano_amd.utils import synth

EXPECTED = Path(__file__).with_name("plan_fingerprint.expected")
GI = 1024 ** 3
PATHS = ("fused run", "bundle continuation", "bundle open",
         "unbundled single class", "multi-class", "subgroup", "nominated")
RULES = ("spread", "affinity", "hypernode", "device", "numa")


# -- a plan as text -----------------------------------------------------------

def _hex(a, dtype):
    return "[" + " ".join(f"{int(x):x}" for x in
                          np.ascontiguousarray(a).view(dtype)) + "]"


def _name(t):
    return f"{t.namespace}/{t.name}"


def fingerprint(plan) -> str:
    """A finalized ``CyclePlan`` as plain text."""
    out = []
    for jp in plan.jobs:
        out.append(f"job {jp.job_key} classes [{jp.class_begin}, "
                   f"{jp.class_end}) occupied {jp.occupied} "
                   f"min_available {jp.min_available}")
    rows = {}
    for c, cp in enumerate(plan.classes):
        if cp.bias is not None:
            rows.setdefault(id(cp.bias), []).append(c)
    for c, cp in enumerate(plan.classes):
        bias = "-" if cp.bias is None else \
            f"row shared with {[x for x in rows[id(cp.bias)] if x != c]}"
        out.append(
            f"class {c} {cp.job_key} queue {cp.queue_idx} ntasks {cp.ntasks} "
            f"min_needed {cp.min_needed} tolerated {int(cp.tolerated)}\n"
            f"  req {_hex(np.asarray(cp.req, dtype=np.float32), np.uint32)} "
            f"require {_hex(cp.require, np.uint64)} "
            f"forbid {_hex(cp.forbid, np.uint64)}\n"
            f"  w {cp.w_least!r} {cp.w_most!r} {cp.w_bal!r} bias {bias}\n"
            f"  spread {cp.spread} affinity {cp.affinity} "
            f"hypernode {cp.hypernode} device {cp.device} numa {cp.numa}")
        for be in cp.bundle or ():
            out.append(f"  entry {be.job_key} ntasks {be.ntasks} min_needed "
                       f"{be.min_needed} " + " ".join(map(_name, be.tasks)))
    for g, sg in enumerate(plan.spread_groups):
        out.append(f"group {g} dom_of {sg.dom_of.tolist()} count "
                   f"{sg.count.tolist()} row {sg.row} leaves {sg.leaves}")
    out.append(f"device_state {plan.device_state is not None} "
               f"numa_state {plan.numa_state is not None}")
    out.append(f"job_alias {getattr(plan, 'job_alias', None)}")
    out.append(f"subgroup_families {getattr(plan, 'subgroup_families', None)}")
    return "\n".join(out)


# -- what a scenario leaves behind ----------------------------------------------

class Recorder:
    """Everything one scenario did that the expected file pins, and the
    counts of the coverage condition."""

    def __init__(self):
        self.events = []
        self.fused = []         # entry lists the fused-run loop returned
        self.nominated = 0

    @contextlib.contextmanager
    def recording(self):
        """Record ``on_allocate`` argument lists, the entry lists of fused
        runs (both the native loop and its Python oracle) and the gangs
        that took the nominated path."""
        rec = self
        fire = Session.fire_allocate
        entries_py = AllocateAction.__dict__["_run_entries_py"]
        nominated = AllocateAction._try_nominated
        mod = host.load()
        entries_native = getattr(mod, "bundle_entries", None)

        def fire_spy(ssn, tclass, node_ids, counts, tasks=None):
            rec.events.append(
                f"{tclass.tasks[0].job_key} {tclass.role} nodes "
                f"{[int(n) for n in node_ids]} counts "
                f"{[int(k) for k in counts]} tasks "
                + " ".join(map(_name, tasks or ())))
            return fire(ssn, tclass, node_ids, counts, tasks)

        def entries_spy(real):
            def run(*args):
                got = real(*args)
                rec.fused.append(got[0])
                return got
            return run

        def nominated_spy(action, *args):
            ok = nominated(action, *args)
            rec.nominated += bool(ok)
            return ok

        Session.fire_allocate = fire_spy
        AllocateAction._run_entries_py = staticmethod(
            entries_spy(entries_py.__func__))
        AllocateAction._try_nominated = nominated_spy
        if entries_native is not None:
            mod.bundle_entries = entries_spy(entries_native)
        try:
            yield
        finally:
            Session.fire_allocate = fire
            AllocateAction._run_entries_py = entries_py
            AllocateAction._try_nominated = nominated
            if entries_native is not None:
                mod.bundle_entries = entries_native

    def count(self, plans) -> Counter:
        """Classes per emission path and per rule.  A bundle that no fused
        run returned was opened by one gang and continued by the rest."""
        n = Counter({"nominated": self.nominated})
        for plan in plans:
            for jp in plan.jobs:
                if jp.class_end - jp.class_begin > 1:
                    n["multi-class"] += jp.class_end - jp.class_begin
                    continue
                cp = plan.classes[jp.class_begin]
                if "#sg" in cp.job_key:
                    n["subgroup"] += 1
                elif cp.bundle is None:
                    n["unbundled single class"] += 1
                elif any(cp.bundle is e for e in self.fused):
                    n["fused run"] += 1
                else:
                    n["bundle open"] += 1
                    n["bundle continuation"] += len(cp.bundle) - 1
            for cp in plan.classes:
                for rule in RULES:
                    n[rule] += getattr(cp, rule) is not None
        return n


# -- scenarios: name -> () -> (plans, binds) ---------------------------------------

def _coherence(name):
    def run():
        world = cc.World(cc.SCENARIOS[name])
        world.run()
        return [r.plan for r in world.runs], world.binds()
    return run


def _deviceshare(exact):
    def run():
        with spying() as plans:
            binds, _, _ = dc.run_cluster(exact)
        return plans, binds
    return run


def _numa(policy, nodes):
    def run():
        with spying() as plans:
            binds, _, _ = numa.run_cluster(policy, nodes)
        return plans, binds
    return run


def _hypernode_gangs():
    with spying() as plans:
        binds = hc.schedule("two-gangs")
    return plans, binds


def _hypernode_subgroups():
    """Two racks of two nodes, one SubGroupPolicy job whose two subgroups
    each carry a topology override (the cluster of
    ``test_subgroups.test_per_subgroup_topology_domains``, with ``exact``)."""
    from volcano_amd.api.objects import (HyperNode, HyperNodeMember,
                                         MemberSelector, ObjectMeta)
    from volcano_amd.scheduler import (FakeBinder, Scheduler, SchedulerCache,
                                       default_config)
    from volcano_amd.scheduler.config import PluginOption
    from volcano_amd.store import ObjectStore
    store, binder = ObjectStore(), FakeBinder()
    config = default_config()
    config.tiers[1].plugins.append(PluginOption(
        "network-topology-aware", arguments={"exact": True}))
    sched = Scheduler(SchedulerCache(store=store, binder=binder), config)
    for rack in "ab":
        names = [f"{rack}{i}" for i in range(2)]
        for name in names:
            store.create("Node", synth.make_node(name, cpu_milli=2000,
                                                 mem=64 * GI))
        store.create("HyperNode", HyperNode(
            meta=ObjectMeta(name=f"rack-{rack}"), tier=1,
            members=[HyperNodeMember(
                type="Node", selector=MemberSelector(exact_match=names))]))
    store.create("Queue", synth.make_queue("default"))
    pg = synth.make_podgroup("tp", min_member=1)
    pg.spec.sub_group_policy = [{
        "subGroupSize": 2, "minSubGroups": 2,
        "networkTopology": {"mode": "hard", "highestTierAllowed": 1}}]
    store.create("PodGroup", pg)
    for i in range(4):
        store.create("Pod", synth.make_pod(f"tp-w-{i}", "tp", cpu_milli=2000,
                                           mem=GI, role="worker"))
    return plans_of(sched), dict(binder.binds)


def _spread():
    """``test_exact_classes_carry_a_spread_descriptor``: zone a saturated at
    session open, two same-signature jobs of the group."""
    store, binder, sched = spr.mk(exact=True)
    sizes = dict(spr.UNEVEN)
    sizes["nolabel"] = (None, 8000)
    spr.inventory(store, sizes)
    spr.spread_job(store, "first", 1, 1)
    plans = plans_of(sched)
    spr.spread_job(store, "web-a", 2, 1)
    spr.spread_job(store, "web-b", 2, 1)
    return plans + plans_of(sched), dict(binder.binds)


def _affinity():
    """``test_exact_class_loses_the_session_open_bit``: followers of a
    hosted group lose the require bit."""
    store, binder, sched = aff.mk(exact=True)
    aff.inventory(store, aff.UNEVEN)
    aff.job(store, "first", 1, 1)
    plans = plans_of(sched)
    aff.job(store, "web-a", 2, 1)
    aff.job(store, "web-b", 2, 1)
    return plans + plans_of(sched), dict(binder.binds)


def _anti_affinity():
    """``test_member_of_an_earlier_cycle_is_avoided``: a keyed anti-affinity
    class loses the forbid bit of the taken zone."""
    store, binder, sched = aff.mk(exact=True)
    aff.inventory(store, aff.ANTI5)
    aff.job(store, "first", 1, 1, kind="podAntiAffinity")
    plans = plans_of(sched)
    aff.job(store, "rest", 3, 1, kind="podAntiAffinity")
    return plans + plans_of(sched), dict(binder.binds)


def _affinity_over_anti():
    """``test_affinity_wins_over_keyed_anti_affinity_on_one_class``."""
    store, binder, sched = aff.mk(exact=True)
    aff.inventory(store, aff.ANTI4)
    aff.job(store, "first", 1, 1, kind="podAntiAffinity", group="rack")
    plans = plans_of(sched)
    aff.job(store, "web", 2, 1, extra={"podAntiAffinity": {
        "group": "rack", "topologyKey": "zone"}})
    return plans + plans_of(sched), dict(binder.binds)


def _class_bias():
    """``task-topology`` registers a class bias function, so no fused runs
    are tracked: two identical plain gangs open and continue a bundle one
    by one, and in the second cycle the workers follow the bound ps with a
    bias row."""
    store, binder, _, sched = ttb.mk({"affinity": [["ps", "worker"]]})
    store.create("PodGroup", synth.make_podgroup("tj", min_member=1))
    store.create("Pod", synth.make_pod("tj-ps-0", "tj", cpu_milli=500,
                                       mem=GI, role="ps"))
    for name in ("plain-a", "plain-b"):
        cc.gang(store, name, 2, cpu=500)
    plans = plans_of(sched)
    for i in range(2):
        store.create("Pod", synth.make_pod(f"tj-worker-{i}", "tj",
                                           cpu_milli=500, mem=GI,
                                           role="worker"))
    return plans + plans_of(sched), dict(binder.binds)


def _legacy(name):
    """A coherence world with the session's ``JobTable`` taken away: the
    per-job selection and ordering, and no fused runs."""
    def run():
        world = cc.World(cc.SCENARIOS[name])
        with spying() as plans:
            ssn = world.sched.open_session()
            ssn.job_table = None
            for action in world.sched._actions:
                action.execute(ssn)
            world.sched.close_session(ssn)
        return plans, world.binds()
    return run


SCENARIOS = {
    **{f"coherence {n}": _coherence(n) for n in cc.SCENARIOS},
    "deviceshare exact": _deviceshare(True),
    "deviceshare default": _deviceshare(None),
    "deviceshare off": _deviceshare(False),
    "numa hard": _numa("single-numa-node", {"a": [4000, 4000], "b": [4000]}),
    "numa best-effort": _numa("best-effort", {"a": [4000, 4000]}),
    "spread": _spread,
    "affinity": _affinity,
    "anti-affinity": _anti_affinity,
    "affinity over anti-affinity": _affinity_over_anti,
    "hypernode gangs": _hypernode_gangs,
    "hypernode subgroups": _hypernode_subgroups,
    "class bias": _class_bias,
    "legacy bundle_quota": _legacy("bundle_quota"),
    "legacy two_role_short": _legacy("two_role_short"),
}


@functools.lru_cache(maxsize=None)
def outcome(name):
    """(text, counts) of one scenario, computed once."""
    rec = Recorder()
    with rec.recording():
        plans, binds = SCENARIOS[name]()
    lines = []
    for k, plan in enumerate(plans):
        lines += [f"-- plan {k}", fingerprint(plan)]
    lines.append("-- binds")
    lines += [f"{pod} {node}" for pod, node in binds.items()]
    lines.append("-- on_allocate")
    lines += rec.events
    return "\n".join(lines) + "\n", rec.count(plans)


def header(name):
    return f"== {name}\n"


def recorded():
    """{scenario: text} of the expected file."""
    out = {}
    for block in re.split(r"^== ", EXPECTED.read_text(), flags=re.M)[1:]:
        name, text = block.split("\n", 1)
        out[name] = text
    return out


def test_the_file_holds_exactly_these_scenarios():
    assert list(recorded()) == list(SCENARIOS)


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_plans_binds_and_events_equal_the_recorded_ones(name):
    got, want = outcome(name)[0], recorded()[name]
    if got != want:
        g, w = got.split("\n"), want.split("\n")
        k = next((i for i, (a, b) in enumerate(zip(g, w)) if a != b),
                 min(len(g), len(w)))
        pytest.fail(f"{name}: line {k} differs\n  recorded: "
                    f"{w[k] if k < len(w) else '<end>'}\n  now:      "
                    f"{g[k] if k < len(g) else '<end>'}")
    assert got.encode() == want.encode()


def test_every_emission_path_and_rule_is_reached():
    total = Counter()
    for name in SCENARIOS:
        total += outcome(name)[1]
    print({k: total[k] for k in PATHS + RULES})
    assert [k for k in PATHS + RULES if total[k] == 0] == []


if __name__ == "__main__":
    text = "".join(header(n) + outcome(n)[0] for n in SCENARIOS)
    total = Counter()
    for n in SCENARIOS:
        total += outcome(n)[1]
    EXPECTED.write_text(text)
    print({k: total[k] for k in PATHS + RULES}, len(text), "bytes")
