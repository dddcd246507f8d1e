"""Several topology-spread constraints per class: the sequential oracle
(``reference.spread_multi_select_commit``) against the single-rule oracle and
a hand-checked case, and pods with a ``topologySpread`` list through the
scheduler on the torch runner."""

from collections import Counter

import numpy as np
import pytest
import torch

import _domain_score_cases as dsc
import _spread_cases as sc
import test_spread_e2e as e2e
from volcano_amd.ops import reference as ref
from volcano_amd.utils import synth


def run_multi(case, rules):
    """The multi-rule oracle on fresh copies of ``case`` -> the result dict of
    ``_spread_cases.run_oracle`` with one count vector per rule."""
    t = torch.from_numpy
    used, qa = t(case.used.copy()), t(case.queue_alloc.copy())
    ln, lc = (torch.zeros(case.K, dtype=torch.int32) for _ in range(2))
    ll, placed = (torch.zeros((), dtype=torch.int32) for _ in range(2))
    jp = torch.full((), 7, dtype=torch.int32)
    rs = [(t(np.array(d, dtype=np.int32)), t(np.array(c, dtype=np.int32)), k)
          for d, c, k in rules]
    ref.spread_multi_select_commit(
        t(case.score.copy()), t(case.cap.copy()), t(case.req.copy()),
        case.ntasks, used, qa, t(case.queue_limit.copy()), ln, lc, ll, placed,
        jp, rs)
    return dict(log_nodes=ln.numpy(), log_counts=lc.numpy(), log_len=int(ll),
                placed=int(placed), job_placed=int(jp), used=used.numpy(),
                queue_alloc=qa.numpy(),
                counts=[c.numpy() for _, c, _ in rs], rules=rs)


@pytest.mark.parametrize("name", [n for n in dsc.SPREAD_CASES
                                  if "gang-revert" not in n])
def test_one_rule_is_spread_select_commit(name):
    case, want = dsc.oracle(name)
    got = run_multi(case, [(case.dom_of, case.dom_count, case.max_skew)])
    for key in ("log_nodes", "log_counts", "used", "queue_alloc"):
        assert np.array_equal(got[key].view(np.int32),
                              want[key].view(np.int32)), key
    for key in ("log_len", "placed", "job_placed"):
        assert got[key] == want[key], key
    assert got["counts"][0].tolist() == want["dom_count"].tolist()


def hand_case():
    """7 nodes, zones a a a b b c c, one domain per host, both maxSkew 1,
    scores descending with the index, cap 2 everywhere, 5 replicas."""
    N = 7
    case = sc.SpreadCase(
        "hand", np.arange(N, 0, -1).astype(np.float32),
        np.full(N, 2, dtype=np.int32), np.ones(1, dtype=np.float32), 5,
        np.zeros((N, 1), dtype=np.float32), np.zeros(1, dtype=np.float32),
        np.full(1, sc.BIG, dtype=np.float32),
        np.array([0, 0, 0, 1, 1, 2, 2], dtype=np.int32),
        np.zeros(3, dtype=np.int32), 1)
    return case, [(case.dom_of, case.dom_count, 1),
                  (np.arange(N, dtype=np.int32), np.zeros(N, dtype=np.int32), 1)]


def test_hand_checked_zone_and_hostname():
    """n0 (zone a); a shut, host 0 shut: n3 (b); n5 (c); the zone minimum
    rises to 1, a reopens but host 0 stays shut (host minimum 0): n1; then
    b: n4.  Zone alone would have taken n0 twice."""
    case, rules = hand_case()
    got = run_multi(case, rules)
    assert got["log_nodes"][:got["log_len"]].tolist() == [0, 3, 5, 1, 4]
    assert [c.tolist() for c in got["counts"]] == [[2, 2, 1],
                                                   [1, 1, 0, 1, 1, 1, 0]]
    assert got["used"][:, 0].tolist() == got["counts"][1].tolist()
    assert run_multi(case, rules[:1])["log_counts"][0] == 2
    # the revert gives every rule its counts back
    t = torch.from_numpy
    ref.spread_multi_revert(
        torch.zeros((), dtype=torch.uint8), t(got["log_nodes"]),
        t(got["log_counts"]), torch.tensor(5), torch.ones(1), t(got["used"]),
        t(got["queue_alloc"]), torch.tensor(5), torch.tensor(12), got["rules"])
    assert not got["counts"][0].any() and not got["counts"][1].any()
    assert not got["used"].any() and not got["log_counts"].any()


@pytest.mark.parametrize("rules", [
    [(0, 1), (0, 2)], [(0, 1), (1, 0)], [(1, 1), (0, 1)], [(0, 1), (2, 1)],
    [(0, 1)] * 5])
def test_plan_rejects_bad_rule_sets(rules):
    """A group twice, skew 0, rule 0 not ``spread``, unknown group, five."""
    plan = sc.build_spread_plan(sc.spread_plan_case(N=65, bulk=False), "cpu")
    plan.classes[0].spread, plan.classes[0].spread_rules = (0, 1), rules
    with pytest.raises(ValueError):
        plan.check_spread_rules(0, plan.classes[0])


HOST = "kubernetes.io/hostname"
# zone a has the two large hosts: scoring alone piles everything on a0
HOSTS = {"a0": ("a", 64000), "a1": ("a", 32000), "b0": ("b", 8000),
         "b1": ("b", 8000), "c0": ("c", 8000), "c1": ("c", 8000)}


def inventory(store, extra=()):
    zones = {}
    for name, (zone, cpu) in HOSTS.items():
        store.create("Node", synth.make_node(
            name, cpu_milli=cpu, mem=256 * e2e.GI,
            labels={"zone": zone, HOST: name}))
        zones[name] = zone
    for name, labels in extra:
        store.create("Node", synth.make_node(name, cpu_milli=256000,
                                             mem=256 * e2e.GI, labels=labels))
    store.create("Queue", synth.make_queue("default"))
    return zones


def two_rule_job(store, name, replicas):
    store.create("PodGroup", synth.make_podgroup(name, min_member=1))
    for i in range(replicas):
        p = synth.make_pod(f"{name}-w-{i}", name, cpu_milli=500, mem=e2e.GI,
                           role="w")
        p.affinity = {"topologySpread": [
            {"group": "web", "topologyKey": "zone", "maxSkew": 1},
            {"group": "web", "topologyKey": HOST, "maxSkew": 1}]}
        store.create("Pod", p)


@pytest.mark.parametrize("exact", [True, None])
def test_two_constraints_through_the_scheduler(exact):
    """Six replicas in one cycle with ``exact``, one pod per cycle without
    (cycle-granular bits): one per host, two per zone, and a node that lacks
    one of the two labels stays out, however large it is."""
    store, binder, sched = e2e.mk(exact=exact)
    zones = inventory(store, extra=[("no-zone", {HOST: "no-zone"}),
                                    ("no-host", {"zone": "a"})])
    if exact:
        two_rule_job(store, "web", 6)
        sched.run_once()
    else:
        for i in range(6):
            two_rule_job(store, f"web{i}", 1)
            sched.run_once()
    nodes = list(binder.binds.values())
    assert len(nodes) == 6 and not {"no-zone", "no-host"} & set(nodes)
    per_host = Counter(nodes + list(HOSTS))      # every host counts from 1
    per_zone = Counter(zones[n] for n in nodes)
    assert max(per_host.values()) - min(per_host.values()) <= 1, per_host
    assert sorted(per_zone.values()) == [2, 2, 2], per_zone
