"""Cases for the predicate compile layer: pods and nodes as API objects, a
plain per-(pod, node) evaluator over their strings, and the session's own
compiled ``(tolerated, require, forbid)`` per class.

The evaluator never touches a bit: it imports nothing from
``volcano_amd.scheduler.tensors`` or the plugins, so a wrong bit in the
compiler cannot be mirrored here.

Semantics of ``feasible`` (k8s nodeunschedulable, tainttoleration,
nodeaffinity as the predicates plugin wraps them):

=============  ==========================================================
ready          node is ready and not cordoned
taint          every NoSchedule / NoExecute taint is tolerated by some
               toleration; PreferNoSchedule never blocks.  A toleration
               with an empty effect matches any effect; ``Exists`` with an
               empty key matches every taint; ``Equal`` needs key and
               value equal
selector       every nodeSelector pair is on the node
in             the label is one of the values; no values: no node
notIn          the label is not among the values; an absent label passes
exists         the key is on the node
notExists      the key is not on the node
gt / lt        the label parses as a number and compares strictly; an
               absent or unparsable label fails
=============  ==========================================================
"""

import copy
import random
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from volcano_amd.api.objects import Taint, Toleration
from volcano_amd.utils import synth

GI = 1024 ** 3
HOSTNAME = "kubernetes.io/hostname"
BLOCKING = ("NoSchedule", "NoExecute")
KINDS = ("taint", "selector", "in", "notIn", "exists", "notExists", "gt",
         "lt")

ZONES = ("a", "b", "c")
DISKS = ("ssd", "hdd")
GENS = ("1", "2", "3", "5", "next")          # "next" is no number
BASE_PAIRS = len(ZONES) + len(DISKS) + len(GENS)


# --------------------------------------------------------------------------
# the evaluator
# --------------------------------------------------------------------------

def _tolerates(tol, taint) -> bool:
    if tol.effect != "" and tol.effect != taint.effect:
        return False
    if tol.operator == "Exists":
        return tol.key == "" or tol.key == taint.key
    return tol.key == taint.key and tol.value == taint.value


def _number(text):
    try:
        return float(text)
    except (TypeError, ValueError):
        return None


def feasible(pod, node, drop: Optional[str] = None) -> bool:
    """Whether ``pod`` may run on ``node`` as far as readiness, taints,
    nodeSelector and node affinity go.  ``drop`` names one clause kind
    (``KINDS`` or ``"ready"``) to leave out."""
    labels = node.meta.labels
    aff = pod.affinity or {}
    if drop != "ready" and (not node.ready or node.unschedulable):
        return False
    if drop != "taint":
        for taint in node.taints:
            if taint.effect not in BLOCKING:
                continue
            if not any(_tolerates(tol, taint) for tol in pod.tolerations):
                return False
    if drop != "selector":
        for k, v in pod.node_selector.items():
            if k not in labels or labels[k] != v:
                return False
    if drop != "in":
        for k, vals in (aff.get("in") or {}).items():
            if k not in labels or labels[k] not in list(vals):
                return False
    if drop != "notIn":
        for k, vals in (aff.get("notIn") or {}).items():
            if k in labels and labels[k] in list(vals):
                return False
    if drop != "exists":
        for k in aff.get("exists") or []:
            if k not in labels:
                return False
    if drop != "notExists":
        for k in aff.get("notExists") or []:
            if k in labels:
                return False
    if drop != "gt":
        for k, v in (aff.get("gt") or {}).items():
            n = _number(labels.get(k))
            if n is None or not n > float(v):
                return False
    if drop != "lt":
        for k, v in (aff.get("lt") or {}).items():
            n = _number(labels.get(k))
            if n is None or not n < float(v):
                return False
    return True


def mask(pod, nodes, drop=None) -> List[bool]:
    return [feasible(pod, n, drop) for n in nodes]


def describe_pod(pod) -> str:
    tols = [(t.key, t.operator, t.value, t.effect) for t in pod.tolerations]
    return (f"pod {pod.meta.name}: selector={pod.node_selector} "
            f"affinity={pod.affinity} tolerations={tols}")


def describe_node(node) -> str:
    taints = [(t.key, t.value, t.effect) for t in node.taints]
    return (f"node {node.meta.name}: ready={node.ready} "
            f"unschedulable={node.unschedulable} labels={node.meta.labels} "
            f"taints={taints}")


# --------------------------------------------------------------------------
# worlds
# --------------------------------------------------------------------------

@dataclass
class World:
    nodes: list                      # Node objects, sorted by name
    pods: list                       # one Pod per job
    name: str = ""
    bit63_taint: Optional[Taint] = None   # 64-taint worlds only
    serial: int = 0                  # pod name counter across swaps


# same key and value under two effects, an empty value, PreferNoSchedule
TAINTS = (Taint("dedicated", "gpu", "NoSchedule"),
          Taint("dedicated", "gpu", "NoExecute"),
          Taint("maint", "", "NoSchedule"),
          Taint("soft", "x", "PreferNoSchedule"),
          Taint("team", "a", "NoSchedule"),
          Taint("team", "b", "NoExecute"))


def _taint_pool(size):
    """``size`` distinct blocking taints (the five of TAINTS first)."""
    pool = [t for t in TAINTS if t.effect in BLOCKING]
    i = 0
    while len(pool) < size:
        pool.append(Taint(f"t{i:02d}", f"v{i % 3}",
                          BLOCKING[i % 2]))
        i += 1
    return pool[:size]


def static_pairs(nodes) -> int:
    """Distinct key=value pairs the pack spends a static bit on."""
    return len({(k, v) for n in nodes for k, v in n.meta.labels.items()
                if k != HOSTNAME})


def _node(name, labels):
    """Sizes and requests (make_pod) are powers of two: every fraction a
    score is made of is exact in f32, so the torch runner and the HIP
    plane cannot differ by a rounding."""
    return synth.make_node(name, cpu_milli=32768, mem=256 * GI, pods=128,
                           labels=labels)


def make_world(seed, filler=63, taint_pool=None, n_pods=80,
               n_nodes=None) -> World:
    """65..130 nodes whose labels make exactly ``filler`` distinct pairs.

    With ``taint_pool=K`` the K blocking taints are handed out so that
    taint i first appears on node i (nodes pack in name order): its bit
    is i, and node K-1 carries taint K-1 alone."""
    rng = random.Random(seed * 7919 + filler)
    n = n_nodes or (rng.randint(65, 130) if taint_pool is None else 130)
    nodes = []
    for i in range(n):
        labels = {}
        if i < len(GENS):            # every base pair exists somewhere
            labels = {"zone": ZONES[i % 3], "disk": DISKS[i % 2],
                      "gen": GENS[i]}
        else:
            if rng.random() < 0.85:
                labels["zone"] = rng.choice(ZONES)
            if rng.random() < 0.75:
                labels["disk"] = rng.choice(DISKS)
            if rng.random() < 0.8:
                labels["gen"] = rng.choice(GENS)
        nodes.append(_node(f"n{i:03d}", labels))
    assert filler >= BASE_PAIRS
    for j in range(filler - BASE_PAIRS):       # shared filler pairs
        for i in {j % n, (j * 7 + 3) % n, rng.randrange(n)}:
            nodes[i].meta.labels[f"fill{j:03d}"] = "1"
    assert static_pairs(nodes) == filler

    world = World(nodes=nodes, pods=[],
                  name=f"seed{seed}-filler{filler}"
                       + (f"-taints{taint_pool}" if taint_pool else ""))
    if taint_pool is None:
        pool = list(TAINTS)
        for node in nodes:
            if rng.random() < 0.4:
                node.taints = rng.sample(pool, rng.choice((1, 1, 2)))
    else:
        pool = _taint_pool(taint_pool)
        for i, t in enumerate(pool):
            nodes[i].taints = [t]
            if 0 < i < taint_pool - 1 and rng.random() < 0.3:
                nodes[i].taints.append(pool[rng.randrange(i)])
        for node in nodes[taint_pool:]:
            if rng.random() < 0.3:
                node.taints = [rng.choice(pool)]
        world.bit63_taint = pool[63] if taint_pool >= 64 else None
    for i in rng.sample(range(len(GENS), n), 3):   # a few not ready
        if i % 2:
            nodes[i].ready = False
        else:
            nodes[i].unschedulable = True
    world.pods = [make_pod(world, rng, pool) for _ in range(n_pods)]
    return world


def _tolerations(rng, pool):
    blocking = [t for t in pool if t.effect in BLOCKING]
    roll = rng.random()
    if roll < 0.25:
        return []
    if roll < 0.35:
        return [Toleration(key="", operator="Exists")]
    out = []
    for _ in range(rng.choice((1, 1, 2, 3, 6))):
        t = rng.choice(blocking)
        form = rng.randrange(6)
        if form == 0:
            out.append(Toleration(t.key, "Exists", "", ""))
        elif form == 1:
            out.append(Toleration(t.key, "Exists", "", t.effect))
        elif form == 2:
            out.append(Toleration(t.key, "Equal", t.value, ""))
        elif form == 3:
            out.append(Toleration(t.key, "Equal", t.value, t.effect))
        elif form == 4:              # right pair, the other effect
            other = BLOCKING[1 - BLOCKING.index(t.effect)]
            out.append(Toleration(t.key, "Equal", t.value, other))
        else:                        # right key, a value nobody has
            out.append(Toleration(t.key, "Equal", "other", ""))
    if rng.random() < 0.1:           # tolerating a soft taint changes nothing
        out.append(Toleration("soft", "Equal", "x", "PreferNoSchedule"))
    return out


def _affinity(rng, multi_in_salt=0):
    """A node-affinity dict of 0..3 clause kinds.  ``multi_in_salt``
    rotates the multi-value ``in`` sets, so swapped-in pods never repeat an
    earlier session's set."""
    aff, selector = {}, {}
    kinds = rng.sample(("selector",) + KINDS[2:],
                       rng.choice((0, 1, 1, 1, 1, 2, 2, 3)))
    domain = {"zone": ZONES, "disk": DISKS, "gen": GENS}
    for kind in kinds:
        if kind == "selector":
            roll = rng.random()
            if roll < 0.15:
                selector = {"zone": "nowhere"}
            elif roll < 0.3:
                selector = {"zone": rng.choice(ZONES),
                            "disk": rng.choice(DISKS)}
            else:
                k = rng.choice(("zone", "disk", "gen"))
                selector = {k: rng.choice(domain[k])}
        elif kind == "in":
            k = rng.choice(("zone", "disk", "gen", "gen"))
            count = rng.choice((0, 1, 1, 2, 2, 3))
            vals = list(domain[k]) + ["elsewhere"]
            if count >= 2 and multi_in_salt:
                vals.append(f"salt{multi_in_salt}")
                picked = rng.sample(vals[:-1], count - 1) + [vals[-1]]
            else:
                picked = rng.sample(vals, min(count, len(vals)))
            aff["in"] = {k: picked}
        elif kind == "notIn":
            k = rng.choice(("zone", "disk", "gen"))
            vals = list(domain[k]) + ["elsewhere"]
            aff["notIn"] = {k: rng.sample(vals, rng.choice((1, 2)))}
        elif kind == "exists":
            aff["exists"] = [rng.choice(("disk", "gen", "zone", "ghost"))]
        elif kind == "notExists":
            aff["notExists"] = [rng.choice(("disk", "gen", "ghost",
                                            "fill000"))]
        elif kind == "gt":
            aff["gt"] = {"gen": rng.choice((0, 1, "2", 2.5))}
        elif kind == "lt":
            aff["lt"] = {"gen": rng.choice((2, "3", 4.5, 10))}
    return selector, aff


def make_pod(world, rng, pool, multi_in_salt=0, tolerations=None,
             selector=None, affinity=None, name=None):
    """One pod of a one-pod job; its request is far below any node."""
    if name is None:
        name = f"p{world.serial:04d}"
        world.serial += 1
    sel, aff = _affinity(rng, multi_in_salt)
    pod = synth.make_pod(
        f"{name}-0", name, cpu_milli=128, mem=GI // 16,
        node_selector=sel if selector is None else selector,
        tolerations=_tolerations(rng, pool) if tolerations is None
        else tolerations)
    aff = aff if affinity is None else affinity
    pod.affinity = aff or None
    return pod


def boundary_world() -> World:
    """64 nodes with a distinct ``rack`` pair each (the registry holds
    exactly one full word), a plain gang, and a gang whose nodeSelector
    names a pair no node carries."""
    nodes = [_node(f"n{i:03d}", {"rack": f"r{i}"}) for i in range(64)]
    world = World(nodes=nodes, pods=[], name="word-boundary")
    rng = random.Random(0)
    world.pods = [
        make_pod(world, rng, (), tolerations=[], selector={}, affinity={}),
        make_pod(world, rng, (), tolerations=[],
                 selector={"zone": "nowhere"}, affinity={})]
    return world


def hostname_world(n=1100, n_pods=40) -> World:
    """``n`` nodes that each carry their own hostname label, plus ``zone``.
    Pods 0 and 1 are the acceptance cases; the rest mix hostname clauses
    with the generator's."""
    rng = random.Random(n)
    nodes = []
    for i in range(n):
        name = f"n{i:04d}"
        nodes.append(_node(name, {HOSTNAME: name, "zone": ZONES[i % 3]}))
    for i in rng.sample(range(n), n // 10):
        nodes[i].taints = [rng.choice(TAINTS)]
    world = World(nodes=nodes, pods=[], name=f"hostnames{n}")
    host = lambda: f"n{rng.randrange(n):04d}"
    world.pods = [
        make_pod(world, rng, TAINTS, tolerations=[Toleration("", "Exists")],
                 selector={HOSTNAME: "n0777"}, affinity={}),
        make_pod(world, rng, TAINTS, tolerations=[Toleration("", "Exists")],
                 selector={}, affinity={"notIn": {HOSTNAME: ["n0003",
                                                             "n1099"]}})]
    while len(world.pods) < n_pods:
        form = len(world.pods) % 5
        if form == 0:
            kw = dict(selector={HOSTNAME: host()})
        elif form == 1:
            kw = dict(selector={}, affinity={"in": {HOSTNAME: [
                host() for _ in range(rng.choice((1, 2, 3)))]}})
        elif form == 2:
            kw = dict(selector={"zone": rng.choice(ZONES)},
                      affinity={"notIn": {HOSTNAME: [host(), host(),
                                                     "no-such-host"]}})
        elif form == 3 and len(world.pods) < 10:
            kw = dict(selector={HOSTNAME: "no-such-host"})
        elif form == 3:
            kw = dict(selector={}, tolerations=[Toleration("", "Exists")],
                      affinity={"in": {HOSTNAME: [host(), "no-such-host"]},
                                "exists": ["zone"]})
        else:
            kw = {}
        world.pods.append(make_pod(world, rng, TAINTS, **kw))
    return world


def mutate(world, seed) -> World:
    """The next cycle's world: a third of the nodes edited (``zone``
    changed, ``disk`` removed, taints replaced, readiness flipped) and half
    the pods swapped for new ones whose multi-value ``in`` sets are new.
    Returns a new World; ``world`` stays as it was."""
    rng = random.Random(seed)
    new = World(nodes=[copy.deepcopy(n) for n in world.nodes],
                pods=list(world.pods), name=f"{world.name}+{seed}",
                bit63_taint=world.bit63_taint, serial=world.serial)
    for i in rng.sample(range(len(new.nodes)), len(new.nodes) // 3):
        node = new.nodes[i]
        node.meta.labels["zone"] = rng.choice(ZONES)
        node.meta.labels.pop("disk", None)
        node.taints = rng.sample(list(TAINTS), rng.choice((0, 1, 2)))
        node.ready = not node.ready
    keep = rng.sample(range(len(new.pods)), len(new.pods) // 2)
    new.pods = [new.pods[i] for i in sorted(keep)]
    while len(new.pods) < len(world.pods):
        new.pods.append(make_pod(new, rng, TAINTS, multi_in_salt=seed))
    return new


# --------------------------------------------------------------------------
# the scheduler side
# --------------------------------------------------------------------------

def build(world, device="cpu"):
    """(store, binder, scheduler) holding ``world``; default plugins."""
    from volcano_amd.scheduler import (FakeBinder, Scheduler, SchedulerCache,
                                       default_config)
    from volcano_amd.store import ObjectStore
    store, binder = ObjectStore(), FakeBinder()
    config = default_config()
    if device == "cuda":
        config.use_hip = True
        config.device = "cuda"
    cache = SchedulerCache(store=store, binder=binder, device=device)
    sched = Scheduler(cache, config)
    store.create("Queue", synth.make_queue("default"))
    for node in world.nodes:
        store.create("Node", copy.deepcopy(node))
    for pod in world.pods:
        _create_pod(store, pod)
    return store, binder, sched


def _create_pod(store, pod):
    store.create("PodGroup", synth.make_podgroup(pod.podgroup_name,
                                                 min_member=1))
    store.create("Pod", copy.deepcopy(pod))


def move_store(store, old, new) -> None:
    """Edit the store from world ``old`` to world ``new`` (``mutate``)."""
    before = {n.meta.name: n for n in old.nodes}
    for node in new.nodes:
        was = before[node.meta.name]
        if (node.meta.labels, node.taints, node.ready, node.unschedulable) \
                != (was.meta.labels, was.taints, was.ready,
                    was.unschedulable):
            store.update("Node", copy.deepcopy(node))
    stay = {p.meta.name for p in new.pods}
    for pod in old.pods:
        if pod.meta.name not in stay:
            store.delete("Pod", pod.meta.namespace, pod.meta.name)
            store.delete("PodGroup", pod.meta.namespace, pod.podgroup_name)
    have = {p.meta.name for p in old.pods}
    for pod in new.pods:
        if pod.meta.name not in have:
            _create_pod(store, pod)


@dataclass
class Compiled:
    pod: object
    task: object
    tolerated: int
    require: np.ndarray            # [W] i64, padded to the plane width
    forbid: np.ndarray             # [W] i64
    raw_width: int                 # len(require) as class_constraints gave it


def compiled(ssn) -> List[Compiled]:
    """Per pending class of ``ssn`` (an open session), in job-key order:
    the pod and the session's own class constraints, padded to the plane
    width the way ``CyclePlan.finalize`` does."""
    nt = ssn.node_tensors
    out = []
    for key in sorted(ssn.jobs):
        job = ssn.jobs[key]
        for tc in job.pending_classes():
            tol, require, forbid = ssn.predicates.class_constraints(tc, job)
            out.append(Compiled(tc.tasks[0].pod, tc.tasks[0], tol, require,
                                forbid, len(require)))
    nt.ensure_plane_width()
    W = nt.planes_t.shape[0]
    for c in out:
        if len(c.require) < W:
            c.require = np.pad(c.require, (0, W - len(c.require)))
        if len(c.forbid) < W:
            c.forbid = np.pad(c.forbid, (0, W - len(c.forbid)))
    return out


def reference_mask(nt, c: Compiled) -> List[bool]:
    """``reference.score_cap(...) > -inf`` over host copies of the
    session's tensors for one compiled class."""
    from volcano_amd.ops import reference as ref
    N, R = nt.n, nt.r
    score = torch.empty(N, dtype=torch.float32)
    cap = torch.empty(N, dtype=torch.int32)
    ref.score_cap(nt.alloc_t.t().cpu(), nt.used_t.t().cpu(),
                  torch.zeros(N, R), nt.ready.cpu().bool(),
                  nt.taint_mask.cpu(), nt.planes_t.t().cpu(),
                  torch.from_numpy(nt.req_vector(c.task)), c.tolerated,
                  torch.from_numpy(c.require), torch.from_numpy(c.forbid),
                  1.0, 0.0, 0.0, torch.ones(R), None, score, cap)
    return (score > float("-inf")).tolist()


def first_difference(world, c: Compiled, got, want) -> str:
    """Failure text: the pod's constraints and the first node on which the
    compiled mask and the evaluator disagree."""
    i = next(i for i, (g, w) in enumerate(zip(got, want)) if g != w)
    return (f"[{world.name}] {describe_pod(c.pod)}\n  compiled says "
            f"{got[i]}, evaluator says {want[i]} on "
            f"{describe_node(world.nodes[i])}\n  tolerated={c.tolerated:#x} "
            f"require={[hex(int(x) & (2**64 - 1)) for x in c.require]} "
            f"forbid={[hex(int(x) & (2**64 - 1)) for x in c.forbid]}")


def check_binds(world, binds) -> None:
    """Every bound pod sits on a feasible node; every unbound pod has
    none."""
    by_name = {n.meta.name: n for n in world.nodes}
    for pod in world.pods:
        node = binds.get(pod.meta.key)
        if node is not None:
            assert feasible(pod, by_name[node]), \
                f"bound to an infeasible node: {describe_pod(pod)}\n  " \
                + describe_node(by_name[node])
        else:
            ok = [n for n in world.nodes if feasible(pod, n)]
            assert not ok, \
                f"left pending with {len(ok)} feasible nodes: " \
                f"{describe_pod(pod)}\n  e.g. {describe_node(ok[0])}"
    assert set(binds) <= {p.meta.key for p in world.pods}


# the case set of both test files: fillers around the word boundaries times
# two seeds, and one world that uses all 64 taint bits
FILLERS = (63, 64, 65, 127, 128, 129)
WORLDS = {f"f{f}-s{s}": (lambda f=f, s=s: make_world(s, filler=f))
          for f in FILLERS for s in (0, 1)}
WORLDS["taints64"] = lambda: make_world(2, filler=64, taint_pool=64)
