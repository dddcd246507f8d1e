"""The predicate compile layer against a plain per-(pod, node) evaluator.

Every kernel test hands kernel and oracle the same ``taints``, ``planes``,
``tolerated``, ``require`` and ``forbid`` words.  These tests check that the
words mean what the pod and node objects say: ``NodeTensors.pack``,
``tolerated_mask``, ``selector_bits``, the dynamic bits,
``PredicatesPlugin.class_constraints`` and the width padding, through a
session's own tensors and through ``Scheduler.run_once``."""

import functools
import random

import pytest

import _predicate_cases as pc


@functools.lru_cache(maxsize=None)
def world(name):
    """Built once, never modified (the store gets deep copies)."""
    return pc.WORLDS[name]()


@functools.lru_cache(maxsize=None)
def truth(name):
    """{pod name: evaluator mask over the world's nodes}."""
    w = world(name)
    return {p.meta.name: pc.mask(p, w.nodes) for p in w.pods}


def informative(w, masks) -> int:
    """Classes whose mask over the READY nodes is neither empty nor full
    (a not-ready node rejects every pod and would make 'not full' free)."""
    ready = [i for i, n in enumerate(w.nodes)
             if n.ready and not n.unschedulable]
    return sum(0 < sum(m[i] for i in ready) < len(ready)
               for m in masks.values())


def open_and_compile(sched):
    ssn = sched.open_session()
    try:
        return ssn, pc.compiled(ssn)
    finally:
        sched.close_session(ssn)


def assert_masks(w, ssn, classes, want=None):
    assert len(classes) == len(w.pods)
    assert ssn.node_tensors.names == [n.meta.name for n in w.nodes]
    for c in classes:
        expect = want[c.pod.meta.name] if want else pc.mask(c.pod, w.nodes)
        got = pc.reference_mask(ssn.node_tensors, c)
        assert got == expect, pc.first_difference(w, c, got, expect)


# --------------------------------------------------------------------------
# non-vacuity: from the evaluator alone, before any comparison
# --------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(pc.WORLDS))
def test_world_is_informative(name):
    w = world(name)
    assert 65 <= len(w.nodes) <= 130
    n = informative(w, truth(name))
    print(f"{name}: {n} of {len(w.pods)} masks neither empty nor full")
    assert 2 * n >= len(w.pods)


def test_static_registry_sits_where_the_world_says():
    for name in pc.WORLDS:
        want = 64 if name == "taints64" else int(name[1:].split("-")[0])
        assert pc.static_pairs(world(name).nodes) == want


def test_every_clause_kind_is_somewhere_the_sole_reason():
    sole = dict.fromkeys(pc.KINDS, 0)
    empty_in = 0
    for name in pc.WORLDS:
        w = world(name)
        for pod in w.pods:
            ins = ((pod.affinity or {}).get("in") or {}).values()
            empty_in += any(len(v) == 0 for v in ins)
            full = truth(name)[pod.meta.name]
            for kind in pc.KINDS:
                dropped = pc.mask(pod, w.nodes, drop=kind)
                sole[kind] += sum(d and not f for d, f in zip(dropped, full))
    print("sole-reason (pod, node) pairs:", sole, "empty-in classes:",
          empty_in)
    assert all(sole[k] > 0 for k in pc.KINDS), sole
    assert empty_in >= 3


def test_taint_bit_63_is_tolerated_by_one_class_and_blocks_another():
    w = world("taints64")
    t = w.bit63_taint
    node = w.nodes[63]
    assert node.taints == [t] and node.ready and not node.unschedulable
    tolerated = [p for p in w.pods if pc.feasible(p, node)]
    blocked = [p for p in w.pods if not pc.feasible(p, node)
               and pc.feasible(p, node, drop="taint")]
    print(f"bit 63: {len(tolerated)} classes pass, {len(blocked)} blocked "
          "by it alone")
    assert tolerated and blocked
    _, _, sched = pc.build(w)
    ssn, classes = open_and_compile(sched)
    nt = ssn.node_tensors
    assert nt.taints.index[f"{t.key}={t.value}:{t.effect}"] == 63
    assert len(nt.taints.index) == 64
    assert int(nt.taints_np[63]) == -2 ** 63
    by_pod = {c.pod.meta.name: c for c in classes}
    assert by_pod[tolerated[0].meta.name].tolerated < 0       # bit 63 set
    assert by_pod[blocked[0].meta.name].tolerated >= 0


# --------------------------------------------------------------------------
# mask equality
# --------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(pc.WORLDS))
def test_compiled_masks_equal_the_evaluator(name):
    w = world(name)
    _, _, sched = pc.build(w)
    ssn, classes = open_and_compile(sched)
    assert_masks(w, ssn, classes, truth(name))


def test_bits_beyond_word_zero_are_in_use():
    """Some class requires, and some class forbids, a bit in a word >= 1."""
    req_hi = forbid_hi = 0
    for name in ("f64-s0", "f128-s0"):
        _, _, sched = pc.build(world(name))
        _, classes = open_and_compile(sched)
        req_hi += sum(bool(c.require[1:].any()) for c in classes)
        forbid_hi += sum(bool(c.forbid[1:].any()) for c in classes)
    print(f"classes with a require bit in word >= 1: {req_hi}, "
          f"with a forbid bit: {forbid_hi}")
    assert req_hi > 0 and forbid_hi > 0


@pytest.mark.parametrize("name", ["f64-s0", "f127-s1", "taints64"])
def test_second_and_third_cycle_on_the_same_cache(name):
    """Node edits and swapped pods between sessions of one cache: sticky
    registries and the full repack on node events (which also zeroes the
    dynamic planes; ``clear_dynamic_bits`` on its own is pinned by
    test_no_dynamic_membership_outlives_its_session)."""
    w = world(name)
    store, _, sched = pc.build(w)
    ssn, classes = open_and_compile(sched)
    assert_masks(w, ssn, classes, truth(name))
    for cycle in (1, 2):
        nxt = pc.mutate(w, seed=cycle)
        masks = {p.meta.name: pc.mask(p, nxt.nodes) for p in nxt.pods}
        assert 2 * informative(nxt, masks) >= len(nxt.pods)
        assert masks != {p.meta.name: pc.mask(p, w.nodes) for p in nxt.pods}
        pc.move_store(store, w, nxt)
        ssn, classes = open_and_compile(sched)
        assert_masks(nxt, ssn, classes, masks)
        w = nxt


def test_no_dynamic_membership_outlives_its_session():
    """Sessions of one cache with pods swapped and NO node event: nothing
    is repacked, so only ``clear_dynamic_bits`` stands between an earlier
    session's node sets and the next one.  After the second open every
    dynamic plane is zero; a third session resolves hostname and
    multi-value bits again and equals the evaluator."""
    from volcano_amd.scheduler.tensors import NodeTensors
    first = pc.hostname_world(n=70, n_pods=20)
    plain = pc.World(nodes=first.nodes, name="plain", serial=first.serial,
                     pods=[pc.make_pod(first, random.Random(1), pc.TAINTS,
                                       selector={"zone": "a"}, affinity={})])
    third = pc.hostname_world(n=70, n_pods=20)
    for p, q in zip(third.pods, first.pods):
        assert p.meta.name == q.meta.name
    third.pods = third.pods[::2]         # another order of registration
    store, _, sched = pc.build(first)
    packs, real = [], NodeTensors.pack

    def counting(self, *a, **kw):
        packs.append(1)
        return real(self, *a, **kw)

    NodeTensors.pack = counting
    try:
        ssn, classes = open_and_compile(sched)
        nt = ssn.node_tensors
        assert_masks(first, ssn, classes)

        def membership():
            return {b: int(((nt.planes_np[b // 64] >> (b % 64)) & 1).sum())
                    for b in nt._dynamic_bits}

        assert packs == [1]
        assert sum(membership().values()) > 0
        assert sum(n > 0 for n in membership().values()) >= 5

        pc.move_store(store, first, plain)
        ssn = sched.open_session()
        assert ssn.node_tensors is nt and packs == [1]
        assert set(membership().values()) == {0}
        assert torch_planes_equal(nt)
        classes = pc.compiled(ssn)
        sched.close_session(ssn)
        assert_masks(plain, ssn, classes)

        pc.move_store(store, plain, third)
        ssn, classes = open_and_compile(sched)
        assert packs == [1]
        assert_masks(third, ssn, classes)
    finally:
        NodeTensors.pack = real


def torch_planes_equal(nt) -> bool:
    """The device planes carry what their host mirror carries."""
    return (nt.planes_t.cpu().numpy() == nt.planes_np).all()


def test_width_grows_inside_one_session():
    """64 static pairs fill word 0.  A plain class compiled first comes out
    one word wide, later classes register bits in word 1; after the
    padding all have the plane width and still equal the evaluator."""
    base = world("f64-s0")
    w = pc.World(nodes=base.nodes, pods=[], name="width-growth")
    plain = pc.make_pod(w, random.Random(0), pc.TAINTS, tolerations=[],
                        selector={}, affinity={},
                        name="a-plain")      # first in job-key order
    w.pods = [plain] + base.pods[:30]
    _, _, sched = pc.build(w)
    ssn, classes = open_and_compile(sched)
    assert classes[0].pod.meta.name == "a-plain-0"
    assert classes[0].raw_width == 1
    assert max(c.raw_width for c in classes) == 2
    W = ssn.node_tensors.planes_t.shape[0]
    assert W == 2 and ssn.node_tensors.planes_np.shape[0] == 2
    assert all(len(c.require) == W and len(c.forbid) == W for c in classes)
    assert_masks(w, ssn, classes)


def test_a_hook_may_open_a_new_word():
    """A class-constraint hook that registers its bit while it runs, with
    word 0 full: the in-place set lands inside the vector it was given."""
    from volcano_amd.scheduler.tensors import set_plane_bit
    w = pc.boundary_world()
    _, _, sched = pc.build(w)
    ssn = sched.open_session()
    nt = ssn.node_tensors
    assert len(nt.labels.index) == 64

    def hook(tclass, job, require, forbid):
        set_plane_bit(forbid, nt.add_dynamic_bit("late", [5]))

    ssn.class_constraint_hooks.append(hook)
    classes = pc.compiled(ssn)
    sched.close_session(ssn)
    plain = classes[0]
    assert plain.raw_width == 2 and plain.forbid[1] == 1
    got = pc.reference_mask(nt, plain)
    assert got == [i != 5 for i in range(64)]


# --------------------------------------------------------------------------
# through the scheduler
# --------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(pc.WORLDS))
def test_run_once_binds_exactly_the_feasible(name):
    w = world(name)
    _, binder, sched = pc.build(w)
    sched.run_once()
    binds = dict(binder.binds)
    assert 0 < len(binds) < len(w.pods)
    pc.check_binds(w, binds)


@pytest.mark.parametrize("pairs", [64, 128])
def test_selector_for_an_unknown_pair_at_a_word_boundary(pairs):
    """The registry holds an exact multiple of 64 pairs and a gang names a
    pair no node carries: its bit opens a new word.  The plain gang binds,
    the selector gang stays pending, nothing raises."""
    w = pc.boundary_world()
    if pairs == 128:
        for i, node in enumerate(w.nodes):
            node.meta.labels["slot"] = f"s{i}"
    assert pc.static_pairs(w.nodes) == pairs
    _, binder, sched = pc.build(w)
    sched.run_once()
    plain, picky = w.pods
    assert plain.meta.key in binder.binds
    assert picky.meta.key not in binder.binds
    pc.check_binds(w, dict(binder.binds))


@pytest.mark.parametrize("affinity", [{"in": {"zone": ["nowhere"]}},
                                      {"notIn": {"zone": ["nowhere"]}}],
                         ids=["in", "notIn"])
def test_affinity_for_an_unknown_pair_at_a_word_boundary(affinity):
    w = pc.boundary_world()
    w.pods[1] = pc.make_pod(w, random.Random(0), (), tolerations=[],
                            selector={}, affinity=affinity)
    _, binder, sched = pc.build(w)
    sched.run_once()
    pc.check_binds(w, dict(binder.binds))
    assert w.pods[0].meta.key in binder.binds
    assert (w.pods[1].meta.key in binder.binds) == ("notIn" in affinity)


# --------------------------------------------------------------------------
# per-node keys and the taint limit
# --------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hostname_session():
    w = pc.hostname_world()
    _, _, sched = pc.build(w)
    ssn, classes = open_and_compile(sched)
    return w, ssn, classes


def test_a_cluster_of_unique_hostnames_packs():
    w, ssn, classes = hostname_session()
    nt = ssn.node_tensors
    assert nt.n == 1100
    # three zone pairs and what the 40 pods named, not one bit per node
    assert len(nt.labels.index) < 200
    by_pod = {c.pod.meta.name: c for c in classes}
    one = pc.reference_mask(nt, by_pod[w.pods[0].meta.name])
    assert [n.meta.name for n, m in zip(w.nodes, one) if m] == ["n0777"]
    two = pc.reference_mask(nt, by_pod[w.pods[1].meta.name])
    assert [n.meta.name for n, m in zip(w.nodes, two) if not m] == \
        ["n0003", "n1099"]


def test_hostname_clauses_equal_the_evaluator():
    w, ssn, classes = hostname_session()
    masks = {p.meta.name: pc.mask(p, w.nodes) for p in w.pods}
    assert 2 * informative(w, masks) >= len(w.pods)
    assert_masks(w, ssn, classes, masks)


def test_the_65th_blocking_taint_overflows_and_says_so():
    """The taint word is one int64 in the kernel ABI: 64 distinct blocking
    taints pack (bit 63 included), one more is an error that names them.
    PreferNoSchedule taints take no bit."""
    from volcano_amd.api.info import NodeInfo
    from volcano_amd.api.objects import Taint
    from volcano_amd.api.resource import ResourceDims
    from volcano_amd.scheduler.tensors import NodeTensors
    w = world("taints64")
    nodes = [NodeInfo(n) for n in w.nodes]
    soft = NodeInfo(pc.synth.make_node("zz-soft", taints=[
        Taint("one-more", "", "PreferNoSchedule")]))
    nt = NodeTensors(ResourceDims())
    nt.pack(nodes + [soft])
    assert len(nt.taints.index) == 64
    assert int(nt.taints_np[63]) == -2 ** 63 and int(nt.taints_np[-1]) == 0
    extra = NodeInfo(pc.synth.make_node("zz-extra", taints=[
        Taint("one-more", "", "NoExecute")]))
    with pytest.raises(OverflowError, match="taints"):
        NodeTensors(ResourceDims()).pack(nodes + [extra])
