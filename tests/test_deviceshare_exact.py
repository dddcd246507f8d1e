"""Per-card packing of device-share slices (``deviceshare`` with ``exact:
true``) on the torch runner, and the closed form of the rule against the
per-pod ``GPUDevicePool`` oracle.  Integers only: every comparison is
equality."""

import numpy as np
import pytest
import torch

import _deviceshare_cases as dc
import _kernel_cases as kc
from volcano_amd.api.devices import ANN_ASSIGNED, DeviceRequest
from volcano_amd.ops import reference as ref

# what the commit before this feature binds in dc.run_cluster, recorded
# from it: every pod the cpu admits, the third 600-MiB pod of g0 and all
# eight 60 % slices of g2 (both of whose cards the ``ex`` pods own) without
# a card
PARENT_BINDS = {**{f"big-w-{i}": n for i, n in enumerate("00011")},
                "ex-w-0": "2", "ex-w-1": "2",
                **{f"vg-w-{i}": "2" for i in range(8)}}
PARENT_CARDS = {"big-w-0": "0", "big-w-1": "1", "big-w-2": None,
                "big-w-3": "0", "big-w-4": "1", "ex-w-0": "0", "ex-w-1": "1",
                **{f"vg-w-{i}": None for i in range(8)}}
PARENT_PLAN = [("default/big", 5, None, [1]), ("default/ex", 2, None, [2]),
               ("default/vg", 8, None, [4])]


def test_exact_packs_per_card_in_one_cycle():
    binds, anns, plans = dc.run_cluster(True)
    assert [p[:3] for p in plans[0]] == [
        ("default/big", 5, (1, 600, 0)), ("default/ex", 2, (1, 0, 0)),
        ("default/vg", 8, (1, 300, 60))]
    mem, cores, whole, pods = {}, {}, set(), {}
    for pod, node in binds.items():
        assert ANN_ASSIGNED in anns[pod], f"{pod} bound without a card"
        rq = DeviceRequest.from_annotations(anns[pod])
        for card in anns[pod][ANN_ASSIGNED].split(","):
            at = (node, card)
            mem[at] = mem.get(at, 0) + rq.memory
            cores[at] = cores.get(at, 0) + rq.cores
            pods[at] = pods.get(at, 0) + 1
            if rq.exclusive:
                whole.add(at)
    assert max(mem.values()) <= 1000 and max(cores.values()) <= 100
    assert whole and all(pods[at] == 1 for at in whole)
    # the cpu admits every pod; the cards leave one ex and three vg pending
    bound = [pod.split("-")[0] for pod in binds]
    assert {j: bound.count(j) for j in ("big", "ex", "vg")} == \
        {"big": 5, "ex": 1, "vg": 5}


@pytest.mark.parametrize("exact", [None, False])
def test_without_exact_plan_and_placements_are_the_parents(exact):
    binds, anns, plans = dc.run_cluster(exact)
    assert plans == [PARENT_PLAN]
    assert binds == {p: f"g{n}" for p, n in PARENT_BINDS.items()}
    assert {p: anns[p].get(ANN_ASSIGNED) for p in binds} == PARENT_CARDS


@pytest.mark.parametrize("request_", dc.REQUESTS, ids=str)
@pytest.mark.parametrize("K", [1, 3, 8, 16])
def test_closed_form_equals_per_pod_oracle(K, request_):
    case = dc.commit_case(20, K, request_, seed=K)
    got = {}
    for name, cap_fn, commit_fn in (
            ("oracle", ref.device_cap, ref.device_commit),
            ("closed", ref.device_cap_closed, ref.device_commit_closed)):
        planes = dc.planes_of(case)
        score, cap = (torch.from_numpy(case[k].copy())
                      for k in ("score", "cap"))
        cap_fn(score, cap, *planes, request_)
        assign = torch.zeros((20, K), dtype=torch.int32)
        commit_fn(torch.from_numpy(case["log_nodes"]),
                  torch.from_numpy(case["log_counts"]), torch.tensor(20),
                  *planes, assign, request_)
        cards = [ref.device_cards(assign[e].numpy(), int(c), request_[0])
                 for e, c in enumerate(case["log_counts"])]
        got[name] = [score.numpy().view(np.int32), cap.numpy(), assign.numpy(),
                     cards] + [p.numpy() for p in planes]
    assert (got["oracle"][1] < case["cap"]).any()       # the clamp bites
    for a, b in zip(got["oracle"], got["closed"]):
        assert np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


# ---- the integer limits: values near 2^28, sums above int32 ---------------

def per_pod(case, request):
    """cap, rows and planes of the per-pod oracles on a commit case."""
    cap = torch.from_numpy(case["cap"].copy())
    ref.device_cap(torch.from_numpy(case["score"].copy()), cap,
                   *dc.planes_of(case), request)
    planes = dc.planes_of(case)
    L = len(case["log_nodes"])
    rows = torch.zeros((L, case["state"].shape[0]), dtype=torch.int32)
    ref.device_commit(torch.from_numpy(case["log_nodes"]),
                      torch.from_numpy(case["log_counts"]), torch.tensor(L),
                      *planes, rows, request)
    return [cap.numpy(), rows.numpy()] + [p.numpy() for p in planes[:3]]


@pytest.mark.parametrize("request_", dc.REQUESTS, ids=str)
@pytest.mark.parametrize("K", [4, 5, 9, 16])
def test_per_pod_rule_is_scale_invariant(K, request_):
    """The link between the closed form at large values and the per-pod
    rule: memory scaled by 2^18 (1000 MiB cards stay below 2^28) changes
    no pick of ``GPUDevicePool.allocate``."""
    f = 1 << 18
    case = dc.commit_case(8, K, request_, seed=K)
    big = dict(case, mem_used=case["mem_used"] * f,
               mem_total=case["mem_total"] * f)
    assert big["mem_total"].dtype == np.int32 and \
        big["mem_total"].max() == 1000 * f < ref.DEV_MEM_LIMIT
    cap, rows, mu, cu, st = per_pod(case, request_)
    count, memory, cores = request_
    cap_f, rows_f, mu_f, cu_f, st_f = per_pod(big, (count, memory * f, cores))
    assert np.array_equal(cap, cap_f) and np.array_equal(rows, rows_f)
    assert np.array_equal(cu, cu_f) and np.array_equal(st, st_f)
    assert np.array_equal(mu.astype(np.int64) * f, mu_f)
    assert rows.any() == bool(case["log_counts"].any())


@pytest.mark.parametrize("name", list(dc.BIG_CARD_CASES))
def test_big_cases_agree_on_python_integers(name):
    """numpy's closed form and the plain-integer derivation agree, so no
    case of the family rests on a wrapped numpy value."""
    case, request, want = dc.big_card_case(name)
    got = dc.card_closed_py(case, request)
    for key in dc.CLOSED_KEYS:
        assert want[key] == got[key], key
    assert any(any(row) for row in want["rows"])
    assert want["cap"] != case["cap"].tolist()          # the clamp bites
    assert all(0 <= take <= dc.TOP and 0 <= card < 16
               for run in want["runs"] for card, take in run)


def test_top_case_holds_the_figures_it_exists_for():
    TOP = dc.TOP
    case, request, want = dc.big_card_case("top-7x1MiB")
    slots = ref.device_slots(*dc.planes_of(case), request)
    assert slots[:, 0].sum() == 2 ** 32 - 16            # S above int32
    assert slots[:, 1].sum() == 2 ** 32 - 16 - 120
    nodes, counts = case["log_nodes"].tolist(), case["log_counts"].tolist()
    assert want["cap"][1] == 613566737 and case["cap"][1] == dc.INT_MAX
    # node B, filled to the brim: cards 15 .. 0 in turn
    full = want["rows"][nodes.index(11)]
    assert full[:3] == [0xfffffff0, 0xeffffff1, 0xdffffff2]
    assert full[15] == TOP - 1          # card 0: one slice of S is left
    assert counts[nodes.index(11)] * 7 > 2 ** 31
    # fourteen whole cards and no more: the prefix is above 2^31
    for n in (5, 1, 2):
        run = want["runs"][nodes.index(n)]
        assert len(run) == 14 and sum(t for _, t in run[:13]) > 2 ** 31
        assert all(t == slots[k, n] for k, t in run)
    # S // 7 pods end mid-card; the zeroed entry takes nothing
    assert want["runs"][0][15] == (15, TOP - 2)
    assert counts[2] == 0 and not any(want["rows"][2])

    case, request, want = dc.big_card_case("top-1x1MiB")
    nodes = case["log_nodes"].tolist()
    assert want["rows"][nodes.index(3)] == [0xFFFFFFFF] + [0] * 15
    assert want["rows"][nodes.index(4)] == [0x8FFFFFFF] + [0] * 15
    assert want["runs"][0][8] == (8, 7)                 # 2^31 - 1 slices
    assert want["cap"][0] == dc.INT_MAX                 # S // 1 is above it


def differs(want, got, keys):
    return [key for key in keys if want[key] != got[key]]


@pytest.mark.parametrize("mutant", dc.MUTANTS)
def test_every_wrong_kernel_fails_a_big_case(mutant):
    """Each switch of ``card_closed_py`` emulates one wrong kernel (or one
    wrong host decode).  The big family catches every one of them.  The
    small-value family catches none of the int32 wraps and not the 24-bit
    mask; a decode that shifts the int32 passes wherever a word is decoded
    today (the whole-plan test, K = 4), though the K = 16 commit rows do
    hold negative words — as raw rows only."""
    killed = {}
    for name in dc.BIG_CARD_CASES:
        case, request, want = dc.big_card_case(name)
        keys = differs(want, dc.card_closed_py(case, request, mutant),
                       dc.CLOSED_KEYS)
        if keys:
            killed[name] = keys
    print(mutant, "caught by", killed)
    assert killed, mutant
    if mutant not in dc.WRAP_MUTANTS + ("mask-24", "decode-sign-extends"):
        return
    decode = mutant == "decode-sign-extends"
    negative = 0
    for K in (1, 3, 4, 8, 16):
        for request in dc.REQUESTS:
            case = dc.commit_case(20, K, request, seed=K)
            want = dc.card_closed(case, request)
            negative += any(w >> 31 for row in want["rows"] for w in row)
            if decode and K > 4:
                continue
            assert not differs(want, dc.card_closed_py(case, request, mutant),
                               dc.CLOSED_KEYS), (mutant, K, request)
    print(mutant, "passes the small-value family")
    assert negative


# ---- what the card planes may hold ----------------------------------------

def _plan_and_planes():
    case, _, _ = dc.device_plan_case()
    plan = kc.build_plan(case, "cpu")
    cards = dc.card_case(case.N, 4, 11)
    return plan, {k: cards[k].copy() for k in
                  ("mem_used", "cores_used", "state", "mem_total")}


@pytest.mark.parametrize("plane,value,text", [
    ("mem_used", -1, "mem_used"), ("mem_used", -2 ** 31, "mem_used"),
    ("cores_used", -1, "cores_used"), ("state", -1, "slice count"),
    ("state", 1 << 28, "slice count"),
    ("state", ref.DEV_GONE | 1 << 28, "slice count"),
    ("mem_total", 1 << 28, "mem_total"), ("mem_total", -1, "mem_total")])
def test_set_device_state_rejects_what_the_kernels_cannot_hold(plane, value,
                                                               text):
    plan, planes = _plan_and_planes()
    plan.set_device_state(**planes)
    planes[plane][..., 7] = value
    with pytest.raises(ValueError, match=text):
        plan.set_device_state(**planes)


def test_an_overfull_card_is_accepted_and_has_no_slot():
    plan, planes = _plan_and_planes()
    planes["mem_used"][0, :] = planes["mem_total"] + 1
    planes["mem_used"][1, :] = dc.INT_MAX
    planes["state"][:, :] = 1
    planes["state"][2, :] = ref.DEV_GONE | dc.TOP
    plan.set_device_state(**planes)
    slots = ref.device_slots(*(torch.from_numpy(planes[k]) for k in
                               ("mem_used", "cores_used", "state",
                                "mem_total")), (1, 1, 0))
    assert not slots[:3].any() and slots[3].any()
    for name in ("overfull-1", "overfull-2"):
        case, request, want = dc.big_card_case(name)
        over = case["mem_used"] > case["mem_total"][None, :]
        slots = ref.device_slots(*dc.planes_of(case), request)
        assert over.any() and not slots[over].any() and slots[~over].any()


@pytest.mark.parametrize("field,value", [
    ("mem_used", -1), ("cores_used", -5), ("slices", -1),
    ("slices", 1 << 28), ("mem_used", 1 << 31)])
def test_card_planes_leaves_such_a_pool_to_the_host_path(field, value):
    from types import SimpleNamespace
    from volcano_amd.api.devices import Card, GPUDevicePool
    from volcano_amd.scheduler.plugins.deviceshare import card_planes
    pools = {}
    for name in ("a", "b"):
        pools[name] = GPUDevicePool.__new__(GPUDevicePool)
        pools[name].cards = [Card(k, 1000, 200 * k, 10 * k, False, k)
                             for k in range(3)]
    nodes = {name: SimpleNamespace(node_id=i) for i, name in enumerate("ab")}
    planes = card_planes(pools, nodes, 2)
    assert planes is not None and planes[0].tolist() == [[0, 0], [200, 200],
                                                         [400, 400]]
    pools["a"].cards[2].mem_used = dc.INT_MAX           # over-full: fine
    assert card_planes(pools, nodes, 2)[0][2, 0] == dc.INT_MAX
    setattr(pools["b"].cards[1], field, value)
    assert card_planes(pools, nodes, 2) is None
