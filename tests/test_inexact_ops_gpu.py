"""Kernel against kernel on inexact inputs, and the exact discard.

No oracle and no tolerance here.  ``node_score_one`` is inlined into five
kernels and the device compiler contracts ``a*b+c`` per inlining context;
on the exact inputs of ``test_ops_gpu_edges.py`` a disagreement between two
inlinings is invisible by construction.  On an inexact state, with the
balanced-allocation term on and off:

* ``fused_score_select`` must equal ``score_cap`` + ``select_commit``: log,
  counters, usage and the score plane;
* ``select_commit`` with and without sort scratch must leave bit-equal
  usage although every ``used += count * req`` rounds;
* a single-class gang that misses its minimum leaves ``used`` and
  ``queue_alloc`` with the bits they had, in every select, at byte-scale
  magnitudes where f32 add-then-subtract would not;
* a multi-class discard (``cond_revert``) still subtracts: its residue is
  bounded by one ulp of the staged value.
"""

import numpy as np
import pytest
import torch

import _kernel_cases as kc
import test_ops_gpu_edges as edges

pytestmark = pytest.mark.gpu

DEV = "cuda"
NEG_INF = float("-inf")
NOLIMIT = 1.0e18


@pytest.fixture(scope="module")
def hip():
    from volcano_amd.ops import hip as h
    h._load()
    return h


def gpu_fused(hip, st, ntasks, used0, qa0, ql, jp0, fuse_min, *, tolerated,
              require, forbid, w_least, w_most, w_bal, bias):
    N = st["alloc"].shape[0]
    K = max(1, min(ntasks, N))
    used_t = used0.t().contiguous().clone().to(DEV)
    qa = qa0.clone().to(DEV)
    score = torch.full((N,), 7.0, device=DEV)
    cap = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    ln = torch.zeros(K, dtype=torch.int32, device=DEV)
    lc = torch.zeros(K, dtype=torch.int32, device=DEV)
    ll = torch.full((1,), -3, dtype=torch.int32, device=DEV)
    pl = torch.full((1,), -3, dtype=torch.int32, device=DEV)
    jp = torch.full((1,), jp0, dtype=torch.int32, device=DEV)
    hip.fused_score_select(
        st["alloc"].t().contiguous().to(DEV), used_t,
        st["extra"].t().contiguous().to(DEV),
        st["ready"].to(torch.uint8).to(DEV), st["taints"].to(DEV),
        st["planes"].t().contiguous().to(DEV), st["req"].to(DEV), tolerated,
        require.to(DEV), forbid.to(DEV), w_least, w_most, w_bal,
        st["dim_w"].to(DEV), None if bias is None else bias.to(DEV), score,
        cap, ntasks, qa, ql.to(DEV), ln, lc, ll, pl, jp, fuse_min)
    torch.cuda.synchronize()
    return dict(ln=ln.cpu(), lc=lc.cpu(), ll=int(ll.cpu()), pl=int(pl.cpu()),
                jp=int(jp.cpu()), used=used_t.t().cpu(), qa=qa.cpu(),
                score=score.cpu(), cap=cap.cpu())


def same_select_bits(a, b, what):
    edges.same_select(a, b, what)
    assert kc.same_bits(a["used"], b["used"]), f"{what}: used bits"
    assert kc.same_bits(a["qa"], b["qa"]), f"{what}: queue_alloc bits"
    assert torch.equal(a["ln"], b["ln"]) and torch.equal(a["lc"], b["lc"])


# --------------------------------------------------------------------------
# fused_score_select == score_cap + select_commit
# --------------------------------------------------------------------------

@pytest.mark.parametrize("w_bal", [0.0, 1.0])
@pytest.mark.parametrize("N", [63, 1000, 4096])
def test_fused_equals_split_on_inexact_state(hip, N, w_bal):
    R, W = 6, 2
    st = kc.dyadic_state(N, R, W, seed=N + 1, inexact=True)
    tol, require, forbid = edges._class_masks(W, N)
    used0 = st["used"]
    qa0 = torch.arange(1, R + 1).float()
    jp0 = 4
    logged = 0
    for bias in (None, st["bias"]):
        kw = dict(tolerated=tol, require=require, forbid=forbid, w_least=0.5,
                  w_most=2.0, w_bal=w_bal, bias=bias)
        s_g, cap_g = edges.gpu_score_cap(hip, st, **kw)
        # the kernel really rounds here: not the float64 formula's bits
        feas = s_g > NEG_INF
        assert bool(feas.any())
        for ntasks, q, fuse_min in ((0, None, -1), (40, None, -1),
                                    (40, 25, 26), (511, None, 0)):
            ql = torch.full((R,), NOLIMIT)
            if q is not None:
                ql[0] = qa0[0] + q
            split = edges.gpu_select(hip, s_g, cap_g, st["req"], ntasks,
                                     used0, qa0, ql, jp0, fuse_min)
            fused = gpu_fused(hip, st, ntasks, used0, qa0, ql, jp0, fuse_min,
                              **kw)
            what = f"N={N} w_bal={w_bal} ntasks={ntasks} q={q}"
            same_select_bits(split, fused, what)
            assert torch.equal(fused["cap"], cap_g), what
            # consumed nodes are knocked out of the plane, nothing else:
            # with ntasks == 0 the plane is score_cap's, bit for bit
            after = s_g.clone()
            after[split["ln"][:split["ll"]].long()] = NEG_INF
            assert kc.same_bits(fused["score"], after), f"{what}: plane"
            if ntasks == 0:
                assert split["ll"] == 0
                assert kc.same_bits(fused["score"], s_g)
            logged += split["ll"]
    assert logged > 20


# --------------------------------------------------------------------------
# select_commit: serial == sort-based although the usage update rounds
# --------------------------------------------------------------------------

@pytest.mark.parametrize("N", [512, 1025])
def test_bulk_equals_serial_when_usage_rounds(hip, N):
    R = 5
    st = kc.dyadic_state(N, R, 1, seed=N, inexact=True)
    score, cap = kc.oracle_score_cap(st, tolerated=-1, w_least=0.5,
                                     w_most=2.0, w_bal=1.0, bias=st["bias"])
    g = torch.Generator().manual_seed(N)
    req = torch.randint(1, 30, (R,), generator=g).float() * 0.1
    used0 = torch.randint(0, 500, (N, R), generator=g).float() * 0.1
    qa0 = torch.randint(1, 200, (R,), generator=g).float() * 0.1
    ql = torch.full((R,), NOLIMIT)
    ntasks = 600
    # the update really rounds: for a good share of (node, dim) the exact
    # used + count * req is no f32 number
    feas = (score > NEG_INF).numpy()
    exact = used0.double().numpy()[feas] + cap.double().numpy()[feas, None] \
        * req.double().numpy()[None, :]
    assert (exact.astype(np.float32).astype(np.float64) != exact).mean() > 0.25
    total = None
    for fuse_min in (-1, 0, 10 ** 6):
        serial = edges.gpu_select(hip, score, cap, req, ntasks, used0, qa0,
                                  ql, 3, fuse_min)
        bulk = edges.gpu_select(hip, score, cap, req, ntasks, used0, qa0, ql,
                                3, fuse_min, bulk=True)
        same_select_bits(serial, bulk, f"N={N} fuse={fuse_min}")
        if fuse_min == -1:
            total = serial["pl"]
            room = int(cap[score > NEG_INF].to(torch.int64).sum())
            assert total == min(ntasks, room) and serial["ll"] > 100
            assert not kc.same_bits(serial["used"], used0)
        if fuse_min == 10 ** 6:
            assert serial["pl"] == 0
            assert kc.same_bits(serial["used"], used0)
            assert kc.same_bits(serial["qa"], qa0)


# --------------------------------------------------------------------------
# a discarded single-class gang leaves no trace
# --------------------------------------------------------------------------

def _no_trace(got, used0, qa0, jp0, what):
    assert got["pl"] == 0 and got["jp"] == jp0, f"{what}: counters"
    assert got["ll"] > 0, f"{what}: nothing was logged"
    assert int(got["lc"].abs().sum()) == 0, f"{what}: log counts"
    assert kc.same_bits(got["used"], used0), f"{what}: used changed"
    assert kc.same_bits(got["qa"], qa0), f"{what}: queue_alloc changed"


@pytest.mark.parametrize("N,R,seed", kc.BYTE_SELECT_SHAPES)
def test_discarded_select_leaves_no_trace(hip, N, R, seed):
    inp = kc.byte_select_inputs(N, R, seed)
    ql = torch.full((R,), NOLIMIT)
    jp0 = 5
    for ntasks, bulk in zip(kc.BYTE_SELECT_TASKS, (False, True)):
        nodes, counts, placed = kc.select_log(inp, ntasks)
        # precondition, in numpy: add-then-subtract would not come back
        res = kc.select_residues(inp["used"], inp["req"], nodes, counts)
        assert min(res) >= 1, res
        got = edges.gpu_select(hip, inp["score"], inp["cap"], inp["req"],
                               ntasks, inp["used"], inp["qa"], ql, jp0,
                               placed + 1, bulk=bulk)
        assert got["ln"][:got["ll"]].tolist() == nodes.tolist()
        _no_trace(got, inp["used"], inp["qa"], jp0,
                  f"select ntasks={ntasks} bulk={bulk}")
        # the same class commits when its minimum is what can be placed
        kept = edges.gpu_select(hip, inp["score"], inp["cap"], inp["req"],
                                ntasks, inp["used"], inp["qa"], ql, jp0,
                                placed, bulk=bulk)
        assert kept["pl"] == placed and kept["jp"] == jp0 + placed
        assert kept["lc"][:kept["ll"]].tolist() == counts.tolist()


@pytest.mark.parametrize("N,R,seed", kc.BYTE_SELECT_SHAPES)
def test_discarded_spread_select_leaves_no_trace(hip, N, R, seed):
    inp = kc.byte_select_inputs(N, R, seed)
    ntasks, D = 60, 8
    K = max(1, min(ntasks, N))
    used_t = inp["used"].t().contiguous().clone().to(DEV)
    qa = inp["qa"].clone().to(DEV)
    ln = torch.zeros(K, dtype=torch.int32, device=DEV)
    lc = torch.zeros(K, dtype=torch.int32, device=DEV)
    ll = torch.full((1,), -3, dtype=torch.int32, device=DEV)
    pl = torch.full((1,), -3, dtype=torch.int32, device=DEV)
    jp = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    dom_of = (torch.arange(N, dtype=torch.int32) % D).to(DEV)
    cnt = torch.zeros(D, dtype=torch.int32, device=DEV)
    # maxSkew 2: the fill really interleaves domains; ntasks + 1 can never
    # be placed
    hip.spread_select(inp["score"].clone().to(DEV), inp["cap"].clone().to(DEV),
                      inp["req"].to(DEV), ntasks, used_t, qa,
                      torch.full((R,), NOLIMIT).to(DEV), ln, lc, ll, pl, jp,
                      dom_of, cnt, 2, ntasks + 1)
    torch.cuda.synchronize()
    got = dict(ln=ln.cpu(), lc=lc.cpu(), ll=int(ll.cpu()), pl=int(pl.cpu()),
               jp=int(jp.cpu()), used=used_t.t().cpu(), qa=qa.cpu())
    _no_trace(got, inp["used"], inp["qa"], 5, "spread")
    assert got["ll"] >= D and int(cnt.cpu().abs().sum()) == 0


@pytest.mark.parametrize("N,R", [(100, 1), (1025, 6)])
def test_discarded_fused_select_leaves_no_trace(hip, N, R):
    st = kc.byte_state(N, R, seed=N + R)
    tol = -1
    zw = torch.zeros(1, dtype=torch.int64)
    kw = dict(tolerated=tol, require=zw, forbid=zw, w_least=0.5, w_most=2.0,
              w_bal=1.0, bias=st["bias"])
    g = torch.Generator().manual_seed(N)
    qa0 = torch.randint(1, 20, (R,), generator=g).float()
    qa0[0] = 37 * 7.0e8 + 11 * 1.5e9
    ql = torch.full((R,), NOLIMIT)
    ntasks, jp0 = 500, 5
    kept = gpu_fused(hip, st, ntasks, st["used"], qa0, ql, jp0, -1, **kw)
    m, placed = kept["ll"], kept["pl"]
    assert m > 1 and placed > 0
    res = kc.select_residues(st["used"], st["req"],
                             kept["ln"][:m].long().numpy(),
                             kept["lc"][:m].numpy())
    assert min(res) >= 1, res
    assert not kc.same_bits(kept["used"], st["used"])
    got = gpu_fused(hip, st, ntasks, st["used"], qa0, ql, jp0, placed + 1,
                    **kw)
    assert got["ln"][:m].tolist() == kept["ln"][:m].tolist()
    _no_trace(got, st["used"], qa0, jp0, "fused")


# --------------------------------------------------------------------------
# multi-class gangs still discard by subtraction: bounded residue
# --------------------------------------------------------------------------

@pytest.mark.parametrize("N,R,seed", kc.BYTE_SELECT_SHAPES)
def test_cond_revert_residue_is_bounded(hip, N, R, seed):
    """select_commit, then cond_revert with flag 0 (what a failed multi-
    class gang does).  Each element went through two roundings of at most
    half an ulp of the staged value: |after - before| <= ulp(before +
    count * req)."""
    inp = kc.byte_select_inputs(N, R, seed)
    ntasks = 600
    K = max(1, min(ntasks, N))
    used0, qa0, req = inp["used"], inp["qa"], inp["req"]
    used_t = used0.t().contiguous().clone().to(DEV)
    qa = qa0.clone().to(DEV)
    ln = torch.zeros(K, dtype=torch.int32, device=DEV)
    lc = torch.zeros(K, dtype=torch.int32, device=DEV)
    ll = torch.zeros(1, dtype=torch.int32, device=DEV)
    pl = torch.zeros(1, dtype=torch.int32, device=DEV)
    jp = torch.full((1,), 5, dtype=torch.int32, device=DEV)
    hip.select_commit(inp["score"].clone().to(DEV), inp["cap"].to(DEV),
                      req.to(DEV), ntasks, used_t, qa,
                      torch.full((R,), NOLIMIT).to(DEV), ln, lc, ll, pl, jp,
                      -1)
    torch.cuda.synchronize()
    m, placed = int(ll.cpu()), int(pl.cpu())
    nodes, counts = ln.cpu()[:m].long().numpy(), lc.cpu()[:m].numpy()
    assert placed == min(ntasks, inp["room"]) and m > 10
    hip.cond_revert(torch.zeros(1, dtype=torch.uint8, device=DEV), ln, lc, ll,
                    req.to(DEV), used_t, qa, pl, jp)
    torch.cuda.synchronize()
    assert int(pl.cpu()) == 0 and int(jp.cpu()) == 5
    assert int(lc.cpu().abs().sum()) == 0
    after = used_t.t().cpu().numpy().astype(np.float64)
    before = used0.numpy().astype(np.float64)
    staged = before.copy()
    staged[nodes] += counts[:, None] * req.double().numpy()[None, :]
    bound = kc.ulp_f32(staged.astype(np.float32)).astype(np.float64)
    untouched = np.ones(N, dtype=bool)
    untouched[nodes] = False
    assert np.array_equal(after[untouched], before[untouched])
    diff = np.abs(after - before)
    print("largest residue / bound:", float((diff / bound).max()),
          "elements off:", int((diff > 0).sum()))
    assert (diff <= bound).all()
    q_before = qa0.double().numpy()
    q_bound = kc.ulp_f32((q_before + placed * req.double().numpy())
                         .astype(np.float32)).astype(np.float64)
    assert (np.abs(qa.cpu().double().numpy() - q_before) <= q_bound).all()
