"""HIP kernels vs the torch oracle at the edges: every branch of every
kernel, at the smallest shapes that reach it.

Inputs come from ``_kernel_cases.dyadic_state``: every f32 operation of the
score is exact there, so scores, capacities, feasibility and logs must be
BIT-equal to ``reference.py`` (FMA contraction cannot hide behind a
tolerance, and the large natural tie groups pin the lowest-index rule and
the log order).  Only the balanced-allocation term (a square root) is
compared with the float64 formula under a measured tolerance.
"""

import numpy as np
import pytest
import torch

import _kernel_cases as kc

pytestmark = pytest.mark.gpu

ref = pytest.importorskip("volcano_amd.ops.reference")

DEV = "cuda"
NEG_INF = float("-inf")
INT32_MAX = 2 ** 31 - 1
NOLIMIT = 1.0e18
ALL_BITS = -1


@pytest.fixture(scope="module")
def hip():
    from volcano_amd.ops import hip as h
    h._load()
    return h


def _sync():
    if DEV == "cuda":
        torch.cuda.synchronize()


# --------------------------------------------------------------------------
# score_cap
# --------------------------------------------------------------------------

def gpu_score_cap(hip, st, *, req=None, tolerated=0, require=None,
                  forbid=None, w_least=1.0, w_most=0.0, w_bal=0.0, bias=None,
                  extra="tensor"):
    N, R = st["alloc"].shape
    W = st["planes"].shape[1]
    zw = torch.zeros(W, dtype=torch.int64)
    extra_t = {"tensor": st["extra"].t().contiguous().to(DEV),
               "zeros": torch.zeros(R, N, device=DEV),
               "null": None}[extra]
    score = torch.full((N,), 7.0, device=DEV)
    cap = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    hip.score_cap(
        st["alloc"].t().contiguous().to(DEV),
        st["used"].t().contiguous().to(DEV), extra_t,
        st["ready"].to(torch.uint8).to(DEV), st["taints"].to(DEV),
        st["planes"].t().contiguous().to(DEV),
        (st["req"] if req is None else req).to(DEV), tolerated,
        (zw if require is None else require).to(DEV),
        (zw if forbid is None else forbid).to(DEV),
        w_least, w_most, w_bal, st["dim_w"].to(DEV),
        None if bias is None else bias.to(DEV), score, cap)
    _sync()
    return score.cpu(), cap.cpu()


def check_score_cap(hip, st, **kw):
    """Kernel vs oracle on one state: feasibility and capacity bit-equal;
    score bit-equal when w_bal == 0, else within the measured bound of the
    float64 formula."""
    s_c, cap_c = kc.oracle_score_cap(st, **kw)
    s_g, cap_g = gpu_score_cap(hip, st, **kw)
    feas = s_c > NEG_INF
    assert torch.equal(feas, s_g > NEG_INF), "feasibility mask"
    assert torch.equal(cap_c, cap_g), "capacity"
    if kw.get("w_bal", 0.0) == 0.0:
        assert kc.same_bits(s_c, s_g), "score bits"
    elif bool(feas.any()):
        want = kc.score_f64(st, req=kw.get("req"), w_least=kw["w_least"],
                            w_most=kw["w_most"], w_bal=kw["w_bal"],
                            bias=kw.get("bias"))
        err = float(np.abs(s_g.double().numpy() - want)[feas.numpy()].max())
        print(f"w_bal score error vs float64: {err:.3e}")
        # the f32 CPU oracle is off by at most 1.33e-7 (kc.BAL_ERR_F32,
        # re-measured by test_kernel_cases.py) on these inputs; the kernel
        # runs the same operation count and FMA only removes roundings,
        # so it gets 4x that
        assert err <= 4 * kc.BAL_ERR_F32, err
    return s_c, cap_c


def _class_masks(W, seed):
    rng = np.random.RandomState(seed)
    require = torch.zeros(W, dtype=torch.int64)
    forbid = torch.zeros(W, dtype=torch.int64)
    require[rng.randint(0, W)] = 4
    forbid[rng.randint(0, W)] = int(kc.BIT62)
    return int(np.int64(1) | kc.BIT63), require, forbid


@pytest.mark.parametrize("R,W", kc.SCORE_RW)
@pytest.mark.parametrize("N", kc.SCORE_NS)
def test_score_cap_small_shapes(hip, N, R, W):
    st = kc.dyadic_state(N, R, W, seed=N % 3)
    tol, require, forbid = _class_masks(W, N + R)
    for bias in (None, st["bias"]):
        for wl, wm in kc.SCORE_WEIGHTS:
            for wb in (0.0, kc.W_BAL):
                check_score_cap(hip, st, tolerated=tol, require=require,
                                forbid=forbid, w_least=wl, w_most=wm,
                                w_bal=wb, bias=bias)
    # extra == nullptr must equal a plane of zeros, bit for bit
    s0, c0 = gpu_score_cap(hip, st, tolerated=ALL_BITS, extra="null",
                           bias=st["bias"], w_most=2.0)
    s1, c1 = gpu_score_cap(hip, st, tolerated=ALL_BITS, extra="zeros",
                           bias=st["bias"], w_most=2.0)
    s2, c2 = kc.oracle_score_cap(st, tolerated=ALL_BITS, extra=False,
                                 bias=st["bias"], w_most=2.0)
    assert kc.same_bits(s0, s1) and torch.equal(c0, c1)
    assert kc.same_bits(s0, s2) and torch.equal(c0, c2)


def test_score_cap_grid_stride_wraps(hip):
    """N one past 4096 blocks x 256 threads: the first 77 threads take a
    second node."""
    N, R, W = kc.GRID_WRAP
    st = kc.dyadic_state(N, R, W, seed=0)
    s, _ = check_score_cap(hip, st, tolerated=ALL_BITS, bias=st["bias"],
                           w_least=0.5, w_most=2.0)
    assert bool((s[4096 * 256:] > NEG_INF).any())
    check_score_cap(hip, st, tolerated=ALL_BITS, w_least=1.0, w_most=0.0,
                    w_bal=kc.W_BAL)


def _edge_state(alloc, used, req):
    alloc = torch.tensor(alloc, dtype=torch.float32)
    N, R = alloc.shape
    return dict(alloc=alloc, used=torch.tensor(used, dtype=torch.float32),
                extra=torch.zeros(N, R), ready=torch.ones(N, dtype=torch.bool),
                taints=torch.zeros(N, dtype=torch.int64),
                planes=torch.zeros(N, 1, dtype=torch.int64),
                req=torch.tensor(req, dtype=torch.float32),
                dim_w=torch.tensor([1.0, 1.0]))


def test_score_cap_capacity_edges(hip):
    # dim 0 is the one under test; dim 1 is roomy
    alloc = [[8192, 64], [8192, 64], [8192, 64], [4, 64], [4, 64],
             [0, 64], [16, 64], [16, 0], [16, 0]]
    used = [[192, 0], [193, 0], [8192, 0], [1, 0], [2, 0],
            [0, 0], [17, 0], [0, 0], [0, 2]]
    st = _edge_state(alloc, used, [1000.0, 0.0])
    s, cap = check_score_cap(hip, st, w_most=1.0)
    # avail == 8*req -> 8 (the +EPS slack decides); one less -> 7; 0 -> out
    assert cap.tolist()[:3] == [8, 7, 0]
    assert s[2] == NEG_INF
    assert cap.tolist()[3:] == [0] * 6 and bool((s[3:] == NEG_INF).all())

    # small exact multiples and the multiple-minus-one, alloc == 0,
    # used > alloc; on a dim nobody asks for alloc == 0 is harmless but
    # used > alloc still rules the node out (the fit test covers every dim)
    st = _edge_state(alloc, used, [1.0, 0.0])
    s, cap = check_score_cap(hip, st, w_most=1.0)
    assert cap.tolist() == [8000, 7999, 0, 3, 2, 0, 0, 16, 0]
    assert bool((s[[5, 6, 8]] == NEG_INF).all()) and s[7] > NEG_INF

    st = _edge_state(alloc, used, [3.0, 0.0])
    _, cap = check_score_cap(hip, st, w_least=1.0)
    assert cap.tolist() == [2666, 2666, 0, 1, 0, 0, 0, 5, 0]

    # nothing requested: unbounded capacity wherever nothing is over-used
    st = _edge_state(alloc, used, [0.0, 0.0])
    s, cap = check_score_cap(hip, st, w_least=1.0)
    big = 2 ** 30
    assert cap.tolist() == [big] * 6 + [0, big, 0]
    assert (s > NEG_INF).tolist() == [True] * 6 + [False, True, False]

    # a request just above EPS against a huge node: the clamp before the
    # integer cast
    st = _edge_state([[2.0 ** 40, 64], [2.0 ** 30, 64], [1.0, 64]],
                     [[0, 0], [0, 0], [0, 0]], [2.0e-4, 0.0])
    _, cap = check_score_cap(hip, st, w_least=1.0)
    assert cap.tolist()[:2] == [2 ** 30, 2 ** 30] and 0 < cap[2] < 2 ** 30

    # non-integer exact multiple: 3 x 0.3 in f32
    third = float(np.float32(0.3))
    st = _edge_state([[float(np.float32(third * 3)), 64], [1.5, 64]],
                     [[0, 0], [0, 0]], [third, 0.0])
    check_score_cap(hip, st, w_least=1.0)


def test_score_cap_mask_bits_62_and_63(hip):
    b62, b63 = int(kc.BIT62), int(kc.BIT63)
    node_bits = [0, 1, b62, b63, b62 | b63, b63 | 1]
    N = len(node_bits) ** 2
    taints = torch.tensor([t for t in node_bits for _ in node_bits],
                          dtype=torch.int64)
    planes = torch.tensor([[p] for _ in node_bits for p in node_bits],
                          dtype=torch.int64)
    st = dict(alloc=torch.full((N, 1), 16.0), used=torch.zeros(N, 1),
              extra=torch.zeros(N, 1), ready=torch.ones(N, dtype=torch.bool),
              taints=taints, planes=planes, req=torch.ones(1),
              dim_w=torch.ones(1))
    m64 = (1 << 64) - 1
    seen = set()
    for tol in (0, b62, b63, b62 | b63, ALL_BITS):
        for require in (0, b62, b63, b62 | b63):
            for forbid in (0, b62, b63):
                s, _ = check_score_cap(
                    hip, st, tolerated=tol,
                    require=torch.tensor([require], dtype=torch.int64),
                    forbid=torch.tensor([forbid], dtype=torch.int64))
                # independent of torch's signed-word arithmetic
                want = [((t & m64) & ~(tol & m64)) == 0
                        and ((p & m64) & (require & m64)) == (require & m64)
                        and ((p & m64) & (forbid & m64)) == 0
                        for t, p in zip(taints.tolist(),
                                        planes[:, 0].tolist())]
                assert (s > NEG_INF).tolist() == want, (tol, require, forbid)
                seen.add(tuple(want))
    assert len(seen) > 20


def test_score_cap_nothing_ready(hip):
    st = kc.dyadic_state(257, 6, 2, seed=1)
    st["ready"] = torch.zeros(257, dtype=torch.bool)
    s, cap = check_score_cap(hip, st, tolerated=ALL_BITS, bias=st["bias"])
    assert bool((s == NEG_INF).all()) and int(cap.abs().sum()) == 0


# --------------------------------------------------------------------------
# select_commit: serial and bulk
# --------------------------------------------------------------------------

def int_state(N, R, seed):
    """Non-zero integer-valued starting usage / queue / job counters: every
    add and subtract of count x req stays exact in f32."""
    g = torch.Generator().manual_seed(seed)
    used = torch.randint(0, 50, (N, R), generator=g).float()
    qa = torch.randint(1, 20, (R,), generator=g).float()
    return used, qa, 5


def int_req(R, seed):
    g = torch.Generator().manual_seed(seed + 77)
    req = torch.randint(0, 4, (R,), generator=g).float()
    req[0] = 1.0
    return req


def oracle_select(score, cap, req, ntasks, used0, qa0, ql, jp0, fuse_min):
    N = score.shape[0]
    K = max(1, min(ntasks, N))
    used, qa = used0.clone(), qa0.clone()
    ln = torch.zeros(K, dtype=torch.int32)
    lc = torch.zeros(K, dtype=torch.int32)
    ll = torch.zeros((), dtype=torch.int32)
    pl = torch.zeros((), dtype=torch.int32)
    jp = torch.tensor(jp0, dtype=torch.int32)
    ref.select_commit(score.clone(), cap, req, ntasks, used, qa, ql, ln, lc,
                      ll, pl, jp)
    if fuse_min >= 0 and int(pl) < fuse_min:
        ref.cond_revert(torch.zeros((), dtype=torch.uint8), ln, lc, ll, req,
                        used, qa, pl, jp)
    return dict(ln=ln, lc=lc, ll=int(ll), pl=int(pl), jp=int(jp), used=used,
                qa=qa)


def gpu_select(hip, score, cap, req, ntasks, used0, qa0, ql, jp0, fuse_min,
               bulk=False):
    N = score.shape[0]
    K = max(1, min(ntasks, N))
    used_t = used0.t().contiguous().clone().to(DEV)
    qa = qa0.clone().to(DEV)
    ln = torch.zeros(K, dtype=torch.int32, device=DEV)
    lc = torch.zeros(K, dtype=torch.int32, device=DEV)
    ll = torch.full((1,), -3, dtype=torch.int32, device=DEV)
    pl = torch.full((1,), -3, dtype=torch.int32, device=DEV)
    jp = torch.full((1,), jp0, dtype=torch.int32, device=DEV)
    scratch = torch.empty(4 * N, dtype=torch.int32, device=DEV) \
        if bulk else None
    hip.select_commit(score.clone().to(DEV), cap.to(DEV), req.to(DEV),
                      ntasks, used_t, qa, ql.to(DEV), ln, lc, ll, pl, jp,
                      fuse_min, sort_scratch=scratch)
    _sync()
    return dict(ln=ln.cpu(), lc=lc.cpu(), ll=int(ll.cpu()), pl=int(pl.cpu()),
                jp=int(jp.cpu()), used=used_t.t().cpu(), qa=qa.cpu())


def same_select(want, got, what):
    m = want["ll"]
    assert got["ll"] == m, f"{what}: log_len {got['ll']} vs {m}"
    # exact ORDER, entry for entry
    assert got["ln"][:m].tolist() == want["ln"][:m].tolist(), f"{what}: nodes"
    assert got["lc"][:m].tolist() == want["lc"][:m].tolist(), f"{what}: counts"
    assert got["pl"] == want["pl"], f"{what}: placed"
    assert got["jp"] == want["jp"], f"{what}: job_placed"
    assert torch.equal(got["used"], want["used"]), f"{what}: used"
    assert torch.equal(got["qa"], want["qa"]), f"{what}: queue_alloc"


def check_select(hip, score, cap, req, ntasks, used0, qa0, ql, jp0, fuse_min,
                 bulk=False, what=""):
    want = oracle_select(score, cap, req, ntasks, used0, qa0, ql, jp0,
                         fuse_min)
    got = gpu_select(hip, score, cap, req, ntasks, used0, qa0, ql, jp0,
                     fuse_min)
    same_select(want, got, f"serial {what}")
    if bulk:
        got_b = gpu_select(hip, score, cap, req, ntasks, used0, qa0, ql, jp0,
                           fuse_min, bulk=True)
        same_select(want, got_b, f"bulk {what}")
        same_select(got, got_b, f"bulk vs serial {what}")
    if fuse_min >= 0 and want["pl"] < fuse_min and fuse_min > 0:
        # reverted: the non-zero starting state comes back exactly
        assert torch.equal(got["used"], used0) and torch.equal(got["qa"], qa0)
        assert got["jp"] == jp0 and got["pl"] == 0
        assert int(got["lc"].abs().sum()) == 0
    return want


def dyadic_scores(N, R, seed):
    """Scores and capacities of a dyadic state: exact, with tie groups."""
    st = kc.dyadic_state(N, R, 1, seed)
    req = st["req"]
    score, cap = kc.oracle_score_cap(st, tolerated=ALL_BITS, w_most=1.0,
                                     bias=st["bias"])
    return score, cap, req


@pytest.mark.parametrize("R", [1, 6, 64])
@pytest.mark.parametrize("N", [1, 100, 1023, 1024, 1025, 3000])
def test_serial_select_exact_order(hip, N, R):
    score, cap, req = dyadic_scores(N, R, seed=N + R)
    if N == 1:                       # the single node must be usable
        score, cap = torch.tensor([0.5]), torch.tensor([3], dtype=torch.int32)
    used0, qa0, jp0 = int_state(N, R, N)
    ql = torch.full((R,), NOLIMIT)
    room = int(cap[score > NEG_INF].to(torch.int64).sum())
    assert room > 0
    for ntasks in (0, 1, room, room + 1):
        want = check_select(hip, score, cap, req, ntasks, used0, qa0, ql,
                            jp0, -1, what=f"ntasks={ntasks}")
        total = want["pl"]
        assert total == min(ntasks, room)
        for fuse_min in (0, total, total + 1):
            check_select(hip, score, cap, req, ntasks, used0, qa0, ql, jp0,
                         fuse_min, what=f"ntasks={ntasks} fuse={fuse_min}")
    if N >= 100:
        # the log really has index-ordered ties in it
        want = oracle_select(score, cap, req, room, used0, qa0, ql, jp0, -1)
        s = score[want["ln"][:want["ll"]].long()]
        assert int((s[1:] == s[:-1]).sum()) >= 3


@pytest.mark.parametrize("N", [1, 100, 1025])
def test_serial_select_all_equal_and_all_infeasible(hip, N):
    R = 6
    req = int_req(R, N)
    used0, qa0, jp0 = int_state(N, R, N + 1)
    ql = torch.full((R,), NOLIMIT)
    g = torch.Generator().manual_seed(N)
    cap = torch.randint(1, 4, (N,), generator=g).to(torch.int32)
    same = torch.full((N,), 0.5)
    for ntasks in (1, N // 2 + 1, int(cap.sum())):
        want = check_select(hip, same, cap, req, ntasks, used0, qa0, ql, jp0,
                            -1, what="all equal")
        m = want["ll"]
        assert want["ln"][:m].tolist() == list(range(m))     # index order
    none = torch.full((N,), NEG_INF)
    for fuse_min in (-1, 0, 1):
        want = check_select(hip, none, torch.zeros(N, dtype=torch.int32), req,
                            5, used0, qa0, ql, jp0, fuse_min,
                            what="all -inf")
        assert want["ll"] == 0 and want["pl"] == 0


@pytest.mark.parametrize("N,R", [(100, 6), (1025, 1), (1025, 64)])
def test_serial_select_quota(hip, N, R):
    score, cap, req = dyadic_scores(N, R, seed=N + R + 1)
    used0, qa0, jp0 = int_state(N, R, N + 2)
    ntasks = 400
    # quota exactly 0: the limit equals what the queue already holds
    ql = torch.full((R,), NOLIMIT)
    ql[0] = qa0[0]
    want = check_select(hip, score, cap, req, ntasks, used0, qa0, ql, jp0, -1,
                        what="quota 0")
    assert want["pl"] == 0 and want["ll"] == 0
    check_select(hip, score, cap, req, ntasks, used0, qa0, ql, jp0, 1,
                 what="quota 0, gang of 1")
    # quota that runs out in the middle of a node
    for q in range(2, 60):
        ql[0] = qa0[0] + q
        want = oracle_select(score, cap, req, ntasks, used0, qa0, ql, jp0, -1)
        last = want["ll"] - 1
        if want["pl"] == q and want["lc"][last] < cap[want["ln"][last]]:
            break
    else:
        raise AssertionError("no quota cuts a node in two")
    check_select(hip, score, cap, req, ntasks, used0, qa0, ql, jp0, -1,
                 what=f"quota {q}")
    check_select(hip, score, cap, req, ntasks, used0, qa0, ql, jp0, q,
                 what=f"quota {q} == gang")
    check_select(hip, score, cap, req, ntasks, used0, qa0, ql, jp0, q + 1,
                 what=f"quota {q} < gang")


def special_scores(N, seed):
    """Negative, both zeros, denormals, +-1e30 and -inf, each many times."""
    vals = torch.tensor([-1.0e30, -2.5, -1.0e-40, -1.0e-45, -0.0, 0.0,
                         1.0e-45, 1.0e-40, 2.5, 1.0e30, NEG_INF, -0.0, 0.0])
    g = torch.Generator().manual_seed(seed)
    return vals[torch.randint(0, len(vals), (N,), generator=g)]


def straddling_ties(N, seed):
    """Distinct scores except one 300-node tie group in the middle of the
    index range (it crosses per-thread chunk boundaries of the radix sort)
    ranked below ~900 others (its sorted positions cross the 1024-wide
    scan chunk)."""
    g = torch.Generator().manual_seed(seed)
    score = torch.randperm(N, generator=g).float() / 4096.0 + 1.0
    lo = N // 2 - 150
    above = min(900, N - 300 - 1)
    kth = torch.sort(score, descending=True).values[above]
    score[lo:lo + 300] = kth - 1.0 / 8192.0
    return score


@pytest.mark.parametrize("kind", ["special", "equal", "straddle", "dyadic"])
@pytest.mark.parametrize("N", [512, 1024, 1025, 2049])
def test_bulk_select_edges(hip, N, kind):
    R = 5
    g = torch.Generator().manual_seed(N)
    cap = torch.randint(1, 3, (N,), generator=g).to(torch.int32)
    req = int_req(R, N)
    if kind == "special":
        score = special_scores(N, N)
    elif kind == "equal":
        score = torch.full((N,), -0.75)
    elif kind == "straddle":
        score = straddling_ties(N, N)
        cap = torch.ones(N, dtype=torch.int32)
    else:
        score, cap, req = dyadic_scores(N, R, seed=N)
    cap = torch.where(score > NEG_INF, cap, torch.zeros_like(cap))
    used0, qa0, jp0 = int_state(N, R, N + 3)
    ql = torch.full((R,), NOLIMIT)
    room = int(cap.to(torch.int64).sum())
    # 512 is the dispatch threshold; the middle value stops inside the
    # straddling tie group; room + 1 runs the log to its end
    mid = min(room, 1050)
    if kind == "straddle":
        mid = int((score > score[N // 2]).sum()) + 150
    for ntasks in sorted({512, mid, room + 1}):
        if ntasks < 512:
            continue
        want = check_select(hip, score, cap, req, ntasks, used0, qa0, ql, jp0,
                            -1, bulk=True, what=f"{kind} ntasks={ntasks}")
        total = want["pl"]
        for fuse_min in (0, total, total + 1):
            check_select(hip, score, cap, req, ntasks, used0, qa0, ql, jp0,
                         fuse_min, bulk=True,
                         what=f"{kind} ntasks={ntasks} fuse={fuse_min}")
    if kind == "special":
        # +0.0 and -0.0 are one tie group: the log interleaves them by index
        want = oracle_select(score, cap, req, room, used0, qa0, ql, jp0, -1)
        nodes = want["ln"][:want["ll"]].long()
        zeros = nodes[score[nodes] == 0.0]
        signs = torch.signbit(score[zeros])
        assert zeros.tolist() == sorted(zeros.tolist())
        assert bool(signs.any()) and not bool(signs.all())
        assert int((signs[1:] != signs[:-1]).sum()) > 2
    if kind == "straddle" and mid >= 512:
        want = oracle_select(score, cap, req, mid, used0, qa0, ql, jp0, -1)
        tied = want["ln"][:want["ll"]].long()
        tied = tied[score[tied] == score[N // 2]]
        assert len(tied) == 150             # the cut falls inside the group
        if N == 2049:
            # sorted positions 900..1199: across the 1024-wide scan chunk
            assert mid - 150 < 1024 < mid + 150


def test_bulk_select_quota_mid_node(hip):
    N, R = 1025, 5
    score, cap, req = dyadic_scores(N, R, seed=4)
    used0, qa0, jp0 = int_state(N, R, 9)
    ql = torch.full((R,), NOLIMIT)
    for q in range(520, 600):
        ql[0] = qa0[0] + q
        want = oracle_select(score, cap, req, 5000, used0, qa0, ql, jp0, -1)
        last = want["ll"] - 1
        if want["pl"] == q and want["lc"][last] < cap[want["ln"][last]]:
            break
    else:
        raise AssertionError("no quota cuts a node in two")
    for fuse_min in (-1, q, q + 1):
        check_select(hip, score, cap, req, 5000, used0, qa0, ql, jp0,
                     fuse_min, bulk=True, what=f"quota {q} fuse {fuse_min}")


# --------------------------------------------------------------------------
# finalize_job / cond_revert
# --------------------------------------------------------------------------

@pytest.mark.parametrize("nc", [1, 2, 7])
def test_finalize_job(hip, nc):
    class_min = torch.arange(1, nc + 1, dtype=torch.int32)
    exact = class_min.clone()
    cases = []
    for delta in (-1, 0, 1):                  # placed + occupied vs minimum
        cases.append((exact, 3, int(exact.sum()) + 3 - delta))
    short = exact.clone()
    short[nc // 2] -= 1                       # one class one short
    cases.append((short, 3, 0))
    cases.append((exact + 2, 0, 0))
    flags = []
    for placed, occupied, min_available in cases:
        jp = placed.sum().to(torch.int32)
        want = torch.full((), 9, dtype=torch.uint8)
        ref.finalize_job(jp, occupied, min_available, placed, class_min, want)
        got = torch.full((1,), 9, dtype=torch.uint8, device=DEV)
        hip.finalize_job(jp.reshape(1).to(DEV), occupied, min_available,
                         placed.to(DEV), class_min.to(DEV), got)
        _sync()
        assert int(got.cpu()) == int(want)
        flags.append(int(want))
    assert flags == [0, 1, 1, 0, 1]


@pytest.mark.parametrize("R", [1, 64])
@pytest.mark.parametrize("log_len", [0, 1, 16, 17, 100])
@pytest.mark.parametrize("flag", [0, 1])
def test_cond_revert(hip, flag, log_len, R):
    N, K = 150, log_len + 3
    g = torch.Generator().manual_seed(log_len * 2 + flag)
    req = int_req(R, log_len)
    used0 = torch.randint(100, 200, (N, R), generator=g).float()
    qa0 = torch.randint(500, 600, (R,), generator=g).float()
    ln0 = torch.randperm(N, generator=g)[:K].to(torch.int32)
    lc0 = torch.randint(0, 4, (K,), generator=g).to(torch.int32)
    lc0[log_len:] = 0
    if log_len:
        lc0[0] = 2
    if log_len > 2:
        lc0[2] = 0                                   # an entry with count 0
    placed0 = int(lc0.sum())
    jp0 = placed0 + 11

    used, qa, lc = used0.clone(), qa0.clone(), lc0.clone()
    pl = torch.tensor(placed0, dtype=torch.int32)
    jp = torch.tensor(jp0, dtype=torch.int32)
    ref.cond_revert(torch.tensor(flag, dtype=torch.uint8), ln0.clone(), lc,
                    torch.tensor(log_len, dtype=torch.int32), req, used, qa,
                    pl, jp)

    used_g = used0.t().contiguous().clone().to(DEV)
    qa_g, ln_g, lc_g = qa0.to(DEV), ln0.to(DEV), lc0.to(DEV)
    pl_g = torch.full((1,), placed0, dtype=torch.int32, device=DEV)
    jp_g = torch.full((1,), jp0, dtype=torch.int32, device=DEV)
    hip.cond_revert(torch.full((1,), flag, dtype=torch.uint8, device=DEV),
                    ln_g, lc_g,
                    torch.full((1,), log_len, dtype=torch.int32, device=DEV),
                    req.to(DEV), used_g, qa_g, pl_g, jp_g)
    _sync()
    assert torch.equal(used_g.t().cpu(), used)
    assert torch.equal(qa_g.cpu(), qa)
    assert int(pl_g.cpu()) == int(pl) and int(jp_g.cpu()) == int(jp)
    assert torch.equal(lc_g.cpu(), lc)
    assert torch.equal(ln_g.cpu(), ln0)              # nodes are never touched
    if flag == 0:
        assert int(lc_g.cpu().abs().sum()) == 0
        assert int(jp_g.cpu()) == 11 and int(pl_g.cpu()) == 0
        if log_len:
            assert not torch.equal(used, used0)      # it SUBTRACTED something
    else:
        assert torch.equal(used, used0) and torch.equal(lc, lc0)


# --------------------------------------------------------------------------
# fused_score_select
# --------------------------------------------------------------------------

@pytest.mark.parametrize("N", [63, 1000, 4096])
def test_fused_score_select_equals_split(hip, N):
    R, W = 6, 2
    st = kc.dyadic_state(N, R, W, seed=N)
    tol, require, forbid = _class_masks(W, N)
    used0 = st["used"]
    qa0 = torch.arange(1, R + 1).float()
    jp0 = 4
    for ntasks, q, fuse_min in ((1, None, -1), (40, None, 40), (40, 25, -1),
                                (40, 25, 26), (511, None, 0),
                                (10 ** 6, None, 10 ** 6)):
        ql = torch.full((R,), NOLIMIT)
        if q is not None:
            ql[0] = qa0[0] + q
        s_c, cap_c = kc.oracle_score_cap(
            st, tolerated=tol, require=require, forbid=forbid, w_least=0.5,
            w_most=2.0, bias=st["bias"])
        want = oracle_select(s_c, cap_c, st["req"], ntasks, used0, qa0, ql,
                             jp0, fuse_min)
        split = gpu_select(hip, s_c, cap_c, st["req"], ntasks, used0, qa0, ql,
                           jp0, fuse_min)

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
            st["planes"].t().contiguous().to(DEV), st["req"].to(DEV), tol,
            require.to(DEV), forbid.to(DEV), 0.5, 2.0, 0.0,
            st["dim_w"].to(DEV), st["bias"].to(DEV), score, cap, ntasks, qa,
            ql.to(DEV), ln, lc, ll, pl, jp, fuse_min)
        _sync()
        fused = dict(ln=ln.cpu(), lc=lc.cpu(), ll=int(ll.cpu()),
                     pl=int(pl.cpu()), jp=int(jp.cpu()),
                     used=used_t.t().cpu(), qa=qa.cpu())
        what = f"ntasks={ntasks} q={q} fuse={fuse_min}"
        same_select(want, fused, f"fused vs oracle {what}")
        same_select(split, fused, f"fused vs split {what}")
        assert torch.equal(cap.cpu(), cap_c)
        # consumed nodes are knocked out of the score plane, nothing else
        after = s_c.clone()
        after[want["ln"][:want["ll"]].long()] = NEG_INF
        assert kc.same_bits(score.cpu(), after)


# --------------------------------------------------------------------------
# topk
# --------------------------------------------------------------------------

@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("N", [5, 16, 17, 1500])
def test_topk(hip, N, count):
    g = torch.Generator().manual_seed(N * 7 + count)
    rows = count + 1                      # the last row must stay untouched
    buf = (torch.rand(rows, N, generator=g) * 8).floor() / 8 - 0.5   # ties
    buf[torch.rand(rows, N, generator=g) < 0.2] = NEG_INF
    if count == 3:
        buf[1] = 0.25                                   # all-equal row
        buf[2] = NEG_INF                                # < 16 feasible
        buf[2, torch.randperm(N, generator=g)[:min(N, 7)]] = 1.5
    before = buf.clone()
    buf_g = buf.to(DEV)
    tv = torch.full((rows, kc.TOPK), 7.0, device=DEV)
    ti = torch.full((rows, kc.TOPK), -7, dtype=torch.int32, device=DEV)
    hip.topk(buf_g, count, tv, ti)
    _sync()
    buf_g, tv, ti = buf_g.cpu(), tv.cpu(), ti.cpu()
    for r in range(count):
        order = torch.argsort(before[r], descending=True, stable=True)
        order = order[before[r][order] > NEG_INF][:kc.TOPK]
        k = len(order)
        assert ti[r, :k].tolist() == order.tolist(), f"row {r} ids"
        assert kc.same_bits(tv[r, :k], before[r][order]), f"row {r} values"
        assert bool((tv[r, k:] == NEG_INF).all())
        assert ti[r, k:].tolist() == [INT32_MAX] * (kc.TOPK - k)
        after = before[r].clone()
        after[order] = NEG_INF
        assert kc.same_bits(buf_g[r], after), f"row {r} knock-outs"
    assert kc.same_bits(buf_g[count], before[count])
    assert bool((tv[count] == 7.0).all()) and bool((ti[count] == -7).all())
