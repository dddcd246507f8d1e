"""Score families, cases and a key-ordered model for the three domain rules
(topology spread, inter-pod affinity, keyed anti-affinity) on signed,
denormal and near-tied scores.

``_spread_cases`` and ``_affinity_cases`` draw four non-negative scores.  The
kernels order nodes by a 64-bit integer key (``spread_key`` of
``scheduler_kernels.hip``): the families below put values on both sides of
every branch of that key.  NaN and +inf stay out: ``score_cap`` cannot
produce them.

``key_fill`` is a NumPy model of a select that orders nodes by such a key;
``MUTANTS`` are wrong keys it can be run with.  Plain module: no fixtures,
no collection hooks, no GPU import.
"""

from __future__ import annotations

import contextlib
import functools
from typing import Callable, Dict

import numpy as np

import _affinity_cases as ac
import _spread_cases as sc

NEG_INF = float("-inf")
AFFINITY, ANTI = ac.AFFINITY, ac.ANTI
SPREAD = 0
UNBOUNDED = 2 ** 30
MIN_NORMAL = np.float32(2.0 ** -126)

# the finite values of test_ops_gpu_edges.special_scores (checked against it
# in test_domain_scores.py)
SPECIAL = np.array([-1.0e30, -2.5, -1.0e-40, -1.0e-45, -0.0, 0.0, 1.0e-45,
                    1.0e-40, 2.5, 1.0e30], dtype=np.float32)
LADDER_BASES = np.array([0.7, -0.7, 1.0, -1.0, 2.0 ** -126, -(2.0 ** -126)],
                        dtype=np.float32)


def fam_special(N, rng):
    return SPECIAL[rng.randint(0, len(SPECIAL), size=N)]


def fam_ladder(N, rng):
    """A base moved k in [-3, 3] ulps on its bit pattern: neighbours one ulp
    apart on both sides of zero, across +-1 and across the smallest
    normal."""
    bits = LADDER_BASES.view(np.uint32)[rng.randint(0, len(LADDER_BASES),
                                                    size=N)]
    k = rng.randint(-3, 4, size=N)
    return (bits.astype(np.int64) + k).astype(np.uint32).view(np.float32)


def fam_dense(N, rng):
    return rng.uniform(-1.0, 1.0, size=N).astype(np.float32)


def fam_grid(N, rng):
    s = (rng.randint(-3, 4, size=N) * 0.25).astype(np.float32)
    flip = (s == 0.0) & (rng.rand(N) < 0.5)
    s[flip] = np.float32(-0.0)
    return s


FAMILIES: Dict[str, Callable] = {"special": fam_special, "ladder": fam_ladder,
                                 "dense": fam_dense, "grid": fam_grid}
RS = (1, 5, 64)


# --------------------------------------------------------------------------
# section 3 cases
# --------------------------------------------------------------------------

def room_of(case) -> int:
    ok = (case.score > NEG_INF) & (case.dom_of >= 0)
    return int(case.cap[ok].sum())


def sized(case, top=160):
    """ntasks = min(room // 2 + 1, top): the sequential oracle is a Python
    loop of ntasks x N steps."""
    case.ntasks = max(1, min(room_of(case) // 2 + 1, top))
    return case


def spread_case(name, N, D, skew, R, seed, family, **kw):
    return sized(sc.random_case(name, N, D, skew, R, seed,
                                scores=FAMILIES[family], **kw))


def _revert_case(name, seed, family):
    case = spread_case(name, 257, 3, 1, 5, seed, family)
    case.fuse_min = case.ntasks + 1000          # can never be met
    return case


def spread_cases() -> Dict[str, Callable]:
    out = {}
    for f, fam in enumerate(FAMILIES):
        seen = set()
        for i, N in enumerate((63, 65, 1025, 2049)):
            for j, D in enumerate((1, 3, 65, "N")):
                d = N if D == "N" else min(D, N)
                if (N, d) in seen:
                    continue
                seen.add((N, d))
                for skew in (1, 2):
                    R = RS[(i + j + skew) % 3]
                    name = f"{fam}-N{N}-D{d}-s{skew}-R{R}"
                    out[name] = functools.partial(
                        spread_case, name, N, d, skew, R,
                        1000 * f + 100 * i + 10 * j + skew, fam,
                        unbalanced=(i + j) % 2 == 0)
        s = 5000 + 10 * f
        p = functools.partial
        out[f"{fam}-unbalanced"] = p(spread_case, "unb", 300, 5, 1, 5, s, fam,
                                     unbalanced=True)
        out[f"{fam}-dead-domain"] = p(spread_case, "dead", 257, 3, 1, 5,
                                      s + 1, fam, dead_domain=True)
        out[f"{fam}-quota"] = p(spread_case, "quota", 300, 4, 2, 5, s + 2,
                                fam, quota=11)
        out[f"{fam}-gang-revert"] = p(_revert_case, "rev", s + 3, fam)
        out[f"{fam}-cap-one"] = p(spread_case, "cap1", 1025, 3, 2, 1, s + 4,
                                  fam, cap_hi=1)
    return out


AFFINITY_SHAPES = ((65, 3), (1025, 65), (1025, 1025))


def _some_domains(D, seed, share):
    """0/1/2 members in about ``share`` of the domains, at least one domain
    of each kind when D > 1."""
    rng = np.random.RandomState(seed)
    count = ((rng.rand(D) < share) * rng.randint(1, 3, size=D)).astype(
        np.int32)
    if D > 1:
        count[0], count[D - 1] = 0, 1
    return count


def affinity_cases() -> Dict[str, Callable]:
    """aff-empty (the anchor is a float argmax), aff-hosting, and anti with
    600 instances (the sort-based select when N >= 512)."""
    out = {}
    p = functools.partial
    for f, fam in enumerate(FAMILIES):
        for i, (N, D) in enumerate(AFFINITY_SHAPES):
            R = (1, 4, 5)[(f + i) % 3]
            s = 7000 + 100 * f + 10 * i
            tag = f"{fam}-N{N}-D{D}"
            out[f"aff-empty-{tag}"] = p(
                ac.base_case, "empty", N, D, R, s, AFFINITY, ntasks=40,
                scores=FAMILIES[fam])
            out[f"aff-hosting-{tag}"] = p(
                ac.base_case, "hosting", N, D, R, s + 1, AFFINITY, ntasks=60,
                count=_some_domains(D, s, 0.25), scores=FAMILIES[fam])
            out[f"anti-{tag}"] = p(
                ac.base_case, "anti", N, D, R, s + 2, ANTI, ntasks=600,
                count=_some_domains(D, s + 2, 0.25), scores=FAMILIES[fam])
    return out


# the three relations between the domain rules and the plain select
RELATION_SHAPES = ((65, 3), (257, 64), (1025, 1025))


def _rel_spread(N, D, seed, fam):
    case = spread_case("rel", N, D, UNBOUNDED, 5, seed, fam, unlabeled=0.0)
    case.dom_count[:] = 0
    return case


def _rel_anti(N, seed, fam):
    return sized(ac.base_case("rel", N, N, 4, seed, ANTI, identity=True,
                              scores=FAMILIES[fam]))


def _rel_aff(N, seed, fam):
    return sized(ac.base_case("rel", N, 1, 4, seed, AFFINITY, count=[1],
                              unlabeled=0.0, scores=FAMILIES[fam]))


def relation_cases() -> Dict[str, Callable]:
    out = {}
    p = functools.partial
    for f, fam in enumerate(FAMILIES):
        for i, (N, D) in enumerate(RELATION_SHAPES):
            s = 9000 + 100 * f + 10 * i
            out[f"spread-{fam}-N{N}"] = p(_rel_spread, N, D, s, fam)
            out[f"anti-{fam}-N{N}"] = p(_rel_anti, N, s + 1, fam)
            out[f"aff-{fam}-N{N}"] = p(_rel_aff, N, s + 2, fam)
    return out


SPREAD_CASES = spread_cases()
AFFINITY_CASES = affinity_cases()
RELATION_CASES = relation_cases()


def rule_of(case) -> int:
    return getattr(case, "mode", SPREAD)


def run_oracle(case):
    return (sc if rule_of(case) == SPREAD else ac).run_oracle(case)


@functools.lru_cache(maxsize=None)
def oracle(name):
    """Case + oracle result: computed once, never modified."""
    table = SPREAD_CASES if name in SPREAD_CASES else \
        AFFINITY_CASES if name in AFFINITY_CASES else RELATION_CASES
    case = table[name]()
    return case, run_oracle(case)


def plain_select(case, *, clip=False, mask_cap=False):
    """reference.select_commit on the case's vectors -> the result dict of
    run_oracle, minus the domain counts.  ``clip``: caps clipped to 1;
    ``mask_cap``: cap zeroed where the score is -inf."""
    import torch
    from volcano_amd.ops import reference as ref
    t = torch.from_numpy
    b = ac._buffers(case)
    cap = case.cap.copy()
    if clip:
        cap = np.minimum(cap, 1)
    if mask_cap:
        cap[case.score == NEG_INF] = 0
    ref.select_commit(t(case.score.copy()), t(cap), b["req"], case.ntasks,
                      b["used"], b["qa"], t(case.queue_limit.copy()),
                      b["ln"], b["lc"], b["ll"], b["placed"], b["jp"])
    return dict(log_nodes=b["ln"].numpy(), log_counts=b["lc"].numpy(),
                log_len=int(b["ll"]), placed=int(b["placed"]),
                job_placed=int(b["jp"]), used=b["used"].numpy(),
                queue_alloc=b["qa"].numpy())


def expected(case, seq, count):
    """What a placement sequence must leave behind (the result dict of
    run_oracle)."""
    nodes, counts = sc.log_of(seq)
    revert = case.fuse_min >= 0 and len(seq) < case.fuse_min
    used = case.used.copy()
    qa = case.queue_alloc.copy()
    if not revert:
        for n, k in zip(nodes, counts):
            used[n] += np.float32(k) * case.req
        qa += np.float32(len(seq)) * case.req
    return dict(log_nodes=nodes,
                log_counts=[0] * len(nodes) if revert else counts,
                log_len=len(nodes), placed=0 if revert else len(seq),
                job_placed=7 + (0 if revert else len(seq)),
                dom_count=case.dom_count.tolist() if revert else list(count),
                used=used, queue_alloc=qa, reverted=revert)


# --------------------------------------------------------------------------
# the integer key, wrong variants of it, and a fill that orders by a key
# --------------------------------------------------------------------------

def spread_key(score, *, flip_negative=True, fold_zero=True, flush=False,
               invert_index=True, bits=64):
    """NumPy model of ``spread_key`` -> uint64 [N]; the keyword arguments
    switch single steps of it off."""
    score = np.ascontiguousarray(score, dtype=np.float32)
    u = score.view(np.uint32).copy()
    if flush:                      # denormals -> zero of the same sign
        u[(u & np.uint32(0x7F800000)) == 0] &= np.uint32(0x80000000)
    if fold_zero:
        u[u == np.uint32(0x80000000)] = 0
    neg = (u >> np.uint32(31)).astype(bool)
    if flip_negative:
        u = np.where(neg, ~u, u ^ np.uint32(0x80000000))
    else:
        u = u ^ np.uint32(0x80000000)
    idx = np.arange(len(score), dtype=np.uint32)
    low = (np.uint32(0xFFFFFFFF) - idx) if invert_index else idx
    key = (u.astype(np.uint64) << np.uint64(32)) | low.astype(np.uint64)
    if bits < 64:
        key &= ~np.uint64((1 << (64 - bits)) - 1)
    return key


MUTANTS: Dict[str, Callable] = {
    "no-negative-flip": functools.partial(spread_key, flip_negative=False),
    "no-zero-fold": functools.partial(spread_key, fold_zero=False),
    "denormals-flushed": functools.partial(spread_key, flush=True),
    "index-not-inverted": functools.partial(spread_key, invert_index=False),
    "upper-48-bits": functools.partial(spread_key, bits=48),
}


def key_fill(case, keyfn=spread_key, *, stats=False):
    """Sequential fill of any of the three rules that takes, before every
    instance, the eligible node with the largest key.  A max-reduce has no
    order among equal keys: the model then takes the LAST such node, the
    opposite of the contract, so that a key which fails to separate two
    nodes shows.  -> (placement sequence, counts[, what the run exercised:
    spread only])."""
    rule = rule_of(case)
    score, dom = case.score, case.dom_of
    key = keyfn(score)
    cnt = case.dom_count.astype(np.int64).copy()
    labelled = dom >= 0
    d_safe = np.where(labelled, dom, 0)
    rem = np.where((score > NEG_INF) & labelled, case.cap, 0).astype(np.int64)
    budget = min(case.ntasks, sc.quota_of(case))
    seen = dict(blocked=False, tie3=False, negative_over_blocked=False,
                zero_pair=False, denormal=False, rescan=False)
    zero_later = set()            # +0.0 nodes a -0.0 node won against
    seq = []
    while len(seq) < budget:
        live = rem > 0
        if rule == SPREAD:
            ok = live & (cnt[d_safe] + 1 - cnt.min() <= case.max_skew)
        elif rule == AFFINITY:
            ok = live & ((cnt[d_safe] > 0) | (not (cnt > 0).any()))
        else:
            ok = live & (cnt[d_safe] == 0)
        cand = np.flatnonzero(ok)
        if not len(cand):
            break
        k = key[cand]
        n = int(cand[len(k) - 1 - int(np.argmax(k[::-1]))])
        if stats:
            s = score[n]
            shut = live & ~ok
            seen["blocked"] |= bool(shut.any())
            seen["tie3"] |= int((score[cand] == s).sum()) >= 3
            seen["negative_over_blocked"] |= bool(
                s < 0 and (score[shut] > 0).any())
            seen["denormal"] |= bool(s != 0 and abs(s) < MIN_NORMAL)
            if s == 0 and np.signbit(s):
                later = cand[(cand > n) & (score[cand] == 0)
                             & ~np.signbit(score[cand])]
                zero_later.update(later.tolist())
            seen["zero_pair"] |= n in zero_later
            seen["rescan"] |= bool(rem[n] == 1 and
                                   (live & (dom == dom[n])).sum() > 1)
        rem[n] -= 1
        cnt[dom[n]] += 1
        seq.append(n)
    out = (seq, cnt.tolist())
    return out + (seen,) if stats else out


# --------------------------------------------------------------------------
# section 4: the domain rules behind the score kernel
# --------------------------------------------------------------------------

BIAS_SHIFT = -1.25            # plans, and scores of the weights (1, 0)
# per (w_least, w_most) of _kernel_cases.SCORE_WEIGHTS: the second pair
# weighs the most-requested term 2, which lifts every score by about 0.65
SCORE_SHIFT = {(1.0, 0.0): BIAS_SHIFT, (0.5, 2.0): -1.875}
SCORED_SHAPES = tuple((N, D) for N in (65, 1025, 2049)
                      for D in sorted({3, 65, N}) if D <= N)
SCORED_RW = ((5, 1), (64, 4))


def scored_states():
    """name -> (N, R, W, seed, w_least, w_most): every score_cap launch of
    section 4."""
    import _kernel_cases as kc
    out = {}
    for i, N in enumerate((65, 1025, 2049)):
        for j, (R, W) in enumerate(SCORED_RW):
            for k, (wl, wm) in enumerate(kc.SCORE_WEIGHTS):
                out[f"N{N}-R{R}-w{k}"] = (N, R, W, 300 + 10 * i + j, wl, wm)
    return out


SCORED_STATES = scored_states()


def scored_state(name):
    """-> (state, kwargs of the score call: w_bal 1, the shifted bias)."""
    import _kernel_cases as kc
    N, R, W, seed, wl, wm = SCORED_STATES[name]
    st = kc.dyadic_state(N, R, W, seed, inexact=True)
    return st, dict(w_least=wl, w_most=wm, w_bal=1.0,
                    bias=st["bias"] + np.float32(SCORE_SHIFT[(wl, wm)]))


def scored_case(name, score, cap, rule, D, skew=1):
    """A spread / affinity / anti case over the score and cap of a
    score_cap run on ``scored_state(name)`` (read back from the kernel on
    the GPU, from the oracle on the CPU).  Usage and request are the
    state's: small integers."""
    N, R, W, seed, _, _ = SCORED_STATES[name]
    st, _ = scored_state(name)
    if rule == SPREAD:
        case = sc.random_case(name, N, D, skew, R, seed + D + skew,
                              unbalanced=(D + skew) % 2 == 0)
    else:
        count = None if rule == "aff-empty" else \
            _some_domains(min(D, N), seed + D, 0.25)
        mode = ANTI if rule == "anti" else AFFINITY
        case = ac.base_case(name, N, D, R, seed + D, mode, count=count,
                            ntasks=60 if mode == AFFINITY else 160)
    case.score = np.array(score, dtype=np.float32)
    case.cap = np.array(cap, dtype=np.int32)
    case.req = st["req"].numpy().copy()
    case.used = st["used"].numpy().copy()
    return sized(case) if rule == SPREAD else case


# --------------------------------------------------------------------------
# whole plans: inexact, bias-shifted twins.  The seeds are the first on which
# the role conditions hold AND a domain-rule select logs nodes of both signs
# (most classes are small and stop among the positive scores).
# --------------------------------------------------------------------------

SPREAD_TWIN = dict(N=1000, seed=27, bulk=True, inexact=True, bias_shift=BIAS_SHIFT)
AFFINITY_TWINS = {N: dict(N=N, seed=39, inexact=True, bias_shift=BIAS_SHIFT)
                  for N in (65, 1500)}


def spread_twin():
    return sc.spread_plan_case(**SPREAD_TWIN)


def affinity_twin(N):
    return ac.affinity_plan_case(**AFFINITY_TWINS[N])


def affinity_plan_conditions(case, snap, records, *, exact=True):
    """Role conditions of an affinity plan.  ``exact=False`` keeps the ones
    that cannot depend on how a score rounds."""
    r = case.roles
    placed = snap["class_placed"]
    assert len(records) == len(case.affinity)
    assert any(x["placed"] > 0 and x["mode"] == AFFINITY for x in records)
    assert any(x["placed"] > 0 and x["mode"] == ANTI for x in records)
    # the job whose minimum is 100 N anchored, then reverted in place
    assert records[0]["placed"] > 0 and placed[r["aff_revert"]] == 0
    assert records[1]["count"] == [0, 0, 0]
    # the two-role gang reverted after its affinity role had placed
    jobs = [b for b, _ in snap["jobs"]]
    j = jobs.index(r["gang_aff"])
    assert snap["jobs"][j] == (r["gang_aff"], r["gang_aff"] + 2)
    assert snap["job_flag"][j] == 0
    assert records[2]["placed"] > 0 and placed[r["gang_aff"]] == 0
    if not exact:
        return
    assert records[1]["placed"] > 0 and placed[r["aff_anchor"]] > 0
    later = [x for x in records if x["mode"] == AFFINITY][3]
    assert later["count"] == records[1]["after"]
    anti = [x for x in records if x["mode"] == ANTI]
    assert anti[0]["placed"] > 0 and anti[1]["count"] == anti[0]["after"]
    assert anti[1]["placed"] > 0
    assert placed[r["spread"]] > 0 and placed[r["host"]] > 0
    if case.base.N >= 512:
        assert placed[r["aff_bulk"]] >= 512


@contextlib.contextmanager
def recording_signs(records: list):
    """Record, for every domain-rule select of an oracle plan run, how many
    of the nodes it logged carry a negative and how many a positive
    score."""
    from volcano_amd.ops import reference as ref
    real = {name: getattr(ref, name) for name in
            ("spread_select_commit", "affinity_select_commit")}

    def wrap(name):
        def spy(score, cap, req, ntasks, used, qa, ql, ln, lc, ll, *rest):
            s = score.clone().numpy()
            real[name](score, cap, req, ntasks, used, qa, ql, ln, lc, ll,
                       *rest)
            at = s[ln[:int(ll)].numpy()]
            records.append(dict(rule=name.split("_")[0], arg=rest[-1],
                                negative=int((at < 0).sum()),
                                positive=int((at > 0).sum())))
        return spy

    for name in real:
        setattr(ref, name, wrap(name))
    try:
        yield
    finally:
        for name, fn in real.items():
            setattr(ref, name, fn)
