"""ctypes bindings for the HIP kernel library + the plan-based cycle runner.

The GPU decision plane calls into ``_vamd_hip.so`` (pure HIP, C ABI).  On a
GPU box this module MUST load — ops fail loudly rather than silently
falling back to eager torch (the torch implementations in ``reference.py``
are the CPU oracle, not a GPU execution path).
"""

from __future__ import annotations

import ctypes
from ctypes import (POINTER, Structure, c_float, c_int, c_int32, c_int64,
                    c_uint64, c_void_p)
from typing import Optional

import numpy as np
import torch

from .build import LIB_PATH, build
from .reference import (DEV_MAX_CARDS, NUMA_MAX_ZONES, SPREAD_MAX_RULES,
                        SPREAD_MULTI_LDS_DOMAINS, SPREAD_SOFT_LDS_DOMAINS,
                        check_device_request,
                        check_hypernode_table, check_numa_request)

_lib = None

# Largest leaf count whose sums mode 3 of ``domain_mask`` keeps in LDS
# (``HN_LDS_LEAVES`` in scheduler_kernels.hip; checked against the library
# on load).  Above it the sums live in the scratch buffer.
HYPERNODE_LDS_LEAVES = 4095


class VamdClassDesc(Structure):
    _fields_ = [
        ("job_idx", c_int32), ("queue_idx", c_int32), ("ntasks", c_int32),
        ("min_needed", c_int32), ("log_off", c_int32), ("log_cap", c_int32),
        ("flags", c_int32), ("bias_row", c_int32),
        ("w_least", c_float), ("w_most", c_float), ("w_bal", c_float),
        ("_padf", c_float),
    ]


class VamdJobDesc(Structure):
    _fields_ = [
        ("class_begin", c_int32), ("class_end", c_int32),
        ("occupied", c_int32), ("min_available", c_int32),
    ]


class VamdSpreadRule(Structure):
    _fields_ = [("dom_of", c_void_p), ("count", c_void_p),
                ("D", c_int32), ("skew", c_int32)]


class VamdSpreadRules(Structure):
    """Mirror of ``VamdSpreadRules`` in ``vamd_api.h``, passed by value."""
    _fields_ = [("r", VamdSpreadRule * SPREAD_MAX_RULES),
                ("n", c_int32), ("_pad", c_int32)]


class VamdSpreadWeights(Structure):
    """Mirror of ``VamdSpreadWeights`` in ``vamd_api.h``, passed by value."""
    _fields_ = [("tw", c_float * SPREAD_MAX_RULES)]


class VamdCycle(Structure):
    """Mirror of ``VamdCycle`` in ``vamd_api.h`` (same order, same types)."""
    _fields_ = [("struct_size", c_uint64)] + [
        (n, c_int32) for n in ("N", "R", "W", "n_classes", "n_jobs", "_pad")
    ] + [(n, c_void_p) for n in (
        "classes", "jobs",
        "alloc", "used", "extra", "ready", "taints", "planes",
        "bias", "bias_rows",
        "class_req", "class_tol", "class_require", "class_forbid",
        "class_min", "dim_w",
        "queue_alloc", "queue_limit",
        "score_scratch", "cap_scratch", "log_nodes", "log_counts", "log_len",
        "class_placed", "job_placed", "job_flag", "sort_scratch",
        "class_group", "class_skew", "class_mode", "dom_of", "count",
        "count_off", "domains", "domain_scratch", "group_row",
        "card_mem_used", "card_cores_used", "card_state", "card_mem_total",
        "class_dev_req", "dev_assign")] + [
        ("card_K", c_int32), ("_pad2", c_int32)] + [
        (n, c_void_p) for n in (
            "zone_free", "class_numa_req", "numa_assign")] + [
        ("zone_Z", c_int32), ("_pad3", c_int32),
        ("class_spread_rules", c_void_p),
        ("class_rescore", c_void_p), ("rescore_slot", c_void_p),
        ("class_spread_rescore", c_void_p),
        ("class_spread_soft", c_void_p)]


def _load():
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        try:
            build()
        except Exception as e:  # pragma: no cover
            raise RuntimeError(
                f"HIP kernel library missing and build failed: {e}. "
                "Run `python -m volcano_amd.ops.build`."
            ) from e
    lib = ctypes.CDLL(str(LIB_PATH))
    lib.vamd_score_cap.restype = None
    lib.vamd_select_commit.restype = None
    lib.vamd_finalize_job.restype = None
    lib.vamd_cond_revert.restype = None
    lib.vamd_run_cycle.argtypes = [POINTER(VamdCycle), c_void_p]
    lib.vamd_run_cycle.restype = c_int
    lib.vamd_fused_score_select.restype = None
    lib.vamd_topk.restype = None
    lib.vamd_spread_select.restype = None
    lib.vamd_spread_revert.restype = None
    lib.vamd_domain_mask.restype = None
    lib.vamd_domain_count_add.restype = None
    lib.vamd_hypernode_lds_leaves.restype = c_int
    if lib.vamd_hypernode_lds_leaves() != HYPERNODE_LDS_LEAVES:
        raise RuntimeError(
            "the loaded kernel library and this module disagree on "
            "HYPERNODE_LDS_LEAVES; rebuild (python -m volcano_amd.ops.build)")
    lib.vamd_spread_multi_select.restype = None
    lib.vamd_spread_multi_count_sub.restype = None
    lib.vamd_spread_multi_lds_domains.restype = c_int
    if lib.vamd_spread_multi_lds_domains() != SPREAD_MULTI_LDS_DOMAINS:
        raise RuntimeError(
            "the loaded kernel library and this module disagree on "
            "SPREAD_MULTI_LDS_DOMAINS; rebuild (python -m "
            "volcano_amd.ops.build)")
    lib.vamd_rescore_select.restype = None
    lib.vamd_spread_rescore_select.restype = None
    lib.vamd_spread_soft_select.restype = None
    lib.vamd_spread_soft_lds_domains.restype = c_int
    if lib.vamd_spread_soft_lds_domains() != SPREAD_SOFT_LDS_DOMAINS:
        raise RuntimeError(
            "the loaded kernel library and this module disagree on "
            "SPREAD_SOFT_LDS_DOMAINS; rebuild (python -m "
            "volcano_amd.ops.build)")
    lib.vamd_device_cap.restype = None
    lib.vamd_device_commit.restype = None
    lib.vamd_device_revert.restype = None
    lib.vamd_device_max_cards.restype = c_int
    if lib.vamd_device_max_cards() != DEV_MAX_CARDS:
        raise RuntimeError(
            "the loaded kernel library and this module disagree on "
            "DEV_MAX_CARDS; rebuild (python -m volcano_amd.ops.build)")
    lib.vamd_numa_cap.restype = None
    lib.vamd_numa_commit.restype = None
    lib.vamd_numa_revert.restype = None
    lib.vamd_numa_max_zones.restype = c_int
    if lib.vamd_numa_max_zones() != NUMA_MAX_ZONES:
        raise RuntimeError(
            "the loaded kernel library and this module disagree on "
            "NUMA_MAX_ZONES; rebuild (python -m volcano_amd.ops.build)")
    _lib = lib
    return lib


def available() -> bool:
    try:
        _load()
        return True
    except Exception:
        return False


def _addr(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else t.data_ptr()


def _p(t: Optional[torch.Tensor]):
    return c_void_p(_addr(t))


def _stream() -> c_void_p:
    return c_void_p(torch.cuda.current_stream().cuda_stream)


# -- per-op wrappers (used by the GPU numerics tests) -----------------------

def score_cap(alloc_t, used_t, extra_t, ready, taints, planes_t, req,
              tolerated, require, forbid, w_least, w_most, w_bal, dim_w,
              bias, score_out, cap_out):
    """All node tensors are the transposed [R, N] / [W, N] device buffers."""
    lib = _load()
    R, N = alloc_t.shape
    W = planes_t.shape[0]
    lib.vamd_score_cap(
        _p(alloc_t), _p(used_t), _p(extra_t), _p(ready), _p(taints),
        _p(planes_t), _p(req), c_int64(int(tolerated)), _p(require),
        _p(forbid), c_float(w_least), c_float(w_most), c_float(w_bal),
        _p(dim_w), _p(bias), _p(score_out), _p(cap_out),
        c_int(N), c_int(R), c_int(W), _stream())


def select_commit(score, cap, req, ntasks, used_t, queue_alloc_row,
                  queue_limit_row, log_nodes, log_counts, log_len, placed,
                  job_placed, fuse_min, sort_scratch=None):
    lib = _load()
    N = score.shape[0]
    R = req.shape[0]
    K = log_nodes.shape[0]
    lib.vamd_select_commit(
        _p(score), _p(cap), _p(req), c_int(int(ntasks)), _p(used_t),
        _p(queue_alloc_row), _p(queue_limit_row), _p(log_nodes),
        _p(log_counts), _p(log_len), _p(placed), _p(job_placed),
        c_int(int(fuse_min)), _p(sort_scratch),
        c_int(N), c_int(R), c_int(K), _stream())


def finalize_job(job_placed, occupied, min_available, class_placed,
                 class_min, flag):
    lib = _load()
    nc = class_placed.shape[0]
    lib.vamd_finalize_job(
        _p(job_placed), c_int(int(occupied)), c_int(int(min_available)),
        _p(class_placed), _p(class_min), _p(flag), c_int(nc), _stream())


def cond_revert(flag, log_nodes, log_counts, log_len, req, used_t,
                queue_alloc_row, placed, job_placed):
    lib = _load()
    R, N = used_t.shape
    lib.vamd_cond_revert(
        _p(flag), _p(log_nodes), _p(log_counts), _p(log_len), _p(req),
        _p(used_t), _p(queue_alloc_row), _p(placed), _p(job_placed),
        c_int(N), c_int(R), _stream())


def spread_scratch(N: int, device) -> torch.Tensor:
    """Scratch of one spread select: D <= N 64-bit head keys + N log-slot
    ints (torch device allocations are at least 8-byte aligned)."""
    return torch.empty(3 * max(int(N), 1), dtype=torch.int32, device=device)


def spread_select(score, cap, req, ntasks, used_t, queue_alloc_row,
                  queue_limit_row, log_nodes, log_counts, log_len, placed,
                  job_placed, dom_of, dom_count, max_skew, fuse_min,
                  scratch=None):
    """Topology-spread select (after score_cap): maxSkew checked before
    every placement.  ``score`` and ``cap`` are consumed."""
    lib = _load()
    N = score.shape[0]
    R = req.shape[0]
    K = log_nodes.shape[0]
    D = dom_count.shape[0]
    if not 1 <= D <= max(N, 1):
        raise ValueError(f"spread_select: D={D} outside [1, N={N}]")
    if int(max_skew) < 1:
        raise ValueError("spread_select: max_skew must be >= 1")
    if dom_of.shape[0] != N:
        raise ValueError("spread_select: dom_of must have one entry per node")
    if scratch is None:
        scratch = spread_scratch(N, score.device)
    lib.vamd_spread_select(
        _p(score), _p(cap), _p(req), c_int(int(ntasks)), _p(used_t),
        _p(queue_alloc_row), _p(queue_limit_row), _p(log_nodes),
        _p(log_counts), _p(log_len), _p(placed), _p(job_placed),
        _p(dom_of), _p(dom_count), c_int(D), c_int(int(max_skew)),
        c_int(int(fuse_min)), _p(scratch),
        c_int(N), c_int(R), c_int(K), _stream())


def spread_revert(flag, log_nodes, log_counts, log_len, req, used_t,
                  queue_alloc_row, placed, job_placed, dom_of, dom_count):
    lib = _load()
    R, N = used_t.shape
    lib.vamd_spread_revert(
        _p(flag), _p(log_nodes), _p(log_counts), _p(log_len), _p(req),
        _p(used_t), _p(queue_alloc_row), _p(placed), _p(job_placed),
        _p(dom_of), _p(dom_count), c_int(dom_count.shape[0]),
        c_int(N), c_int(R), _stream())


def _spread_rules(op, rules, N) -> VamdSpreadRules:
    """Layout check of 1..4 ``(dom_of, dom_count, max_skew)`` rules -> the
    struct the launchers take by value."""
    rules = list(rules)
    if not 1 <= len(rules) <= SPREAD_MAX_RULES:
        raise ValueError(f"{op}: 1 to {SPREAD_MAX_RULES} rules, got "
                         f"{len(rules)}")
    out = VamdSpreadRules(n=len(rules))
    total = 0
    for k, (dom_of, dom_count, skew) in enumerate(rules):
        D = dom_count.shape[0]
        if not 1 <= D <= max(N, 1):
            raise ValueError(f"{op}: rule {k}: D={D} outside [1, N={N}]")
        if int(skew) < 1:
            raise ValueError(f"{op}: rule {k}: max_skew must be >= 1")
        if dom_of.shape[0] != N:
            raise ValueError(f"{op}: rule {k}: dom_of must have one entry "
                             "per node")
        if dom_of.dtype != torch.int32 or dom_count.dtype != torch.int32 \
                or not dom_of.is_contiguous() \
                or not dom_count.is_contiguous():
            raise ValueError(f"{op}: rule {k}: dom_of and dom_count are "
                             "contiguous int32")
        total += D
        out.r[k] = VamdSpreadRule(_addr(dom_of), _addr(dom_count), D,
                                  int(skew))
    if total > SPREAD_MULTI_LDS_DOMAINS:
        raise ValueError(f"{op}: {total} domains over all rules, at most "
                         f"{SPREAD_MULTI_LDS_DOMAINS}")
    return out


def spread_multi_select(score, cap, req, ntasks, used_t, queue_alloc_row,
                        queue_limit_row, log_nodes, log_counts, log_len,
                        placed, job_placed, rules, fuse_min, scratch=None):
    """``spread_select`` under 1 to 4 rules ``(dom_of, dom_count, max_skew)``
    at once: a node is eligible in the intersection of the rules' open
    domains, every placement joins the counts of every rule.  ``score`` and
    ``cap`` are consumed; ``scratch`` holds 4*N bytes."""
    lib = _load()
    N = score.shape[0]
    R = req.shape[0]
    K = log_nodes.shape[0]
    rs = _spread_rules("spread_multi_select", rules, N)
    if scratch is None:
        scratch = spread_scratch(N, score.device)
    elif scratch.numel() * scratch.element_size() < 4 * N:
        raise ValueError("spread_multi_select: scratch smaller than 4*N "
                         "bytes")
    lib.vamd_spread_multi_select(
        _p(score), _p(cap), _p(req), c_int(int(ntasks)), _p(used_t),
        _p(queue_alloc_row), _p(queue_limit_row), _p(log_nodes),
        _p(log_counts), _p(log_len), _p(placed), _p(job_placed), rs,
        c_int(int(fuse_min)), _p(scratch), c_int(N), c_int(R), c_int(K),
        _stream())


def spread_multi_count_sub(flag, log_nodes, log_counts, log_len, rules):
    """When ``flag`` is 0 the logged placements leave the counts of rules
    1..n-1 — before ``spread_revert``, which handles rule 0 and zeroes the
    log."""
    lib = _load()
    N = rules[0][0].shape[0]
    K = log_nodes.shape[0]
    if log_counts.shape[0] != K:
        raise ValueError("spread_multi_count_sub: log_nodes/log_counts "
                         "differ in length")
    rs = _spread_rules("spread_multi_count_sub", rules, N)
    lib.vamd_spread_multi_count_sub(
        _p(flag), _p(log_nodes), _p(log_counts), _p(log_len), rs, c_int(N),
        c_int(K), _stream())


def rescore_select(alloc_t, used_t, extra_t, ready, taints, planes_t, req,
                   tolerated, require, forbid, w_least, w_most, w_bal, dim_w,
                   bias, score, cap, ntasks, queue_alloc_row, queue_limit_row,
                   log_nodes, log_counts, log_len, placed, job_placed,
                   fuse_min, slot=None):
    """``select_commit`` with the chosen node scored again after every
    placement (after ``score_cap`` and any cap or mask op, whose inputs it
    takes as well).  ``score`` is consumed; ``slot`` holds N int32."""
    lib = _load()
    R, N = alloc_t.shape
    W = planes_t.shape[0]
    K = log_nodes.shape[0]
    if score.shape[0] != N or cap.shape[0] != N:
        raise ValueError("rescore_select: score and cap need one entry per "
                         "node")
    if K < 1 or log_counts.shape[0] != K:
        raise ValueError("rescore_select: log_nodes/log_counts differ in "
                         "length or are empty")
    if slot is None:
        slot = torch.empty(max(N, 1), dtype=torch.int32, device=score.device)
    elif slot.numel() * slot.element_size() < 4 * N:
        raise ValueError("rescore_select: slot smaller than 4*N bytes")
    lib.vamd_rescore_select(
        _p(alloc_t), _p(used_t), _p(extra_t), _p(ready), _p(taints),
        _p(planes_t), _p(req), c_int64(int(tolerated)), _p(require),
        _p(forbid), c_float(w_least), c_float(w_most), c_float(w_bal),
        _p(dim_w), _p(bias), _p(score), _p(cap), c_int(int(ntasks)),
        _p(queue_alloc_row), _p(queue_limit_row), _p(log_nodes),
        _p(log_counts), _p(log_len), _p(placed), _p(job_placed),
        c_int(int(fuse_min)), _p(slot), c_int(N), c_int(R), c_int(W),
        c_int(K), _stream())


def spread_rescore_select(alloc_t, used_t, extra_t, req, w_least, w_most,
                          w_bal, dim_w, bias, score, cap, ntasks,
                          queue_alloc_row, queue_limit_row, log_nodes,
                          log_counts, log_len, placed, job_placed, rules,
                          fuse_min, slot=None):
    """``spread_multi_select`` under 1 to 4 rules with the chosen node scored
    again after every placement, as ``rescore_select`` scores it (after
    ``score_cap`` and any cap op).  ``score`` is consumed, ``cap`` only read;
    ``slot`` holds N int32."""
    lib = _load()
    R, N = alloc_t.shape
    K = log_nodes.shape[0]
    if score.shape[0] != N or cap.shape[0] != N:
        raise ValueError("spread_rescore_select: score and cap need one "
                         "entry per node")
    if K < 1 or log_counts.shape[0] != K:
        raise ValueError("spread_rescore_select: log_nodes/log_counts differ "
                         "in length or are empty")
    rs = _spread_rules("spread_rescore_select", rules, N)
    if slot is None:
        slot = torch.empty(max(N, 1), dtype=torch.int32, device=score.device)
    elif slot.numel() * slot.element_size() < 4 * N:
        raise ValueError("spread_rescore_select: slot smaller than 4*N bytes")
    lib.vamd_spread_rescore_select(
        _p(alloc_t), _p(used_t), _p(extra_t), _p(req), c_float(w_least),
        c_float(w_most), c_float(w_bal), _p(dim_w), _p(bias), _p(score),
        _p(cap), c_int(int(ntasks)), _p(queue_alloc_row),
        _p(queue_limit_row), _p(log_nodes), _p(log_counts), _p(log_len),
        _p(placed), _p(job_placed), rs, c_int(int(fuse_min)), _p(slot),
        c_int(N), c_int(R), c_int(K), _stream())


def _soft_weights(op, rules) -> VamdSpreadWeights:
    """The ``tw`` of 1..4 ``(dom_of, dom_count, max_skew, tw)`` rules as the
    launcher takes them, after the limits of the two LDS tables: the hard
    rules' domains fill the bitmaps, the soft rules' the count table."""
    tws = [float(tw) for _, _, _, tw in rules]
    if not np.isfinite(tws).all():
        raise ValueError(f"{op}: the weights must be finite")
    soft = sum(c.shape[0] for (_, c, _, _), tw in zip(rules, tws) if tw != 0)
    if soft > SPREAD_SOFT_LDS_DOMAINS:
        raise ValueError(f"{op}: {soft} domains over the soft rules, at most "
                         f"{SPREAD_SOFT_LDS_DOMAINS}")
    return VamdSpreadWeights((c_float * SPREAD_MAX_RULES)(*tws))


def spread_soft_select(alloc_t, used_t, extra_t, req, w_least, w_most, w_bal,
                       dim_w, bias, score, cap, ntasks, queue_alloc_row,
                       queue_limit_row, log_nodes, log_counts, log_len,
                       placed, job_placed, rules, rescore, fuse_min,
                       slot=None):
    """``spread_rescore_select`` under 1 to 4 rules ``(dom_of, dom_count,
    max_skew, tw)``: a rule with ``tw == 0`` is hard; one with ``tw != 0`` is
    soft (ScheduleAnyway), never filters on counts and costs ``tw`` per
    member already in the node's domain, before every placement.  With
    ``rescore`` the chosen node is scored again after every placement.
    ``score`` is consumed, ``cap`` only read; ``slot`` holds N int32."""
    lib = _load()
    R, N = alloc_t.shape
    K = log_nodes.shape[0]
    if score.shape[0] != N or cap.shape[0] != N:
        raise ValueError("spread_soft_select: score and cap need one entry "
                         "per node")
    if K < 1 or log_counts.shape[0] != K:
        raise ValueError("spread_soft_select: log_nodes/log_counts differ in "
                         "length or are empty")
    rules = list(rules)
    rs = _spread_rules("spread_soft_select", [r[:3] for r in rules], N)
    ws = _soft_weights("spread_soft_select", rules)
    if slot is None:
        slot = torch.empty(max(N, 1), dtype=torch.int32, device=score.device)
    elif slot.numel() * slot.element_size() < 4 * N:
        raise ValueError("spread_soft_select: slot smaller than 4*N bytes")
    lib.vamd_spread_soft_select(
        _p(alloc_t), _p(used_t), _p(extra_t), _p(req), c_float(w_least),
        c_float(w_most), c_float(w_bal), _p(dim_w), _p(bias), _p(score),
        _p(cap), c_int(int(ntasks)), _p(queue_alloc_row),
        _p(queue_limit_row), _p(log_nodes), _p(log_counts), _p(log_len),
        _p(placed), _p(job_placed), rs, ws, c_int(1 if rescore else 0),
        c_int(int(fuse_min)), _p(slot), c_int(N), c_int(R), c_int(K),
        _stream())


def domain_mask(score, cap, dom_of, dom_count, mode, scratch=None):
    """Inter-pod affinity (``mode`` 1) / keyed anti-affinity (``mode`` 2)
    mask over ``score``/``cap`` (after score_cap, before select_commit),
    from the group's live per-domain counts.  Both are changed in place."""
    lib = _load()
    N = score.shape[0]
    D = dom_count.shape[0]
    if not 1 <= D <= max(N, 1):
        raise ValueError(f"domain_mask: D={D} outside [1, N={N}]")
    if int(mode) not in (1, 2):
        raise ValueError("domain_mask: mode must be 1 (affinity) or 2 (anti)")
    if dom_of.shape[0] != N or cap.shape[0] != N:
        raise ValueError("domain_mask: dom_of and cap must have one entry "
                         "per node")
    if scratch is None:
        scratch = spread_scratch(N, score.device)
    elif scratch.numel() * scratch.element_size() < 8 * D:
        raise ValueError("domain_mask: scratch smaller than 8*D bytes")
    lib.vamd_domain_mask(
        _p(score), _p(cap), _p(dom_of), _p(dom_count), c_int(D),
        c_int(int(mode)), _p(scratch), c_int(N), _stream())


def hypernode_mask(score, cap, leaf_of, table, n_leaves, scratch=None,
                   check=True):
    """Network-topology domain choice (mode 3 of the domain mask; after
    score_cap, before select_commit): keeps the nodes of the one hypernode
    the ``table`` rule picks from the live ``cap`` (layout in
    ``vamd_api.h``; built by ``reference.hypernode_table``), masks the
    rest.  ``score`` and ``cap`` are changed in place.

    The kernel trusts the table's offsets, so ``check`` (default) copies
    the table to the host and validates it first — a device-to-host copy
    and a sync.  A caller that validated its table on the host
    (``reference.check_hypernode_table``; plan building does) passes
    ``check=False`` and gets a plain asynchronous launch."""
    lib = _load()
    N = score.shape[0]
    D = int(n_leaves)
    if not 1 <= D <= max(N, 1):
        raise ValueError(f"hypernode_mask: D={D} outside [1, N={N}]")
    if leaf_of.shape[0] != N or cap.shape[0] != N:
        raise ValueError("hypernode_mask: leaf_of and cap must have one "
                         "entry per node")
    if leaf_of.dtype != torch.int32 or table.dtype != torch.int32 \
            or cap.dtype != torch.int32 or score.dtype != torch.float32:
        raise ValueError("hypernode_mask: score is float32; cap, leaf_of "
                         "and table are int32")
    if check:
        check_hypernode_table(table.cpu().numpy(), D)
    if scratch is None:
        scratch = spread_scratch(N, score.device)
    elif scratch.numel() * scratch.element_size() < 8 * (D + 1):
        raise ValueError("hypernode_mask: scratch smaller than 8*(D+1) "
                         "bytes")
    lib.vamd_domain_mask(
        _p(score), _p(cap), _p(leaf_of), _p(table), c_int(D), c_int(3),
        _p(scratch), c_int(N), _stream())


def domain_count_add(log_nodes, log_counts, log_len, dom_of, dom_count):
    """The logged placements of a domain-mask class join the group's
    per-domain counts (after select_commit)."""
    lib = _load()
    N = dom_of.shape[0]
    D = dom_count.shape[0]
    K = log_nodes.shape[0]
    if not 1 <= D <= max(N, 1):
        raise ValueError(f"domain_count_add: D={D} outside [1, N={N}]")
    if log_counts.shape[0] != K:
        raise ValueError("domain_count_add: log_nodes/log_counts differ in "
                         "length")
    lib.vamd_domain_count_add(
        _p(log_nodes), _p(log_counts), _p(log_len), _p(dom_of),
        _p(dom_count), c_int(D), c_int(N), c_int(K), _stream())


# what a set of unit planes allows and how each family words its three
# complaints: (limit on U, wrong rank or U, shapes differ, wrong layout)
_CARDS = (DEV_MAX_CARDS,
          f"card planes are [K, N], 1 <= K <= {DEV_MAX_CARDS}",
          "card planes differ in shape", "card planes are contiguous int32")
_ZONES = (NUMA_MAX_ZONES,) + 3 * (
    f"zone_free is contiguous int32 [Z, N], 1 <= Z <= {NUMA_MAX_ZONES}",)


def _unit_planes(op, family, planes, per_node=None):
    """(U, N) of the unit planes of a family, checked: contiguous int32
    [U, N], 1 <= U <= limit, all the same shape (``per_node``: [N]).
    Plain loops: this runs in front of every launch.  The planes live on
    the device, so what they HOLD is the caller's precondition, checked
    where they are built from host arrays (``plan.set_device_state``,
    ``plan.set_numa_state``): 0 <= mem_total < 2^28, mem_used >= 0,
    cores_used >= 0, a slice count in [0, 2^28); 0 <= zone_free < 2^28."""
    limit, bad_rank, bad_shape, bad_layout = family
    shape = planes[0].shape
    if len(shape) != 2 or not 1 <= shape[0] <= limit:
        raise ValueError(f"{op}: {bad_rank}")
    for t in planes:
        if t.shape != shape:
            raise ValueError(f"{op}: {bad_shape}")
    if per_node is not None:
        if per_node.shape != shape[1:]:
            raise ValueError(f"{op}: {bad_shape}")
        planes += (per_node,)
    for t in planes:
        if t.dtype != torch.int32 or not t.is_contiguous():
            raise ValueError(f"{op}: {bad_layout}")
    return shape


def _assign_rows(op, assign, L, U, dims):
    """``assign`` is contiguous int32 [L, U]; ``dims`` words the shape."""
    if assign.shape != (L, U) or assign.dtype != torch.int32 \
            or not assign.is_contiguous():
        raise ValueError(f"{op}: assign is contiguous int32 {dims}, "
                         "parallel to the log")


def device_cap(score, cap, mem_used, cores_used, state, mem_total, request):
    """Per-card packing clamp (after score_cap, before any domain rule):
    ``cap = min(cap, S // count)`` with ``S`` the node's slots for
    ``request`` = (count, memory, cores) on the card planes [K, N];
    ``score = -inf`` where that leaves 0.  Both change in place."""
    lib = _load()
    count, memory, cores = check_device_request(request)
    K, N = _unit_planes("device_cap", _CARDS, (mem_used, cores_used, state),
                        mem_total)
    if score.shape != (N,) or cap.shape != (N,):
        raise ValueError("device_cap: score and cap need one entry per node")
    lib.vamd_device_cap(
        _p(score), _p(cap), _p(mem_used), _p(cores_used), _p(state),
        _p(mem_total), c_int(count), c_int(memory), c_int(cores), c_int(K),
        c_int(N), _stream())


def device_commit(log_nodes, log_counts, log_len, mem_used, cores_used, state,
                  mem_total, assign, request):
    """The logged placements take their slices on the card planes (after
    the select); ``assign`` [L, K] int32 receives, per log entry, the used
    cards in fill order as ``card << 28 | take``."""
    lib = _load()
    count, memory, cores = check_device_request(request)
    K, N = _unit_planes("device_commit", _CARDS, (mem_used, cores_used, state),
                        mem_total)
    L = log_nodes.shape[0]
    # a log_counts of another length gets the same complaint
    _assign_rows("device_commit", assign,
                 L if log_counts.shape[0] == L else -1, K, "[L, K]")
    lib.vamd_device_commit(
        _p(log_nodes), _p(log_counts), _p(log_len), _p(mem_used),
        _p(cores_used), _p(state), _p(mem_total), _p(assign), c_int(count),
        c_int(memory), c_int(cores), c_int(K), c_int(N), c_int(L), _stream())


def device_revert(flag, log_nodes, log_len, mem_used, cores_used, state,
                  mem_total, assign, request):
    """When ``flag`` is 0: the card planes give back what ``assign``
    recorded, and ``assign`` is zeroed."""
    lib = _load()
    _, memory, cores = check_device_request(request)
    K, N = _unit_planes("device_revert", _CARDS, (mem_used, cores_used, state),
                        mem_total)
    L = log_nodes.shape[0]
    _assign_rows("device_revert", assign, L, K, "[L, K]")
    lib.vamd_device_revert(
        _p(flag), _p(log_nodes), _p(log_len), _p(mem_used), _p(cores_used),
        _p(state), _p(assign), c_int(memory), c_int(cores), c_int(K),
        c_int(N), c_int(L), _stream())


def numa_cap(score, cap, zone_free, cpu):
    """Per-zone clamp of a hard NUMA policy (after score_cap and
    device_cap, before any domain rule): ``cap = min(cap, S)`` with ``S``
    the pods of ``cpu`` millicores the node's zones [Z, N] still pin;
    ``score = -inf`` where that leaves 0.  Both change in place."""
    lib = _load()
    cpu, _ = check_numa_request(cpu, 1)
    Z, N = _unit_planes("numa_cap", _ZONES, (zone_free,))
    if score.shape != (N,) or cap.shape != (N,):
        raise ValueError("numa_cap: score and cap need one entry per node")
    lib.vamd_numa_cap(_p(score), _p(cap), _p(zone_free), c_int(cpu), c_int(Z),
                      c_int(N), _stream())


def numa_commit(log_nodes, log_counts, log_len, zone_free, assign, cpu):
    """The logged placements take their zones (after the select); pods
    past what the zones pin stay unpinned.  ``assign`` [L, Z] int32
    receives, per log entry, the used zones in fill order as
    ``zone << 28 | take``."""
    lib = _load()
    cpu, _ = check_numa_request(cpu, 1)
    Z, N = _unit_planes("numa_commit", _ZONES, (zone_free,))
    L = log_nodes.shape[0]
    if log_counts.shape[0] != L:
        raise ValueError("numa_commit: log_nodes and log_counts differ")
    _assign_rows("numa_commit", assign, L, Z, "[L, Z]")
    lib.vamd_numa_commit(
        _p(log_nodes), _p(log_counts), _p(log_len), _p(zone_free), _p(assign),
        c_int(cpu), c_int(Z), c_int(N), c_int(L), _stream())


def numa_revert(flag, log_nodes, log_len, zone_free, assign, cpu):
    """When ``flag`` is 0: the zones get back what ``assign`` recorded,
    and ``assign`` is zeroed."""
    lib = _load()
    cpu, _ = check_numa_request(cpu, 1)
    Z, N = _unit_planes("numa_revert", _ZONES, (zone_free,))
    L = log_nodes.shape[0]
    _assign_rows("numa_revert", assign, L, Z, "[L, Z]")
    lib.vamd_numa_revert(
        _p(flag), _p(log_nodes), _p(log_len), _p(zone_free), _p(assign),
        c_int(cpu), c_int(Z), c_int(N), c_int(L), _stream())


def fused_score_select(alloc_t, used_t, extra_t, ready, taints, planes_t,
                       req, tolerated, require, forbid, w_least, w_most,
                       w_bal, dim_w, bias, score, cap, ntasks,
                       queue_alloc_row, queue_limit_row, log_nodes,
                       log_counts, log_len, placed, job_placed, fuse_min):
    """score_cap + serial select_commit in one launch (the N <= 4096
    small-class path of the cycle runner)."""
    lib = _load()
    R, N = alloc_t.shape
    W = planes_t.shape[0]
    K = log_nodes.shape[0]
    lib.vamd_fused_score_select(
        _p(alloc_t), _p(used_t), _p(extra_t), _p(ready), _p(taints),
        _p(planes_t), _p(req), c_int64(int(tolerated)), _p(require),
        _p(forbid), c_float(w_least), c_float(w_most), c_float(w_bal),
        _p(dim_w), _p(bias), _p(score), _p(cap), c_int(int(ntasks)),
        _p(queue_alloc_row), _p(queue_limit_row), _p(log_nodes),
        _p(log_counts), _p(log_len), _p(placed), _p(job_placed),
        c_int(int(fuse_min)), c_int(N), c_int(R), c_int(W), c_int(K),
        _stream())


def topk(score_buf, count, topk_vals, topk_ids):
    """Top-16 candidates of the first ``count`` rows of score_buf [*, N];
    chosen entries are knocked out of the row."""
    lib = _load()
    N = score_buf.shape[1]
    lib.vamd_topk(_p(score_buf), c_int(int(count)), _p(topk_vals),
                  _p(topk_ids), c_int(N), _stream())


# -- whole-cycle runner ------------------------------------------------------

def run_cycle(class_descs: bytes, n_classes: int, job_descs: bytes,
              n_jobs: int, alloc_t, used_t, extra_t, ready, taints, planes_t,
              bias, bias_rows, class_req, class_tol, class_require,
              class_forbid, class_min, dim_w, queue_alloc, queue_limit,
              score_scratch, cap_scratch, log_nodes, log_counts, log_len,
              class_placed, job_placed, job_flag, sort_scratch=None,
              spread=None, devices=None, numa=None, rescore=None):
    """One library call = one whole allocate cycle (plan built host-side).

    ``class_descs`` / ``job_descs`` are host buffers of ``VamdClassDesc`` /
    ``VamdJobDesc``; ``class_tol`` is a host tensor, every other tensor is
    on the device.

    ``spread`` (plans with domain-rule classes only) is a dict:
    ``class_group``/``class_skew`` host int32 numpy [C], ``dom_of`` device
    i32 [G, N], ``count`` device i32 (groups back to back), ``count_off``/
    ``domains`` host int32 numpy [G], ``scratch`` device
    (``spread_scratch``).  An optional ``class_mode`` (host int32 numpy
    [C]: 0 spread, 1 inter-pod affinity, 2 keyed anti-affinity, 3 network
    topology) fills the mode column; without it every class of a group is
    a spread class.  An optional ``group_row`` (host int32 numpy [G]) names
    the row of ``dom_of`` each group reads — all network-topology groups
    share one ``leaf_of`` row; without it group g reads row g.  The
    ``count`` slice of a mode-3 group is its table.  An optional
    ``class_rules`` (host int32 numpy [C, 9]: n, then four (group, maxSkew)
    pairs) names every rule of the spread classes that have several (n >= 2;
    rule 0 is also the class's ``class_group``/``class_skew``).  An optional
    ``class_rescore`` (host int32 numpy [C]) flags the spread classes whose
    chosen node is scored again after every placement
    (``spread_rescore_select``, for one rule or several).  An optional
    ``class_soft`` (host float32 numpy [C, 4]) holds one weight per rule of
    every spread class, in the order of ``class_rules`` (or rule 0 alone): a
    row with a nonzero weight runs ``spread_soft_select``.

    ``devices`` (plans with device-request classes only) is a dict: the
    card planes ``mem_used``/``cores_used``/``state`` device i32 [K, N],
    ``mem_total`` device i32 [N], ``class_req`` host int32 numpy [C, 4]
    (count, memory, cores, 0; count 0 = no request) and ``assign`` device
    i32 [L, K] (zeroed), parallel to the log.

    ``numa`` (plans with NUMA-request classes only) is a dict:
    ``zone_free`` device i32 [Z, N], ``class_req`` host int32 numpy [C, 2]
    (cpu millicores, policy: 0 = none, 1 = hard, 2 = best-effort) and
    ``assign`` device i32 [L, Z] (zeroed), parallel to the log.

    ``rescore`` (plans with re-scoring classes only) is a dict:
    ``class_rescore`` host int32 numpy [C] (nonzero = the class's chosen
    node is scored again after every placement) and ``slot`` device i32
    [N] scratch."""
    lib = _load()
    R, N = alloc_t.shape
    cy = VamdCycle(
        struct_size=ctypes.sizeof(VamdCycle), N=N, R=R, W=planes_t.shape[0],
        n_classes=n_classes, n_jobs=n_jobs,
        classes=ctypes.cast(class_descs, c_void_p),
        jobs=ctypes.cast(job_descs, c_void_p),
        alloc=_addr(alloc_t), used=_addr(used_t), extra=_addr(extra_t),
        ready=_addr(ready), taints=_addr(taints), planes=_addr(planes_t),
        bias=_addr(bias), bias_rows=_addr(bias_rows),
        class_req=_addr(class_req), class_tol=_addr(class_tol),
        class_require=_addr(class_require), class_forbid=_addr(class_forbid),
        class_min=_addr(class_min), dim_w=_addr(dim_w),
        queue_alloc=_addr(queue_alloc), queue_limit=_addr(queue_limit),
        score_scratch=_addr(score_scratch), cap_scratch=_addr(cap_scratch),
        log_nodes=_addr(log_nodes), log_counts=_addr(log_counts),
        log_len=_addr(log_len), class_placed=_addr(class_placed),
        job_placed=_addr(job_placed), job_flag=_addr(job_flag),
        sort_scratch=_addr(sort_scratch))
    if spread is not None:
        mode = spread.get("class_mode")
        if mode is not None:
            if mode.shape[0] != n_classes or mode.dtype != "int32":
                raise ValueError("run_cycle: class_mode must be int32 [C]")
            cy.class_mode = mode.ctypes.data
        cy.class_group = spread["class_group"].ctypes.data
        cy.class_skew = spread["class_skew"].ctypes.data
        cy.dom_of = _addr(spread["dom_of"])
        cy.count = _addr(spread["count"])
        cy.count_off = spread["count_off"].ctypes.data
        cy.domains = spread["domains"].ctypes.data
        cy.domain_scratch = _addr(spread["scratch"])
        rows = spread.get("group_row")
        if rows is not None:
            if rows.dtype != "int32" or \
                    rows.shape[0] != spread["domains"].shape[0]:
                raise ValueError("run_cycle: group_row must be int32 [G]")
            cy.group_row = rows.ctypes.data
        cr = spread.get("class_rules")
        if cr is not None:
            doms = spread["domains"]
            if cr.shape != (n_classes, 9) or cr.dtype != "int32" \
                    or not cr.flags["C_CONTIGUOUS"]:
                raise ValueError("run_cycle: class_rules must be int32 "
                                 "[C, 9]")
            # the slice of a group that a mode-3 class names is a table
            tables = set() if mode is None else \
                set(spread["class_group"][mode == 3].tolist())
            for c, row in enumerate(cr):
                n = int(row[0])
                if n < 2:
                    continue
                gs, skews = row[1:1 + 2 * n:2], row[2:2 + 2 * n:2]
                if n > SPREAD_MAX_RULES or gs.min() < 0 \
                        or gs.max() >= doms.shape[0] or skews.min() < 1 \
                        or gs[0] != spread["class_group"][c] \
                        or (mode is not None and mode[c] != 0) \
                        or len(set(gs.tolist())) != n \
                        or tables & set(gs.tolist()) \
                        or int(doms[gs].sum()) > SPREAD_MULTI_LDS_DOMAINS:
                    raise ValueError(f"run_cycle: class_rules row {c}: 2 to "
                                     f"{SPREAD_MAX_RULES} distinct spread "
                                     "groups, maxSkew >= 1, rule 0 = "
                                     "class_group with mode 0, at most "
                                     f"{SPREAD_MULTI_LDS_DOMAINS} domains in "
                                     "all")
            cy.class_spread_rules = cr.ctypes.data
        flags = spread.get("class_rescore")
        if flags is not None:
            if flags.shape != (n_classes,) or flags.dtype != "int32" \
                    or not flags.flags["C_CONTIGUOUS"]:
                raise ValueError("run_cycle: spread.class_rescore must be "
                                 "int32 [C]")
            cy.class_spread_rescore = flags.ctypes.data
        soft = spread.get("class_soft")
        if soft is not None:
            if soft.shape != (n_classes, SPREAD_MAX_RULES) \
                    or soft.dtype != "float32" \
                    or not soft.flags["C_CONTIGUOUS"]:
                raise ValueError("run_cycle: spread.class_soft must be "
                                 f"float32 [C, {SPREAD_MAX_RULES}]")
            doms = spread["domains"]
            for c in soft.any(axis=1).nonzero()[0]:
                gs = spread["class_group"][c:c + 1]
                if cr is not None and cr[c, 0] >= 2:
                    gs = cr[c, 1:1 + 2 * int(cr[c, 0]):2]
                tw = soft[c, :len(gs)]
                if gs[0] < 0 or (mode is not None and mode[c] != 0) \
                        or soft[c, len(gs):].any() \
                        or not np.isfinite(tw).all() \
                        or int(doms[gs][tw != 0].sum()) \
                        > SPREAD_SOFT_LDS_DOMAINS:
                    raise ValueError(
                        f"run_cycle: class_soft row {c}: finite weights for "
                        "the rules of a spread class only, at most "
                        f"{SPREAD_SOFT_LDS_DOMAINS} domains over the soft "
                        "ones")
            cy.class_spread_soft = soft.ctypes.data
    if devices is not None:
        K, _ = _unit_planes("run_cycle", _CARDS, (
            devices["mem_used"], devices["cores_used"], devices["state"]),
            devices["mem_total"])
        creq = devices["class_req"]
        if creq.shape != (n_classes, 4) or creq.dtype != "int32" \
                or not creq.flags["C_CONTIGUOUS"]:
            raise ValueError("run_cycle: devices.class_req must be int32 "
                             "[C, 4]")
        for row in creq[creq[:, 0] > 0]:
            check_device_request(row[:3])
        _assign_rows("run_cycle", devices["assign"], log_nodes.shape[0], K,
                     "[L, K]")
        cy.card_mem_used = _addr(devices["mem_used"])
        cy.card_cores_used = _addr(devices["cores_used"])
        cy.card_state = _addr(devices["state"])
        cy.card_mem_total = _addr(devices["mem_total"])
        cy.class_dev_req = creq.ctypes.data
        cy.dev_assign = _addr(devices["assign"])
        cy.card_K = K
    if numa is not None:
        Z, zn = _unit_planes("run_cycle", _ZONES, (numa["zone_free"],))
        nreq = numa["class_req"]
        if zn != N or nreq.shape != (n_classes, 2) \
                or nreq.dtype != "int32" or not nreq.flags["C_CONTIGUOUS"]:
            raise ValueError("run_cycle: numa.zone_free must be [Z, N] and "
                             "numa.class_req int32 [C, 2]")
        for row in nreq[nreq[:, 1] != 0]:
            check_numa_request(*row)
        _assign_rows("run_cycle", numa["assign"], log_nodes.shape[0], Z,
                     "[L, Z]")
        cy.zone_free = _addr(numa["zone_free"])
        cy.class_numa_req = nreq.ctypes.data
        cy.numa_assign = _addr(numa["assign"])
        cy.zone_Z = Z
    if rescore is not None:
        flags = rescore["class_rescore"]
        if flags.shape != (n_classes,) or flags.dtype != "int32" \
                or not flags.flags["C_CONTIGUOUS"]:
            raise ValueError("run_cycle: rescore.class_rescore must be "
                             "int32 [C]")
        slot = rescore["slot"]
        if slot.dtype != torch.int32 or slot.numel() < N \
                or not slot.is_contiguous():
            raise ValueError("run_cycle: rescore.slot must be int32 [N]")
        cy.class_rescore = flags.ctypes.data
        cy.rescore_slot = _addr(slot)
    rc = lib.vamd_run_cycle(ctypes.byref(cy), _stream())
    if rc != 0:
        raise RuntimeError(
            f"vamd_run_cycle rejected the call (rc={rc}): the loaded "
            "library and this module disagree on the VamdCycle layout")
