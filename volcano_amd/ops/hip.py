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

import torch

from .build import LIB_PATH, build

_lib = None


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
        "count_off", "domains", "domain_scratch")]


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
              spread=None):
    """One library call = one whole allocate cycle (plan built host-side).

    ``class_descs`` / ``job_descs`` are host buffers of ``VamdClassDesc`` /
    ``VamdJobDesc``; ``class_tol`` is a host tensor, every other tensor is
    on the device.

    ``spread`` (plans with domain-rule classes only) is a dict:
    ``class_group``/``class_skew`` host int32 numpy [C], ``dom_of`` device
    i32 [G, N], ``count`` device i32 (groups back to back), ``count_off``/
    ``domains`` host int32 numpy [G], ``scratch`` device
    (``spread_scratch``).  An optional ``class_mode`` (host int32 numpy
    [C]: 0 spread, 1 inter-pod affinity, 2 keyed anti-affinity) fills the
    mode column; without it every class of a group is a spread class."""
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
    rc = lib.vamd_run_cycle(ctypes.byref(cy), _stream())
    if rc != 0:
        raise RuntimeError(
            f"vamd_run_cycle rejected the call (rc={rc}): the loaded "
            "library and this module disagree on the VamdCycle layout")
