"""Loader for the host-native per-job loops (``_vamd_host`` CPython
extension).

``AllocateAction._apply`` hands the cycle readback to
``_vamd_host.apply_walk`` instead of interpreting the slot walk in Python.
The Python walk stays as the oracle and the fallback:

* ``VAMD_NATIVE_APPLY=0`` (read per cycle) forces the Python walk;
* a failed import makes ONE build attempt, then falls back with a single
  logged warning.  ``native_apply_loaded()`` tells callers which path is
  live so a lost speed-up cannot hide (``smoke()`` asserts it).

The other per-job loops of a cycle (JobTable column scan, fused-run
bundle entries, bulk pod-group phase stores) follow the same scheme under
their own switch, ``VAMD_NATIVE_JOBS=0``; ``native_jobs_enabled()`` is the
per-cycle test and is also false for a stale module without them.

All the native loops run in blocks behind a prefetching lookahead
(``csrc/lookahead.h``).  ``VAMD_HOST_PREFETCH=0`` turns it off; the
extension reads it from the process environment at every call, so
``os.environ`` changes take effect at once.  Results do not depend on it.
"""

from __future__ import annotations

import importlib
import logging
import os

log = logging.getLogger(__name__)

_mod = None
_tried = False


def _import():
    return importlib.import_module("volcano_amd.ops._vamd_host")


def load():
    """The extension module, or None when it can be neither imported nor
    built (warned once)."""
    global _mod, _tried
    if _mod is not None or _tried:
        return _mod
    _tried = True
    try:
        _mod = _import()
    except ImportError as first:
        try:
            from .build import build_host
            build_host(verbose=False)
            importlib.invalidate_caches()
            _mod = _import()
        except Exception as e:
            log.warning("host-native apply unavailable (%s; build: %s) — "
                        "using the Python apply walk", first, e)
            _mod = None
    return _mod


def native_apply_loaded() -> bool:
    return load() is not None


def native_apply_enabled() -> bool:
    """Per-cycle switch: on unless VAMD_NATIVE_APPLY=0 or the module is
    unavailable."""
    if os.environ.get("VAMD_NATIVE_APPLY", "1") == "0":
        return False
    return load() is not None


_JOBS_FUNCS = ("scan_jobs", "bundle_entries", "set_podgroup_phase")


def native_jobs_enabled() -> bool:
    """Per-cycle switch for the per-job loops: on unless VAMD_NATIVE_JOBS=0,
    the module is unavailable, or it predates these functions."""
    if os.environ.get("VAMD_NATIVE_JOBS", "1") == "0":
        return False
    mod = load()
    if mod is None:
        return False
    for name in _JOBS_FUNCS:
        if not hasattr(mod, name):
            return False
    return True
