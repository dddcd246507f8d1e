"""In-tree build of the native libraries (no JIT cache).

Two targets:

* ``_vamd_hip.so`` — the HIP kernel library (gfx950 only).  Pure HIP with
  a C ABI (ctypes-loaded) — no torch/pybind link, so there is nothing to
  version-match.  ``hipcc --offload-arch=gfx950`` cross-compiles fine on a
  GPU-less box; the produced ``.so`` travels to the GPU box with the repo
  snapshot.
* ``_vamd_host<EXT_SUFFIX>`` — the host-native apply walk, a CPython
  extension compiled by the same ``hipcc`` in host-only mode.  Not linked
  against libpython; the interpreter-tagged file name turns an
  interpreter mismatch into an import error.
"""

from __future__ import annotations

import os
import subprocess
import sysconfig
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
CSRC = PKG_DIR / "csrc"
LIB_PATH = PKG_DIR / "_vamd_hip.so"
SOURCES = ["scheduler_kernels.hip", "cycle_runner.hip"]
HOST_LIB_PATH = PKG_DIR / ("_vamd_host" + (
    sysconfig.get_config_var("EXT_SUFFIX") or ".so"))
HOST_SOURCES = ["vamd_host.cpp"]
HOST_DEPS = HOST_SOURCES + ["settle_core.h", "lookahead.h"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ARCH = os.environ.get("VAMD_GPU_ARCH", "gfx950")


def _mtime(p: Path) -> float:
    try:
        return p.stat().st_mtime
    except FileNotFoundError:
        return 0.0


def _stale(out: Path, deps) -> bool:
    if not out.exists():
        return True
    out_t = _mtime(out)
    return any(_mtime(CSRC / d) > out_t for d in deps)


def needs_build_hip() -> bool:
    return _stale(LIB_PATH, SOURCES + ["vamd_api.h"])


def needs_build_host() -> bool:
    return _stale(HOST_LIB_PATH, HOST_DEPS)


def needs_build() -> bool:
    return needs_build_hip() or needs_build_host()


def build_host(force: bool = False, verbose: bool = True) -> Path:
    if not force and not needs_build_host():
        return HOST_LIB_PATH
    # compile to a private name, then rename: a concurrent importer never
    # sees a half-written module
    tmp = HOST_LIB_PATH.with_name(f".{HOST_LIB_PATH.name}.{os.getpid()}.tmp")
    cmd = [
        HIPCC, "-x", "c++", "-O2", "-std=c++17", "-fPIC", "-shared",
        f"-I{sysconfig.get_paths()['include']}", "-o", str(tmp),
    ] + [str(CSRC / s) for s in HOST_SOURCES]
    if verbose:
        print("[vamd build]", " ".join(cmd), flush=True)
    try:
        subprocess.run(cmd, check=True, cwd=str(CSRC))
        os.replace(tmp, HOST_LIB_PATH)
    finally:
        if tmp.exists():
            tmp.unlink()
    return HOST_LIB_PATH


def build(force: bool = False, verbose: bool = True) -> Path:
    if force or needs_build_hip():
        cmd = [
            HIPCC, f"--offload-arch={ARCH}", "-O3", "-std=c++17",
            "-fPIC", "-shared", "-o", str(LIB_PATH),
        ] + [str(CSRC / s) for s in SOURCES]
        if verbose:
            print("[vamd build]", " ".join(cmd), flush=True)
        subprocess.run(cmd, check=True, cwd=str(CSRC))
    build_host(force=force, verbose=verbose)
    return LIB_PATH


if __name__ == "__main__":
    build(force="--force" in os.sys.argv)
