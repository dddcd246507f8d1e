"""Dispatch of the whole-cycle runner, without a GPU: a stand-alone C++
program (``tests/native/cycle_trace_main.cpp``) links ``cycle_runner.hip``
as plain host C++ against recording stubs of every launcher and HIP call it
can reach, replays a fixed list of hand-built plans (every branch of the
runner, every ``VAMD_*`` switch, a failing allocation) and prints one line
per call (long plans: the launcher sequence and a hash of the lines).  The
output must equal ``tests/native/cycle_trace.expected`` byte
for byte; that file was recorded from the three positional entry points
that ``vamd_run_cycle(const VamdCycle*)`` replaced.  Built under
AddressSanitizer + UndefinedBehaviorSanitizer, run as a plain subprocess.

The size guard of the entry point is checked through ctypes as well: the
kernel library loads without a GPU and the guarded calls reach no HIP call.
"""

import ctypes
import subprocess
from pathlib import Path

import pytest

from test_settle_core_native import SAN_VARIANTS, _compiler, _usable
from volcano_amd.ops import build as vbuild

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "cycle_trace_main.cpp"
EXPECTED = ROOT / "tests" / "native" / "cycle_trace.expected"
INC = ROOT / "volcano_amd" / "ops" / "csrc"
HIP_INC = Path(vbuild.HIPCC).resolve().parent.parent / "include"


def test_dispatch_trace_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    if not (HIP_INC / "hip" / "hip_runtime.h").exists():
        pytest.skip("no HIP headers next to the HIP compiler")
    san = next((f for f in SAN_VARIANTS if _usable(cxx, f, tmp_path)), None)
    if san is None:
        pytest.skip("host compiler has no usable sanitizer runtime")
    exe = tmp_path / "cycle_trace_main"
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", *san, "-D__HIP_PLATFORM_AMD__",
         f"-I{HIP_INC}", f"-I{INC}", "-x", "c++",
         str(INC / "cycle_runner.hip"), str(SRC), "-o", str(exe)],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, timeout=120)
    assert run.returncode == 0, run.stderr.decode()
    assert run.stderr == b"", run.stderr.decode()
    want = EXPECTED.read_bytes()
    if run.stdout != want:
        got_l, want_l = run.stdout.splitlines(), want.splitlines()
        k = next((i for i, (a, b) in enumerate(zip(got_l, want_l)) if a != b),
                 min(len(got_l), len(want_l)))
        head = max((i for i in range(k + 1) if i < len(want_l)
                    and want_l[i].startswith(b"==")), default=0)
        pytest.fail(
            f"trace differs at line {k + 1} "
            f"({want_l[head].decode() if want_l else ''}):\n"
            f"  want: {want_l[k].decode() if k < len(want_l) else '<end>'}\n"
            f"  got:  {got_l[k].decode() if k < len(got_l) else '<end>'}\n"
            "(the program prints every call of every plan with --full)")


def test_struct_size_guard():
    from volcano_amd.ops import hip

    lib = hip._load()
    cy = hip.VamdCycle(struct_size=ctypes.sizeof(hip.VamdCycle))
    # an empty plan: no class, no job, so not one launch or HIP call
    assert lib.vamd_run_cycle(ctypes.byref(cy), None) == 0
    for off in (8, -8):
        cy.struct_size = ctypes.sizeof(hip.VamdCycle) + off
        assert lib.vamd_run_cycle(ctypes.byref(cy), None) != 0
