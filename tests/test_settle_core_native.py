"""Core-only test of the settle walk: a stand-alone C++ program
(``tests/native/settle_core_main.cpp``) replays the fixed cases and the
boundary sizes against ``volcano_amd/ops/csrc/settle_core.h`` under
AddressSanitizer + UndefinedBehaviorSanitizer.  Host code only, run as a
plain subprocess; the CPython extension itself is not sanitizer-tested.
"""

import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "settle_core_main.cpp"
INC = ROOT / "volcano_amd" / "ops" / "csrc"
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
# preferred first: runtimes linked into the program itself, so nothing
# depends on the order in which shared libraries load
SAN_VARIANTS = [SAN + ["-static-libasan", "-static-libubsan"],
                SAN + ["-static-libsan"], SAN]


def _compiler():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cand and shutil.which(cand):
            return shutil.which(cand)
    return None


def _usable(cxx, flags, tmp_path):
    probe = tmp_path / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    exe = tmp_path / "probe"
    got = subprocess.run([cxx, *flags, str(probe), "-o", str(exe)],
                         capture_output=True, text=True)
    return got.returncode == 0 and subprocess.run(
        [str(exe)], capture_output=True).returncode == 0


def test_settle_core_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    san = next((f for f in SAN_VARIANTS if _usable(cxx, f, tmp_path)), None)
    if san is None:
        pytest.skip("host compiler has no usable sanitizer runtime")

    exe = tmp_path / "settle_core_main"
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *san,
         f"-I{INC}", str(SRC), "-o", str(exe)],
        capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True,
                         timeout=60)
    assert run.returncode == 0, run.stdout + run.stderr
    assert run.stderr == "", run.stderr
    assert "settle core OK" in run.stdout
