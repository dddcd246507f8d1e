"""The interpreter-internal dict layout that ``lookahead.h`` mirrors, checked
against the interpreter's own lookups: a stand-alone C++ program
(``tests/native/lookahead_main.cpp``) embeds Python, builds dicts of every
index width (with deleted entries, enum and tuple keys, split and combined
instance dicts) and compares ``dict_value`` / ``inst_dict`` with
``PyDict_Next`` / ``PyObject_GenericGetDict`` under AddressSanitizer +
UndefinedBehaviorSanitizer.  Host code only, run as a plain subprocess.
"""

import subprocess
import sysconfig
from pathlib import Path

import pytest

from test_settle_core_native import SAN_VARIANTS, _compiler, _usable

ROOT = Path(__file__).resolve().parent.parent
SRC = ROOT / "tests" / "native" / "lookahead_main.cpp"
INC = ROOT / "volcano_amd" / "ops" / "csrc"


def test_dict_layout_mirror_under_sanitizers(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    san = next((f for f in SAN_VARIANTS if _usable(cxx, f, tmp_path)), None)
    if san is None:
        pytest.skip("host compiler has no usable sanitizer runtime")
    var = sysconfig.get_config_var
    ver = var("LDVERSION") or var("VERSION")
    link = [f"-L{var('LIBPL')}", f"-L{var('LIBDIR')}", f"-lpython{ver}",
            *(var("LIBS") or "").split(), *(var("SYSLIBS") or "").split()]
    exe = tmp_path / "lookahead_main"
    build = subprocess.run(
        [cxx, "-std=c++17", "-O1", "-g", *san, f"-I{INC}",
         f"-I{sysconfig.get_paths()['include']}", str(SRC), "-o", str(exe),
         *link], capture_output=True, text=True)
    if build.returncode != 0 and "-lpython" in build.stderr:
        pytest.skip("no embeddable libpython on this host")
    assert build.returncode == 0, build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "lookahead OK" in run.stdout
    assert int(run.stdout.split(":")[1].split()[0]) > 100000
