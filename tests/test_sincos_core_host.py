"""orbx_sincos_core on the host: the exact-floor, branch-free quadrant form of
csrc/orbx_sincos.h against a verbatim copy of the form it replaced
(tests/cpp/sincos_core_cmp.c: (double)(int64_t) floor with a fix-up, switch on
doubles).  Same -ffp-contract=off as the library and the table generator.

Inputs: every float within 64 ulp of each multiple of pi/4 up to 2 pi (where
the floor steps and where sin / cos cross zero), 0, the largest reachable
angle 0x40c90fdb, denormals, and 2^20 evenly strided bit patterns of the
reachable range.  The two forms must agree in every bit of sin and cos.
"""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "sincos_core_cmp.c")


def test_sincos_core_equals_previous_form(tmp_path):
    exe = tmp_path / "sincos_core_cmp"
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-o", str(exe),
                           SRC, "-lm"])
    r = subprocess.run([str(exe)], stdout=subprocess.PIPE, universal_newlines=True)
    print(r.stdout)
    m = re.search(r"checked (\d+) differences (\d+)", r.stdout)
    assert m, r.stdout
    assert int(m.group(1)) > (1 << 20) + 9 * 100
    assert int(m.group(2)) == 0 and r.returncode == 0, r.stdout
