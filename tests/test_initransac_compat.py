"""ORB_SLAM2::Initializer of cpp/orbslam2_compat.hpp over a stand-in Frame
(tests/cpp/initransac_compat_main.cpp): the rand() draw against a restated draw
after srand(0), FindHomography / FindFundamental against the CPU restatement
(tests/cpp/initransac_ref.c) bit for bit, single (from two threads, as
Initialize calls them) and batched, the batched form against the single one."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam-system_amd")
CPP = os.path.join(ROOT, "tests", "cpp")


def _build(tmp_path):
    exe, ref = tmp_path / "initransac_compat_main", tmp_path / "initransac_ref.o"
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-Wall", "-c", os.path.join(CPP, "initransac_ref.c"),
                           "-o", str(ref)])
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", "-I", os.path.join(PKG, "cpp"), "-I", CPP,
                           os.path.join(CPP, "initransac_compat_main.cpp"), str(ref), "-o", str(exe),
                           "-L", PKG, "-lorbx", "-lm", "-Wl,-rpath," + PKG])
    return exe


def test_call_site_compiles(tmp_path):
    assert _build(tmp_path).exists()


@pytest.mark.gpu
def test_compat_members_equal_the_restatement(gpu, tmp_path):
    r = subprocess.run([str(_build(tmp_path))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "initransac_compat_main: 0 failures" in r.stdout
    assert "draw: 4 of 4 set tables equal the restated draw" in r.stdout
    lines = re.findall(r"^(.+): (\d+) of 23 words, (\d+) of (\d+) flags, RH (\S+), (\d+) H inliers$", r.stdout, re.M)
    assert [l[0] for l in lines] == ["single pair 0", "single pair 1"] + ["batch pair %d" % k for k in range(4)], r.stdout
    for what, words, same, total, _, _ in lines:
        assert words == "23" and same == total, (what, r.stdout)
    assert [l[3] for l in lines] == ["240", "80", "240", "80", "514", "16"]
    assert float(lines[0][4]) > 0.40 >= float(lines[1][4]) and int(lines[0][5]) >= 90
    assert lines[5][5] == "0"  # the pair without an H winner: all flags clear, the matrix left empty
