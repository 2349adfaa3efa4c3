"""ORB_SLAM2::Initializer of cpp/orbslam2_compat.hpp over a stand-in Frame
(tests/cpp/initransac_compat_main.cpp): the rand() draw against a restated draw
after srand(0), FindHomography / FindFundamental against the CPU restatement
(tests/cpp/initransac_ref.c) bit for bit, single (from two threads, as
Initialize calls them) and batched, the batched form against the single one."""
import os
import re
import subprocess

import pytest

import native


def _build():
    return native.program("initransac_compat_main.cpp", ("initransac_ref.c",), ("-pthread",))


def test_call_site_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_compat_members_equal_the_restatement(gpu, tmp_path):
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=120)
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
