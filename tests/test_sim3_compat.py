"""ORB_SLAM2::Sim3Solver of cpp/orbslam2_compat.hpp over stand-in KeyFrame and
MapPoint classes (tests/cpp/sim3_compat_main.cpp): the constructor's filtering,
the rand() draw against a restated draw after srand(0), iterate, find and the
getters against the CPU restatement (tests/cpp/sim3_ref.c) bit for bit, single
and through IterateAll, IterateAll against successive single calls given the
same triples, a continued solver, and two solvers from two threads."""
import os
import re
import subprocess

import pytest

import native
import sim3_util  # noqa: F401  (registers sim3_ref.c's build flags)


def _build():
    return native.program("sim3_compat_main.cpp", ("sim3_ref.c",), ("-pthread",))


def test_call_site_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_compat_members_equal_the_restatement(gpu):
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "sim3_compat_main: 0 failures" in r.stdout
    assert "draw: 3 of 3 triple tables equal the restated draw" in r.stdout
    lines = re.findall(r"^(.+): (\d+) of 37 words, (\d+) of (\d+) flags, it_hit (-?\d+), (\d+) inliers$", r.stdout, re.M)
    want = (["batch solver %d" % k for k in range(3)] + ["single solver %d" % k for k in range(3)] +
            ["continued %d" % k for k in (1, 2, 3)] + ["find", "thread 0", "thread 1"])
    assert [l[0] for l in lines] == want, r.stdout
    for what, words, same, total, _, _ in lines:
        assert words == "37" and same == total, (what, r.stdout)
    assert [l[3] for l in lines[:3]] == ["63", "27", "133"]  # one flag per row of vpMatched12
    by = {l[0]: l for l in lines}
    for k in range(3):  # the scenes are solvable: every solver returns a transformation, single as batched
        assert int(by["batch solver %d" % k][4]) >= 0 and by["batch solver %d" % k][4:] == by["single solver %d" % k][4:]
        assert int(by["batch solver %d" % k][5]) > (12 if k == 1 else 20)
    for k in (1, 2, 3):
        assert by["continued %d" % k][4] == "-1" and by["continued %d" % k][5] == "0"
    assert int(by["find"][4]) >= 0 and int(by["thread 0"][4]) >= 0 and int(by["thread 1"][4]) >= 0
