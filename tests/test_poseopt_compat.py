"""ORB_SLAM2::Optimizer::PoseOptimization of cpp/orbslam2_compat.hpp over a
stand-in Frame (tests/cpp/poseopt_compat_main.cpp): the frame's mvbOutlier, the
pose handed to SetPose and the return value against the CPU restatement
(tests/cpp/poseopt_ref.c), single and batched, with the return-0 path."""
import os
import re
import subprocess

import pytest

import native


def _build():
    return native.program("poseopt_compat_main.cpp", ("poseopt_ref.c",))


def test_call_site_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_compat_member_equals_the_restatement(gpu, tmp_path):
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "poseopt_compat_main: 0 failures" in r.stdout
    lines = re.findall(r"^(.+): (\d+) inliers, (\d+) of (\d+) flags, (\d+) of 16 pose words, SetPose x (\d+)$",
                       r.stdout, re.M)
    assert [l[0] for l in lines] == ["single frame"] + ["batch frame %d" % f for f in range(5)], r.stdout
    for what, nin, same, total, words, _ in lines:
        assert same == total and words == "16", (what, r.stdout)
    assert int(lines[0][1]) > 300 and lines[0][5] == "1"
    assert (lines[3][1], lines[3][5]) == ("0", "0") and (lines[4][1], lines[4][5]) == ("0", "0")  # the return-0 path
