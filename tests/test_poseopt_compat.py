"""ORB_SLAM2::Optimizer::PoseOptimization of cpp/orbslam2_compat.hpp over a
stand-in Frame (tests/cpp/poseopt_compat_main.cpp): the frame's mvbOutlier, the
pose handed to SetPose and the return value against the CPU restatement
(tests/cpp/poseopt_ref.c), single and batched, with the return-0 path."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam-system_amd")
CPP = os.path.join(ROOT, "tests", "cpp")


def _build(tmp_path):
    exe, ref = tmp_path / "poseopt_compat_main", tmp_path / "poseopt_ref.o"
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-Wall", "-c", os.path.join(CPP, "poseopt_ref.c"),
                           "-o", str(ref)])
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(PKG, "cpp"), "-I", CPP,
                           os.path.join(CPP, "poseopt_compat_main.cpp"), str(ref), "-o", str(exe),
                           "-L", PKG, "-lorbx", "-lm", "-Wl,-rpath," + PKG])
    return exe


def test_call_site_compiles(tmp_path):
    assert _build(tmp_path).exists()


@pytest.mark.gpu
def test_compat_member_equals_the_restatement(gpu, tmp_path):
    r = subprocess.run([str(_build(tmp_path))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "poseopt_compat_main: 0 failures" in r.stdout
    lines = re.findall(r"^(.+): (\d+) inliers, (\d+) of (\d+) flags, (\d+) of 16 pose words, SetPose x (\d+)$",
                       r.stdout, re.M)
    assert [l[0] for l in lines] == ["single frame"] + ["batch frame %d" % f for f in range(5)], r.stdout
    for what, nin, same, total, words, _ in lines:
        assert same == total and words == "16", (what, r.stdout)
    assert int(lines[0][1]) > 300 and lines[0][5] == "1"
    assert (lines[3][1], lines[3][5]) == ("0", "0") and (lines[4][1], lines[4][5]) == ("0", "0")  # the return-0 path
