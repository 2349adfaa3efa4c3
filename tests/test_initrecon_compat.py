"""ORB_SLAM2::Initializer::Initialize of cpp/orbslam2_compat.hpp over a stand-in
Frame (tests/cpp/initrecon_compat_main.cpp): single and batched over three
initializers against the CPU restatements (tests/cpp/initransac_ref.c,
initrecon_ref.c) bit for bit, ReconstructH / ReconstructF called directly, and
the false path leaving vP3D / vbTriangulated as they were."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam-system_amd")
CPP = os.path.join(ROOT, "tests", "cpp")


def _build(tmp_path):
    exe = tmp_path / "initrecon_compat_main"
    objs = []
    for name in ("initransac_ref", "initrecon_ref"):
        o = tmp_path / (name + ".o")
        subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-fno-strict-aliasing", "-Wall", "-c",
                               os.path.join(CPP, name + ".c"), "-o", str(o)])
        objs.append(str(o))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-pthread", "-I", os.path.join(PKG, "cpp"), "-I", CPP,
                           os.path.join(CPP, "initrecon_compat_main.cpp")] + objs +
                          ["-o", str(exe), "-L", PKG, "-lorbx", "-lm", "-Wl,-rpath," + PKG])
    return exe


def test_call_site_compiles(tmp_path):
    assert _build(tmp_path).exists()


@pytest.mark.gpu
def test_initialize_equals_the_restatement(gpu, tmp_path):
    r = subprocess.run([str(_build(tmp_path))], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "initrecon_compat_main: 0 failures" in r.stdout
    assert "false path: vP3D and vbTriangulated untouched" in r.stdout
    lines = re.findall(r"^(.+): ok (\d), model (\d), (\d+) of (\d+) words, (\d+) of (\d+) flags, (\d+) triangulated", r.stdout,
                       re.M)
    assert [l[0] for l in lines] == ["single pair 0", "single pair 1", "ReconstructF pair 1", "ReconstructH pair 0",
                                     "batch pair 1", "batch pair 2", "batch pair 3"], r.stdout
    for what, ok, model, words, total, flags, nflags, ntri in lines:
        assert words == total and flags == nflags, (what, r.stdout)
    assert [l[1] for l in lines] == ["1", "1", "1", "1", "1", "1", "0"]
    assert [l[2] for l in lines[:4]] == ["0", "1", "1", "0"]  # planar through H, general through F
    assert all(int(l[7]) >= 50 for l in lines[:6])
