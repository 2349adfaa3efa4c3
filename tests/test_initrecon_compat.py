"""ORB_SLAM2::Initializer::Initialize of cpp/orbslam2_compat.hpp over a stand-in
Frame (tests/cpp/initrecon_compat_main.cpp): single and batched over three
initializers against the CPU restatements (tests/cpp/initransac_ref.c,
initrecon_ref.c) bit for bit, ReconstructH / ReconstructF called directly, and
the false path leaving vP3D / vbTriangulated as they were."""
import os
import re
import subprocess

import pytest

import native


def _build():
    return native.program("initrecon_compat_main.cpp", ("initransac_ref.c", "initrecon_ref.c"), ("-pthread",))


def test_call_site_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_initialize_equals_the_restatement(gpu, tmp_path):
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=120)
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
