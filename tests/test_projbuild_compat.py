"""The device-side projection's call sites of cpp/orbslam2_compat.hpp --
ORBmatcher::SearchLocalPoints and the last-frame and keyframe forms of
SearchByProjection -- over stand-in Frame / KeyFrame / MapPoint classes
(tests/cpp/projbuild_compat_main.cpp): the helper's written-back fields and the
members' matches against the CPU restatement (tests/cpp/projbuild_ref.c)."""
import os
import re
import subprocess

import pytest

import native


def _build():
    return native.program("projbuild_compat_main.cpp", ("projbuild_ref.c",))


def test_call_site_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_compat_members_equal_the_restatement(gpu, tmp_path):
    r = subprocess.run([_build()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "projbuild_compat_main: 0 failures" in r.stdout
    m = re.search(r"SearchLocalPoints: nToMatch (\d+), (\d+) of (\d+) points", r.stdout)
    assert m and int(m.group(1)) >= 100 and m.group(2) == m.group(3), r.stdout
    for what in ("last frame, forward", "last frame, backward", "last frame, mono", "keyframe"):
        m = re.search(re.escape(what) + r": (\d+) matches, (\d+) of (\d+) features", r.stdout)
        assert m and int(m.group(1)) >= 40 and m.group(2) == m.group(3), (what, r.stdout)
