"""ORBmatcher::Fuse (both forms), the batched Fuse and SearchBySim3 of
cpp/orbslam2_compat.hpp with SetKfProjection(KfProjection::Device): on the
stand-in classes of tests/cpp/kfwin_mocks.hpp each returns what the CPU
restatement of the projection (tests/cpp/kfbuild_ref.c) followed by the
reference's search and walk returns on the same planted scene: the same return
value, the same Replace / AddObservation / AddMapPoint events in the same
order, the same final GetMapPoint table (GPU; tests/cpp/kfbuild_compat_main.cpp)."""
import os
import subprocess

import pytest

import native
from native import PKG


def _build():
    return native.program("kfbuild_compat_main.cpp", ("kfbuild_ref.c",))


def test_call_site_compiles():
    assert os.path.exists(_build())


def test_switch_defaults_to_the_host_projection():
    src = open(os.path.join(PKG, "cpp", "orbslam2_compat.hpp")).read()
    assert "KfProjection mKfProjection = KfProjection::Host;" in src


@pytest.mark.gpu
def test_device_projection_members_equal_restatement_and_walk(gpu, tmp_path):
    exe = _build()
    out = tmp_path / "out.txt"
    subprocess.check_call([exe, "7", str(out)], timeout=120)
    got, counts = {}, None
    for line in out.read_text().split("\n"):
        w = line.split()
        if w and w[0] == "RS":
            counts = (int(w[2]), int(w[4]))
        elif w:
            got.setdefault((w[0], w[1]), []).append(tuple(w[2:]))
    # the restatement projected, and rejected, a good share of the points
    assert counts and counts[0] > 2000 and 0.3 * counts[0] < counts[1] < counts[0], counts
    for mode in ("FUSE", "SCW", "SIM3", "BATCH"):
        H, D = got[(mode, "H")], got[(mode, "D")]
        kinds = lambda k: [x for x in H if x[0] == k]
        ret = int(kinds("RET")[0][1])
        ev = kinds("EV")
        assert ret > 20, (mode, ret)  # not vacuous, on the restatement's side alone
        if mode in ("FUSE", "BATCH"):
            nrep = len([e for e in ev if e[1] == "R"])
            nadd = len([e for e in ev if e[1] == "M"])
            assert nrep > 5 and nadd > 5 and ret > nrep + nadd, (mode, ret, nrep, nadd)
        if mode == "BATCH":
            assert len({e[2] for e in ev if e[1] == "M"}) == 5  # AddMapPoint in every keyframe
        if mode == "SCW":
            assert len(kinds("OUT")) > 5 and len([e for e in ev if e[1] == "M"]) > 5
        if mode == "SIM3":
            assert len(kinds("OUT")) > 5 and not ev
        assert D == H, (mode, [x for x in zip(H, D) if x[0] != x[1]][:5])
