"""ORBmatcher::SearchForInitialization of cpp/orbslam2_compat.hpp in a loop
shaped like Tracking::MonocularInitialization: the initial frame, then three
frames with mvIniMatches and mvbPrevMatched carried along, compared line by
line with a straight host loop written from src/ORBmatcher.cc:197-276 on the
same stand-in Frame class (tests/cpp/init_compat_main.cpp)."""
import os
import subprocess

import pytest

import native


def _build():
    return native.program("init_compat_main.cpp")


def test_call_site_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_compat_member_equals_the_host_loop(gpu, tmp_path):
    exe = _build()
    out = tmp_path / "out.txt"
    subprocess.check_call([exe, "7", str(out)], timeout=120)
    got = {"H": [], "D": []}
    for line in out.read_text().split("\n"):
        w = line.split()
        if w:
            got[w[0]].append(tuple(w[1:]))
    H, D = got["H"], got["D"]
    # not vacuous, on the host loop alone: every frame matches, entries
    # survive from one frame to the next, and the carried positions move
    ret = {int(x[1]): int(x[2]) for x in H if x[0] == "RET"}
    assert sorted(ret) == [0, 1, 2, 10, 11] and all(v > 20 for v in ret.values()), ret
    rows = {}
    for x in H:
        if x[0] == "M":
            rows.setdefault(int(x[1]), []).append((int(x[3]), x[4], x[5]))
    for k in (1, 2):
        held = sum(1 for m in rows[k] if m[0] >= 0)
        assert held > ret[k], (k, held, ret[k])  # stale survivors beside this call's matches
        assert sum(1 for a, b in zip(rows[k - 1], rows[k]) if a[1:] != b[1:]) > 20
    assert len(rows[0]) == 400
    assert D == H, [x for x in zip(H, D) if x[0] != x[1]][:5]
