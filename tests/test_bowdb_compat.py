"""KeyFrameDatabase and ORBVocabulary::score of cpp/orbslam2_compat.hpp through
a sequence shaped like LoopClosing::DetectLoop / Tracking::Relocalization
calls: adds, loop queries, relocalisation queries and an erase, compared line
by line -- candidate vectors and the six members the reference writes, of
every keyframe, after every step -- with a straight host loop written from
src/KeyFrameDatabase.cc on a second copy of the same stand-in classes and
covisibility graph (tests/cpp/bowdb_compat_main.cpp)."""
import os
import subprocess

import pytest

import native

PLANTED = "3e800000"  # 0.25f, what mLoopScore / mRelocScore start at


def _build():
    return native.program("bowdb_compat_main.cpp")


def _run(exe, tmp_path, *mode):
    out = tmp_path / "out.txt"
    subprocess.check_call([exe, "7", str(out), str(tmp_path / "voc.txt")] + list(mode), timeout=120)
    got = {"H": [], "D": [], "X": []}
    for line in out.read_text().split("\n"):
        w = line.split()
        if w:
            got[w[0]].append(tuple(w[1:]))
    return got


def _host_loop_conditions(H, X):
    """on the host loop's output alone: the sequence contains what it is for"""
    ret = {int(x[1]): int(x[2]) for x in H if x[0] == "RET"}
    assert sorted(ret) == list(range(1, 10))
    assert max(ret.values()) >= 2                                  # some query returns >= 2 candidates
    x = {}
    for r in X:
        x.setdefault(r[1], {})[int(r[0])] = [int(v) for v in r[2:] if v.lstrip("-").isdigit()]
    assert any(v[0] > 0 for v in x["GATE"].values())               # a sharing keyframe under the word gate
    assert any(v[0] > 0 for v in x["BEST"].values())               # a neighbour changes pBestKF
    assert any(v[0] > 0 for v in x["STALE"].values())              # (c) a stale score changes an accumulated one
    rows = {}
    for r in H:
        if r[0] == "K":  # step, id, loop query / words / score, reloc query / words / score
            rows[(int(r[1]), int(r[2]))] = (int(r[3]), int(r[4]), r[5], int(r[6]), int(r[7]), r[8])
    # (a) step 1: the query (keyframe 20, mnId 30) has its neighbours 18 and 19 in the database: they share
    # words, are never stamped and end with one word
    assert x["LOOP"][1][0] > 0
    for kid in (28, 29):
        assert rows[(1, kid)][:3] == (0, 1, PLANTED)
    assert any(rows[(1, k)][0] == 30 and rows[(1, k)][1] > 1 for k in range(10, 28))
    # (b) step 2: the same id again: nothing returned, nobody reset, the counts only grow
    assert ret[1] > 0 and ret[2] == 0 and x["LOOP"][2][1] > 0
    stamped = [k for k in range(10, 28) if rows[(1, k)][0] == 30]
    assert stamped and all(rows[(2, k)][1] == 2 * rows[(1, k)][1] for k in stamped)
    assert all(rows[(2, k)][2] == rows[(1, k)][2] for k in stamped)
    # (c) step 4: keyframes stamped by the relocalisation query but under its gate still hold the planted score
    assert any(rows[(4, k)][3] == 100 and rows[(4, k)][5] == PLANTED for k in range(10, 36))
    assert any(rows[(4, k)][3] == 100 and rows[(4, k)][5] != PLANTED for k in range(10, 36))
    return ret


def test_call_site_compiles():
    assert os.path.exists(_build())


def test_host_loop_contains_every_quirk(tmp_path):
    got = _run(_build(), tmp_path, "host")  # the host loop alone: no GPU
    assert not got["D"]
    _host_loop_conditions(got["H"], got["X"])


@pytest.mark.gpu
def test_compat_database_equals_the_host_loop(gpu, tmp_path):
    got = _run(_build(), tmp_path)
    H, D, X = got["H"], got["D"], got["X"]
    _host_loop_conditions(H, X)
    assert ("0", "SCORE", "differ", "0") in X  # ORBVocabulary::score, single and batched
    assert len(H) > 200
    assert D == H, [x for x in zip(H, D) if x[0] != x[1]][:5]
