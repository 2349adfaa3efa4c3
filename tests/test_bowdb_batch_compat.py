"""KeyFrameDatabase::DetectRelocalizationCandidates(const std::vector<FR*>&) of
cpp/orbslam2_compat.hpp over four frames -- one orbv_db_query_batch, then the
host step per frame in list order -- against four calls of the single form on
a second copy of the same stand-in graph (tests/cpp/bowdb_batch_compat_main.cpp
over the classes of tests/cpp/bowdb_compat_main.cpp): the candidate vectors of
every frame and the six members of every keyframe, line by line."""
import os
import subprocess

import pytest

import native


def _build():
    return native.program("bowdb_batch_compat_main.cpp", extra=("-Wno-unused-function",))


def test_batched_call_site_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_batched_relocalization_equals_the_single_calls(gpu, tmp_path):
    out = tmp_path / "out.txt"
    subprocess.check_call([_build(), "7", str(out), str(tmp_path / "voc.txt")], timeout=120)
    got = {"H": [], "D": [], "X": {}}
    for line in out.read_text().split("\n"):
        w = line.split()
        if w and w[0] == "X":
            got["X"][w[1]] = [int(x) for x in w[2:] if x.isdigit()]
        elif w:
            got[w[0]].append(tuple(w[1:]))
    H, D, X = got["H"], got["D"], got["X"]
    # on the single calls alone: the sequence contains what it is for
    ret = {int(r[1]): int(r[2]) for r in H if r[0] == "RET"}
    assert sorted(ret) == [0, 1, 2, 3] and X["candidates"][0] >= 2 and sum(1 for v in ret.values() if v) >= 2
    assert X["reversed_differ"][0] > 0           # the frames' order matters to what is left behind
    assert X["stamped"][0] >= 10 and 0 < X["stamped"][1] < X["stamped"][0]  # stamped keyframes under the gate
    assert len([r for r in H if r[0] == "K"]) == 26
    assert D == H, [x for x in zip(H, D) if x[0] != x[1]][:5]
