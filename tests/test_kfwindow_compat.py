"""ORBmatcher::Fuse (both forms), SearchBySim3 and the batched Fuse of
cpp/orbslam2_compat.hpp: the reference's parameter lists bind (CPU), and on
stand-in KeyFrame / MapPoint classes each returns what a straight host loop
written from src/ORBmatcher.cc:504-730 returns on the same planted scene: the
same return value, the same Replace / AddObservation / AddMapPoint events in
the same order and the same final GetMapPoint table (GPU;
tests/cpp/kfwin_compat_main.cpp)."""
import os
import re
import subprocess

import pytest

import native
from native import CPP, ROOT
from test_signatures import COMPAT, REF, _params, _strip


# include/ORBmatcher.h:56-62; used where the reference header is absent and
# checked against it where it is present
_DECLS = {
    "SearchBySim3": ["int SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint *> &vpMatches12, "
                     "const float &s12, const cv::Mat &R12, const cv::Mat &t12, const float th);"],
    "Fuse": ["int Fuse(KeyFrame* pKF, const vector<MapPoint *> &vpMapPoints, const float th=3.0);",
             "int Fuse(KeyFrame* pKF, cv::Mat Scw, const std::vector<MapPoint*> &vpPoints, float th, "
             "vector<MapPoint *> &vpReplacePoint);"],
}
# the batched form has no counterpart in the reference
_BATCHED = ("const std::vector<KeyFrame*>&", "const std::vector<MapPoint*>&", "const float")

_PRELUDE = '#include "kfwin_mocks.hpp"\nusing namespace ORB_SLAM2;\nusing std::vector;\n'


def _lists(name, decls):
    return [_params(re.search(r"%s\s*\(([^()]*)\)" % name, d).group(1)) for d in decls]


def _reference_lists():
    """{name: parameter lists}, from the reference header where it is present"""
    out = {}
    have = os.path.exists(os.path.join(REF, "ORBmatcher.h"))
    ref = _strip(open(os.path.join(REF, "ORBmatcher.h")).read()) if have else ""
    for name, decls in _DECLS.items():
        if have:
            found = re.findall(r"int %s\s*\([^()]*\)\s*;" % name, ref)
            assert _lists(name, found) == _lists(name, decls), found
            decls = found
        out[name] = _lists(name, decls)
    return out


def _probe(tmp_path, binds):
    """binds: (member name, parameter list) pairs, each bound to a member
    function pointer of exactly that type"""
    src = _PRELUDE
    for i, (name, ps) in enumerate(binds):
        src += "int (ORBmatcher::*f%d)(%s) = &ORBmatcher::%s;\n" % (i, ", ".join(ps), name)
    p = tmp_path / "kfw_sig.cpp"
    p.write_text(src)
    return subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.dirname(COMPAT), "-I", CPP,
                           "-I", os.path.join(ROOT, "include"), str(p)], capture_output=True, text=True)


def test_fuse_and_sim3_bind_reference_signatures(tmp_path):
    L = _reference_lists()
    assert L["SearchBySim3"] == [("KeyFrame*", "KeyFrame*", "std::vector<MapPoint*>&", "const float&",
                                  "const cv::Mat&", "const cv::Mat&", "const float")]
    assert L["Fuse"] == [("KeyFrame*", "const vector<MapPoint*>&", "const float"),
                         ("KeyFrame*", "cv::Mat", "const std::vector<MapPoint*>&", "float",
                          "vector<MapPoint*>&")]
    binds = [("SearchBySim3", L["SearchBySim3"][0]), ("Fuse", L["Fuse"][0]), ("Fuse", L["Fuse"][1]),
             ("Fuse", _BATCHED)]
    r = _probe(tmp_path, binds)
    assert r.returncode == 0, r.stderr


def test_probe_rejects_drifted_signatures(tmp_path):
    """The probe is sharp: the candidate list by non-const reference, the
    replace list by const reference, s12 by value, or the target keyframes by
    value, do not bind."""
    sim3 = _lists("SearchBySim3", _DECLS["SearchBySim3"])[0]
    f1, f2 = _lists("Fuse", _DECLS["Fuse"])
    assert _probe(tmp_path, [("Fuse", f1)]).returncode == 0
    assert _probe(tmp_path, [("Fuse", (f1[0], "vector<MapPoint*>&", f1[2]))]).returncode != 0
    assert _probe(tmp_path, [("Fuse", f2[:4] + ("const " + f2[4],))]).returncode != 0
    assert _probe(tmp_path, [("SearchBySim3", sim3[:3] + ("float",) + sim3[4:])]).returncode != 0
    assert _probe(tmp_path, [("Fuse", ("std::vector<KeyFrame*>",) + _BATCHED[1:])]).returncode != 0


def _build():
    return native.program("kfwin_compat_main.cpp")


def test_call_site_compiles():
    assert os.path.exists(_build())


@pytest.mark.gpu
def test_compat_members_equal_the_host_loop(gpu, tmp_path):
    exe = _build()
    out = tmp_path / "out.txt"
    subprocess.check_call([exe, "7", str(out)], timeout=120)
    got = {}
    for line in out.read_text().split("\n"):
        w = line.split()
        if w:
            got.setdefault((w[0], w[1]), []).append(tuple(w[2:]))
    for mode in ("FUSE", "SCW", "SIM3", "BATCH"):
        H, D = got[(mode, "H")], got[(mode, "D")]
        kinds = lambda k: [x for x in H if x[0] == k]
        ret = int(kinds("RET")[0][1])
        ev = kinds("EV")
        # not vacuous, on the host loop alone
        assert ret > 20, (mode, ret)
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
        # the same return value, events in order, final table and output vector
        assert D == H, (mode, [x for x in zip(H, D) if x[0] != x[1]][:5])
