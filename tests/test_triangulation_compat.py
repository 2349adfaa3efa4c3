"""ORBmatcher::SearchForTriangulation of cpp/orbslam2_compat.hpp: the
reference's parameter list binds (CPU), and the single and the batched
overload on a stand-in KeyFrame return the restatement's vMatchedPairs (GPU;
tests/cpp/tri_compat_main.cpp)."""
import os
import re
import subprocess

import numpy as np
import pytest

import native
from native import ROOT
import triangulation_util as T
from test_signatures import COMPAT, REF, _params, _strip


# include/ORBmatcher.h:51-52; used where the reference header is absent and
# checked against it where it is present
_TRI_DECL = ("int SearchForTriangulation(KeyFrame *pKF1, KeyFrame* pKF2, cv::Mat F12, "
             "std::vector<pair<size_t, size_t> > &vMatchedPairs, const bool bOnlyStereo);")

_TRI_STANDINS = r"""
#include <map>
#include <utility>
#include <vector>
#include "orbslam2_compat.hpp"
namespace ORB_SLAM2 {
class MapPoint {};
class KeyFrame {
 public:
  int N = 0;
  std::vector<cv::KeyPoint> mvKeysUn;
  cv::Mat mDescriptors;
  std::map<unsigned int, std::vector<unsigned int>> mFeatVec;  // DBoW2::FeatureVector
  std::vector<float> mvLevelSigma2;
  MapPoint* GetMapPoint(const size_t &idx) { return nullptr; }
};
}  // namespace ORB_SLAM2
using namespace ORB_SLAM2;
using std::pair;  // the reference's headers sit under `using namespace std`
"""


def _tri_params(decl):
    m = re.search(r"SearchForTriangulation\s*\(([^()]*)\)", decl)
    # _params splits at commas: the pair's own comma is protected first
    ps = _params(m.group(1).replace("size_t, size_t", "size_t@size_t"))
    return tuple(p.replace("@", ",") for p in ps)


def _tri_probe(tmp_path, params):
    src = _TRI_STANDINS + "int (ORBmatcher::*tri)(%s) = &ORBmatcher::SearchForTriangulation;\n" % ", ".join(params)
    p = tmp_path / "tri_sig.cpp"
    p.write_text(src)
    return subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.dirname(COMPAT),
                           "-I", os.path.join(ROOT, "include"), str(p)], capture_output=True, text=True)


def test_search_for_triangulation_binds_reference_signature(tmp_path):
    decl = _TRI_DECL
    if os.path.exists(os.path.join(REF, "ORBmatcher.h")):
        ref = _strip(open(os.path.join(REF, "ORBmatcher.h")).read())
        found = re.findall(r"int SearchForTriangulation\s*\([^()]*\)\s*;", ref)
        assert len(found) == 1 and _tri_params(found[0]) == _tri_params(_TRI_DECL), found
        decl = found[0]
    params = _tri_params(decl)
    assert params == ("KeyFrame*", "KeyFrame*", "cv::Mat", "std::vector<pair<size_t,size_t>>&", "const bool")
    r = _tri_probe(tmp_path, params)
    assert r.returncode == 0, r.stderr


def test_search_for_triangulation_probe_rejects_drifted_signature(tmp_path):
    """The probe is sharp: the pair vector by const reference, or the second
    KeyFrame by reference, does not bind."""
    p = _tri_params(_TRI_DECL)
    assert _tri_probe(tmp_path, p[:3] + ("const " + p[3],) + p[4:]).returncode != 0
    assert _tri_probe(tmp_path, p[:1] + ("KeyFrame&",) + p[2:]).returncode != 0


def _build():
    return native.program("tri_compat_main.cpp")


def test_call_site_compiles():
    assert os.path.exists(_build())


def _write_kf(f, k):
    n, nn = len(k["keys"]), len(k["node_id"])
    f.write(np.array([n, nn, len(k["feat"]), len(k["level_sigma2"])], np.int32).tobytes())
    f.write(np.ascontiguousarray(k["keys"], T.KEYPOINT_DTYPE).tobytes())
    f.write(np.ascontiguousarray(k["desc"], np.uint8).tobytes())
    f.write(np.ascontiguousarray(k["has_mp"], np.uint8).tobytes())
    for name in ("node_id", "off", "feat"):
        f.write(np.ascontiguousarray(k[name], np.uint32).tobytes())
    f.write(np.ascontiguousarray(k["level_sigma2"], np.float32).tobytes())


@pytest.mark.gpu
def test_compat_overloads_return_restatement_pairs(gpu, tmp_path):
    exe = _build()
    nodes1 = {3 * j + 1: 8 + (5 * j) % 11 for j in range(8)}
    kf1, kf2s, Fs = T.make_case(31, nodes1, [{3 * j + 1: 4 + (7 * j + 3 * p) % 13 for j in range(8) if (j + p) % 4}
                                             for p in range(3)])
    m, nm, st = T.ref_batch(kf1, kf2s, Fs)
    assert (nm > 0).all() and (m == -2).any() and sum(s["multi"] for s in st) > 0
    with open(tmp_path / "in.bin", "wb") as f:
        f.write(np.array([len(kf2s)], np.int32).tobytes())
        _write_kf(f, kf1)
        for k in kf2s:
            _write_kf(f, k)
        for F in Fs:
            f.write(np.ascontiguousarray(F, np.float32).tobytes())
    out = tmp_path / "out.txt"
    subprocess.check_call([exe, str(tmp_path / "in.bin"), str(out)], timeout=120)
    # vMatchedPairs (ORBmatcher.cc:459-465): the matched rows in ascending i
    want = [[(int(i), int(m[p, i])) for i in range(m.shape[1]) if m[p, i] >= 0] for p in range(len(kf2s))]
    got = {"S": [[] for _ in kf2s], "B": [[] for _ in kf2s]}
    ns, nb, stereo = {}, None, None
    for line in out.read_text().split("\n"):
        w = line.split()
        if not w:
            continue
        if w[0] in ("S", "B"):
            got[w[0]][int(w[1])].append((int(w[2]), int(w[3])))
        elif w[0] == "NS":
            ns[int(w[1])] = int(w[2])
        elif w[0] == "NB":
            nb = int(w[1])
        elif w[0] == "STEREO":
            stereo = (int(w[1]), int(w[2]))
    assert got["S"] == want
    assert got["B"] == want
    assert [ns[p] for p in range(len(kf2s))] == nm.tolist() and nb == int(nm.sum())
    assert stereo == (0, 0)
