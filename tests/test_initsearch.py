"""ORBmatcher::SearchForInitialization on the CPU: the restatement
(tests/cpp/initsearch_ref.c) against an independent brute force in numpy and
against hand-made known answers, and the reference's parameter list against
the member of cpp/orbslam2_compat.hpp.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

import initsearch_util as U
from kfwindow_util import frame_dict
from test_signatures import COMPAT, REF, _params, _strip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def _desc(bits):
    """the zero descriptor with its first `bits` bits set: distance `bits` to zero"""
    d = np.zeros(32, np.uint8)
    for b in range(bits):
        d[b >> 3] |= np.uint8(1 << (b & 7))
    return d


def _frame(rows):
    """rows of (x, y, octave, angle, descriptor or number of set bits)"""
    keys = U.make_keys([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows])
    desc = np.array([_desc(r[4]) if np.isscalar(r[4]) else r[4] for r in rows], np.uint8).reshape(-1, 32)
    return frame_dict(keys, desc)


def _both(pair, **kw):
    """the restatement's result, checked against the brute force"""
    rc, m12, prev, nm, st = U.ref_search(pair, **kw)
    assert rc == 0
    bm, bp, bn = U.brute_force(pair, **kw)
    assert np.array_equal(m12, bm) and np.array_equal(prev.view(np.uint32), bp.view(np.uint32)) and nm == bn
    return m12, prev, nm, st


# --------------------------------------------------------------------------- known answers
def test_a_later_row_steals_a_closer_feature():
    f1 = _frame([(100, 100, 0, 0, 10), (101, 100, 0, 0, 2), (102, 100, 0, 0, 6)])
    f2 = _frame([(100, 100, 0, 0, 0)])
    m12, prev, nm, st = _both(U.first_pair(f1, f2), window_size=10)
    # row 0 takes it at 10, row 1 steals it at 2, row 2 at 6 is filtered out
    assert m12.tolist() == [-1, 0, -1] and nm == 1
    assert st["accepted"].tolist() == [1, 1, 0] and st["displaced"].tolist() == [1, 0, 0]
    assert st["filter_changed"].tolist() == [0, 0, 1]
    assert prev.tolist() == [[100, 100], [100, 100], [102, 100]]


def test_tie_goes_to_the_first_visited_not_the_lowest_index():
    # feature 0 lies in a later column of the grid than feature 1
    f1 = _frame([(100, 100, 0, 0, 0)])
    f2 = _frame([(130, 100, 0, 0, 5), (90, 100, 0, 0, 5)])
    m12, _, nm, _ = _both(U.first_pair(f1, f2), window_size=50, nnratio=2.0)
    assert m12.tolist() == [1] and nm == 1


def test_second_best_equal_to_best_rejects():
    f1 = _frame([(100, 100, 0, 0, 0)])
    f2 = _frame([(130, 100, 0, 0, 5), (90, 100, 0, 0, 5)])
    m12, _, nm, st = _both(U.first_pair(f1, f2), window_size=50, nnratio=0.9)
    assert m12.tolist() == [-1] and nm == 0 and st["ratio_rejected"].tolist() == [1]
    # a distinct second best accepts
    f2 = _frame([(130, 100, 0, 0, 5), (90, 100, 0, 0, 6)])
    assert _both(U.first_pair(f1, f2), window_size=50, nnratio=0.9)[0].tolist() == [0]


def _histogram_case(with_displaced):
    """11 rows in bin 0 each with a feature of its own; row Z in bin 5; and,
    if asked, a row D in bin 5 that a later row S (bin 0) displaces.  Bin 5
    survives ComputeThreeMaxima only with two entries (1 < 0.1 * 12)."""
    r1, r2 = [], []
    for k in range(11):
        r1.append((40 + 50 * k, 60, 0, 0, 0))
        r2.append((40 + 50 * k, 60, 0, 0, 1))
    r1.append((100, 300, 0, 150, 0))  # Z: rot 150 -> bin 5
    r2.append((100, 300, 0, 0, 1))
    if with_displaced:
        r1.append((300, 300, 0, 150, 10))  # D, then S
        r1.append((301, 300, 0, 0, 2))
        r2.append((300, 300, 0, 0, 0))
    else:
        r1.append((301, 300, 0, 0, 2))  # S alone: bin 0 holds 12 either way
        r2.append((300, 300, 0, 0, 0))
    return U.first_pair(_frame(r1), _frame(r2))


def test_a_displaced_row_still_counts_in_the_histogram():
    m12, _, nm, st = _both(_histogram_case(True), window_size=10)
    assert st["displaced"].tolist()[12] == 1 and m12[12] == -1
    assert m12[11] == 11 and nm == 13  # Z survives: bin 5 holds Z and the displaced D
    m12, _, nm, st = _both(_histogram_case(False), window_size=10)
    assert m12[11] == -1 and st["rot_removed"][11] == 1 and nm == 12


def test_negative_octave_row_matches_an_octave_3_feature():
    f1 = _frame([(100, 100, -1, 0, 0), (200, 200, 0, 0, 0), (300, 300, 1, 0, 0)])
    f2 = _frame([(100, 100, 3, 0, 1), (200, 200, 3, 0, 1), (300, 300, 1, 0, 1)])
    m12, _, nm, _ = _both(U.first_pair(f1, f2), window_size=10)
    # octave 0 admits octave 0 alone; octave 1 is skipped
    assert m12.tolist() == [0, -1, -1] and nm == 1


def test_window_zero_finds_nothing():
    f1 = _frame([(100, 100, 0, 0, 0)])
    f2 = _frame([(100, 100, 0, 0, 0)])
    m12, _, nm, _ = _both(U.first_pair(f1, f2), window_size=0)
    assert m12.tolist() == [-1] and nm == 0
    assert _both(U.first_pair(f1, f2), window_size=1)[0].tolist() == [0]


def test_a_stale_entry_survives_and_moves_prev_matched():
    f1 = _frame([(100, 100, 1, 0, 0), (200, 200, 0, 0, 0), (300, 300, 0, 0, 0)])
    f2 = _frame([(210, 200, 0, 0, 1), (50, 60, 0, 0, 200), (400, 50, 0, 0, 200)])
    pair = U.first_pair(f1, f2)
    pair["match12"][:] = [2, -1, 1]  # as an earlier call left them
    m12, prev, nm, st = _both(pair, window_size=20)
    assert m12.tolist() == [2, 0, 1] and nm == 1  # nmatches counts this call's only
    assert st["stale"].tolist() == [1, 0, 1]
    assert prev.tolist() == [[400, 50], [210, 200], [50, 60]]
    # a survivor past F2 is the reference's out-of-range read
    pair["match12"][0] = 3
    assert U.ref_search(pair, window_size=20)[0] == -1


def test_cut_distance():
    assert U.cut_distance(0.9) == 56 and U.cut_distance(0.6) == 84
    assert U.cut_distance(0.1) == 257 and U.cut_distance(-1.0) == 257 and U.cut_distance(float("nan")) == 257
    assert U.cut_distance(5.0) == 51  # never below TH_LOW + 1


# --------------------------------------------------------------------------- restatement vs brute force
@pytest.mark.parametrize("seed,kw", [(1, {}), (2, dict(nnratio=0.6)), (3, dict(check_ori=False)),
                                     (4, dict(window_size=30)), (5, dict(nnratio=0.1))])
def test_restatement_equals_brute_force_over_three_frames(seed, kw):
    pair, _, _ = U.planted_pair(seed, 150, 150)
    rng = np.random.RandomState(100 + seed)
    seen = dict(steals=0, stale=0, accepted=0)
    for _ in range(3):
        m12, prev, nm, st = _both(pair, **kw)
        s = U.summary(st, len(m12))
        for k in seen:
            seen[k] += s[k]
        pair = U.next_pair(pair, (m12, prev), U.make_f2(rng, pair["f1"], 150))
    if "nnratio" not in kw:
        assert seen["steals"] > 0 and seen["stale"] > 0 and seen["accepted"] > 20, seen


# --------------------------------------------------------------------------- the compat member's parameter list
_DECL = ("int SearchForInitialization(Frame &F1, Frame &F2, std::vector<cv::Point2f> &vbPrevMatched, "
         "std::vector<int> &vnMatches12, int windowSize=10);")  # include/ORBmatcher.h:48
_PRELUDE = ('#include "orbslam2_compat.hpp"\nnamespace ORB_SLAM2 { struct Frame { std::vector<cv::KeyPoint> '
            'mvKeysUn; cv::Mat mDescriptors; float mnMinX, mnMinY, mfGridElementWidthInv, '
            'mfGridElementHeightInv; }; }\nusing namespace ORB_SLAM2;\n')


def _list(decl):
    return _params(re.search(r"SearchForInitialization\s*\(([^()]*)\)", decl).group(1))


def _reference_list():
    path = os.path.join(REF, "ORBmatcher.h")
    if os.path.exists(path):  # checked against the reference header where it is present
        found = re.findall(r"int SearchForInitialization\s*\([^()]*\)\s*;", _strip(open(path).read()))
        assert [_list(f) for f in found] == [_list(_DECL)], found
    return _list(_DECL)


def _probe(tmp_path, params, ret="int"):
    src = _PRELUDE + "%s (ORBmatcher::*f)(%s) = &ORBmatcher::SearchForInitialization;\n" % (ret, ", ".join(params))
    p = tmp_path / "ini_sig.cpp"
    p.write_text(src)
    return subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-I", os.path.dirname(COMPAT), "-I",
                           os.path.join(ROOT, "include"), str(p)], capture_output=True, text=True)


def test_member_binds_the_reference_parameter_list(tmp_path):
    L = _reference_list()
    assert L == ("Frame&", "Frame&", "std::vector<cv::Point2f>&", "std::vector<int>&", "int")
    r = _probe(tmp_path, L)
    assert r.returncode == 0, r.stderr
    # the default window is the reference's
    src = _strip(open(COMPAT).read())
    assert re.search(r"int SearchForInitialization\(FR& F1, FR& F2,[^()]*int windowSize = 10\)", src)
    batched = ("const std::vector<Frame*>&", "const std::vector<Frame*>&",
               "std::vector<std::vector<cv::Point2f> >&", "std::vector<std::vector<int> >&", "int")
    assert _probe(tmp_path, batched, ret="std::vector<int>").returncode == 0


def test_probe_rejects_a_drifted_parameter_list(tmp_path):
    L = _reference_list()
    assert _probe(tmp_path, L[:3] + ("const std::vector<int>&", "int")).returncode != 0
    assert _probe(tmp_path, L[:2] + ("std::vector<cv::Point2f>", L[3], "int")).returncode != 0
    assert _probe(tmp_path, L[:4] + ("float",)).returncode != 0
    assert _probe(tmp_path, ("Frame*", "Frame*") + L[2:]).returncode != 0
    assert _probe(tmp_path, L[:4]).returncode != 0
