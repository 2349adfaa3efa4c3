"""Initializer's homography / fundamental RANSAC: the CPU
restatement (tests/cpp/initransac_ref.c over csrc/initransac_math.h) alone.  It
is the reference of the GPU tests, so it is checked here against what does not
depend on it: the planted inliers of synthetic two-view scenes, numpy's SVD in
double, and the control flow of Initialize stated case by case.  No GPU."""
import ctypes

import numpy as np
import pytest

import initransac_util as U

# Seeds: the conditions below are properties of a scene and its 60 sets, not of
# the arithmetic, and were checked on this restatement for seeds 1..24.  H's
# flags were exact on every planar scene.  F's flags on a general scene are
# exact only where no planted outlier happens to lie within 1.96 px of its
# epipolar line and one of the 60 sets is good enough to keep every inlier (11
# of 24 seeds); three of those are used.
PLANAR_SEEDS = (1, 2, 3)
GENERAL_SEEDS = (1, 2, 11)
NM, NIT = 120, 60


@pytest.mark.parametrize("seed", PLANAR_SEEDS)
def test_planar_scene_selects_h_and_flags_the_planted_inliers(seed):
    _, truth = U.scene("planar", NM, seed, NIT)
    r = U.scene_ref("planar", NM, seed, NIT)
    assert r["nmatch"] == NM and truth["planted"].sum() == 96
    assert r["RH"] > 0.40, r["RH"]  # measured 0.491 .. 0.492
    assert np.array_equal(r["inliers_H"], truth["planted"])
    assert r["it_H"] >= 0 and r["it_F"] >= 0


@pytest.mark.parametrize("seed", GENERAL_SEEDS)
def test_general_scene_selects_f_and_flags_the_planted_inliers(seed):
    _, truth = U.scene("general", NM, seed, NIT)
    r = U.scene_ref("general", NM, seed, NIT)
    assert r["RH"] <= 0.40, r["RH"]  # measured 0.081 .. 0.118
    assert np.array_equal(r["inliers_F"], truth["planted"])


def _all_scenes():
    return [(k, s) for k, seeds in (("planar", PLANAR_SEEDS), ("general", GENERAL_SEEDS)) for s in seeds]


def _normalised_sets(kind, seed):
    """the 8 normalised point pairs of every set of a scene: float32[nit, 8, 4]"""
    pair, _ = U.scene(kind, NM, seed, NIT)
    p1, _ = U.ref_normalize(pair["keys1"])
    p2, _ = U.ref_normalize(pair["keys2"])
    first, second = U.match_list(pair["match12"])
    return np.concatenate([p1[first[pair["sets"]]], p2[second[pair["sets"]]]], 2)


# The header's Jacobi against numpy.linalg.svd in double on the 360 H-model DLT
# matrices (16 x 9) of the six scenes: the largest entry-wise difference of the
# null vector, up to sign, measured 6.13e-7 (sweeps 6 .. 8; 1.98e-6 over seeds
# 1 .. 6 of both kinds); the bound is 16 x the former.
NULL_H_MEASURED = 6.13e-7
# For the F model (8 x 9) the null vector is as ill-conditioned as sigma_8 is
# small: a perturbation of eps * sigma_1 turns it by eps * sigma_1 / sigma_8
# whatever the algorithm, and sets with sigma_8 / sigma_1 of 2e-4 occur.  The
# difference is therefore scaled by sigma_8 / sigma_1 (general scenes only: on a
# plane the matrix has rank 6 and no single null vector); measured 2.55e-7.
NULL_F_MEASURED = 2.55e-7


def test_null_vector_against_numpy_svd_in_double():
    worst_h = worst_f = 0.0
    sweeps = []
    for kind, seed in _all_scenes():
        for pn in _normalised_sets(kind, seed):
            A, h, sw = U.ref_dlt(pn, 0)
            vt = np.linalg.svd(A.astype(np.float64))[2][8]
            worst_h = max(worst_h, min(np.abs(vt - h).max(), np.abs(vt + h).max()))
            sweeps.append(sw)
            assert abs(np.linalg.norm(h.astype(np.float64)) - 1) < 1e-5
            if kind == "general":
                A, h, sw = U.ref_dlt(pn, 1)
                _, w, vt = np.linalg.svd(A.astype(np.float64))
                worst_f = max(worst_f, min(np.abs(vt[8] - h).max(), np.abs(vt[8] + h).max()) * w[7] / w[0])
                sweeps.append(sw)
    print("null vector: H %.3g, F scaled %.3g, sweeps %d .. %d" % (worst_h, worst_f, min(sweeps), max(sweeps)))
    assert worst_h <= 16 * NULL_H_MEASURED
    assert worst_f <= 16 * NULL_F_MEASURED
    assert max(sweeps) < U.IR_SWEEPS  # none of them ran to the cap (measured 5 .. 8)


# |det F21i| / ||F21i||_F^3 over the 360 hypotheses: measured 7.51e-11 (a matrix
# of full rank with equal singular values has 0.19); the bound is 16 x.
DET_MEASURED = 7.51e-11
# max |H21i H12i - I| / (||H21i||_F ||H12i||_F), in double: measured 1.22e-8 (the
# inverse is computed in double and rounded once, so this is float rounding of
# the nine entries); the bound is 16 x.
IDENT_MEASURED = 1.22e-8


def test_rank_two_f_and_inverse_h():
    worst_det = worst_id = 0.0
    for kind, seed in _all_scenes():
        hyp = U.scene_ref(kind, NM, seed, NIT)["hyp"].astype(np.float64)
        for row in hyp:
            H, Hi, F = row[:9].reshape(3, 3), row[9:18].reshape(3, 3), row[18:].reshape(3, 3)
            worst_det = max(worst_det, abs(np.linalg.det(F)) / np.linalg.norm(F) ** 3)
            worst_id = max(worst_id, np.abs(H @ Hi - np.eye(3)).max() / (np.linalg.norm(H) * np.linalg.norm(Hi)))
    print("rank-2 F: %.3g, H Hi - I: %.3g" % (worst_det, worst_id))
    assert worst_det <= 16 * DET_MEASURED
    assert worst_id <= 16 * IDENT_MEASURED


def test_normalize_is_the_sequential_float_form():
    """meanX and meanDevX as float sums in key order over all keys, 1.0 / meanDev
    divided in double; T maps a key to its normalised point"""
    pair, _ = U.scene("general", 50, 2, 3)
    keys = pair["keys1"]
    pts, T = U.ref_normalize(keys)
    f32 = np.float32
    mx = f32(0)
    for x in keys["x"]:
        mx = f32(mx + x)
    mx = f32(mx / f32(len(keys)))
    dev = f32(0)
    for x in keys["x"]:
        dev = f32(dev + abs(f32(x - mx)))
    dev = f32(dev / f32(len(keys)))
    sx = f32(1.0 / np.float64(dev))
    assert T[0, 0] == sx and T[0, 2] == f32(-mx * sx) and T[2, 2] == 1 and T[1, 0] == 0
    assert np.array_equal(pts[:, 0], (keys["x"] - mx).astype(f32) * sx)
    # an unmatched key moves the means: Normalize runs over the whole frame
    first, _ = U.match_list(pair["match12"])
    assert U.ref_normalize(keys[first])[1][0, 2] != T[0, 2]


def test_inverse_of_a_singular_matrix_is_zero():
    assert not U.ref_inv3([[1, 2, 3], [2, 4, 6], [0, 1, 5]]).any()
    assert not U.ref_inv3(np.zeros((3, 3))).any()
    R = U.ref_inv3([[2, 0, 1], [0, 4, -3], [0, 0, 1]])
    assert np.array_equal(R, np.array([[0.5, 0, -0.5], [0, 0.25, 0.75], [0, 0, 1]], np.float32))


# --------------------------------------------------------------------------- planted cases
CASES = U.planted_cases()


def _ref(name):
    pair, nit, sigma = CASES[name]
    return pair, U.ref_initialize(pair, nit, sigma)


def test_repeated_point_and_collinear_sets_are_scored_like_any_other():
    for name in ("repeated_point", "collinear"):
        pair, r = _ref(name)
        assert np.isfinite(r["it_scores"]).all() and np.isfinite(r["hyp"]).all(), name
        assert r["counters"]["h_capped"] == 0 and r["counters"]["f_capped"] == 0
        assert r["counters"]["skipped_floor"] > 0  # rank-deficient: a column vanished and was left alone
        assert r["it_H"] >= 0 and r["it_F"] >= 0


def test_singular_h_has_a_zero_inverse_and_a_nan_score_and_never_wins():
    pair, r = _ref("singular_h")
    assert not r["hyp"][0, 9:18].any() and r["hyp"][0, :9].any()
    assert np.isnan(r["it_scores"][0, 0])
    assert r["it_H"] == 1 and r["SH"] == r["it_scores"][1, 0] and np.isfinite(r["RH"])


def test_no_hypothesis_above_zero():
    pair, r = _ref("no_winner")
    assert (r["it_scores"] == 0).all()
    assert r["it_H"] == r["it_F"] == -1 and r["SH"] == 0 and r["SF"] == 0 and np.isnan(r["RH"])
    assert not r["inliers_H"].any() and not r["inliers_F"].any() and not r["H21"].any() and not r["F21"].any()


def test_of_equal_scores_the_first_wins():
    pair, r = _ref("equal_scores")
    s = r["it_scores"]
    assert s[2, 0] == s[4, 0] == s[:, 0].max() and r["it_H"] == 2
    assert s[1, 1] == s[3, 1] == s[:, 1].max() and r["it_F"] == 1
    assert r["counters"]["h_replaced"] >= 1  # iteration 1 won before iteration 2 replaced it


def test_chi_exactly_at_th_is_an_inlier_that_adds_nothing():
    pair, nit, s_at, s_above, i = U.chi_exact_case()
    at, above = U.ref_initialize(pair, nit, s_at), U.ref_initialize(pair, nit, s_above)
    assert at["inliers_H"][i] == 1 and above["inliers_H"][i] == 0
    first, second = U.match_list(pair["match12"])
    k1, k2 = pair["keys1"][first[i]], pair["keys2"][second[i]]
    sd1, _ = U.h_square_dists(at["hyp"][0, :9], at["hyp"][0, 9:18], k1["x"], k1["y"], k2["x"], k2["y"])
    assert np.float32(sd1 * U.inv_sigma2(s_at)) == U.TH_H < np.float32(sd1 * U.inv_sigma2(s_above))


def test_nit_zero_and_one():
    pair, r = _ref("nit0")
    assert r["it_H"] == r["it_F"] == -1 and np.isnan(r["RH"]) and r["nmatch"] == 40 and not r["inliers_F"].any()
    pair, r = _ref("nit1")
    assert r["it_H"] == r["it_F"] == 0 and r["SH"] == r["it_scores"][0, 0] and r["SF"] == r["it_scores"][0, 1]
    assert np.float32(r["SH"] / np.float32(r["SH"] + r["SF"])) == r["RH"]


def test_exactly_eight_matches():
    pair, r = _ref("eight_matches")
    assert r["nmatch"] == 8 and r["it_F"] >= 0
    # every set is a permutation of the same eight points: F fits them all
    assert r["inliers_F"].all()


def test_interleaved_unmatched_rows_and_unequal_frames():
    pair, r = _ref("interleaved")
    m = pair["match12"]
    assert len(pair["keys1"]) != len(pair["keys2"]) and (m < 0).sum() == 40 and (np.diff(np.nonzero(m >= 0)[0]) > 1).any()
    first, second = U.match_list(m)
    assert r["nmatch"] == 33 == len(first) and (np.diff(first) > 0).all()
    # the same matches as frames without the unmatched keys: another normalisation,
    # the same geometry, so the flags agree though the words do not
    bare = dict(keys1=pair["keys1"][first], keys2=pair["keys2"][second], match12=np.arange(33, dtype=np.int32),
                sets=pair["sets"])
    b = U.ref_initialize(bare, 7)
    assert not U.same_bits(b["hyp"], r["hyp"])
    assert np.array_equal(b["inliers_H"], r["inliers_H"]) and (b["it_H"], b["it_F"]) == (r["it_H"], r["it_F"])


def test_overflowing_keys_run_the_jacobi_to_its_cap():
    pair, r = _ref("capped")
    c = r["counters"]
    assert c["h_capped"] == c["f_capped"] == c["f3_capped"] == 2 and c["h_sweeps_max"] == U.IR_SWEEPS
    assert np.isnan(r["it_scores"]).all() and r["it_H"] == r["it_F"] == -1 and np.isnan(r["RH"])


def test_coverage_counters_over_the_scenes():
    tot = dict.fromkeys(U.COUNTERS, 0)
    for kind, seed in _all_scenes():
        for k, v in U.scene_ref(kind, NM, seed, NIT)["counters"].items():
            tot[k] = max(tot[k], v) if k.endswith("_max") else tot[k] + v
    n = 6 * NIT
    assert tot["h_converged"] == tot["f_converged"] == tot["f3_converged"] == n
    assert tot["h_capped"] == tot["f_capped"] == tot["f3_capped"] == 0
    assert tot["rotations"] > 0 and tot["skipped_orth"] > 0 and tot["skipped_floor"] > 0
    assert tot["h_replaced"] > 0 and tot["f_replaced"] > 0
    assert 5 * n <= tot["h_sweeps"] <= 9 * n and tot["h_sweeps_max"] <= 9  # measured 6.7 a run, at most 8


def test_the_draw_restated_from_rand():
    """draw_sets over glibc's rand() after srand(0): eight distinct indices per
    set, within the match list, and reproducible"""
    libc = ctypes.CDLL(None)
    libc.srand(0)
    a = U.draw_sets(50, 20, libc.rand)
    libc.srand(0)
    b = U.draw_sets(50, 20, libc.rand)
    assert np.array_equal(a, b) and a.min() >= 0 and a.max() < 50
    assert all(len(set(row)) == 8 for row in a.tolist())
    assert all(len(set(row)) == 8 for row in U.draw_sets(8, 5, libc.rand).tolist())


def test_out_of_range_indices_are_refused_by_the_restatement():
    pair, _ = U.scene("general", 20, 2, nit=4)
    bad = dict(pair, sets=np.full((4, 8), 20, np.int32))
    with pytest.raises(ValueError):
        U.ref_initialize(bad, 4)
