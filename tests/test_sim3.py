"""The CPU restatement of Sim3Solver (tests/cpp/sim3_ref.c over
csrc/sim3_math.h) on its own: that it solves the scenes, the
numerics of the forms OpenCV and libm would supply (measured against double
precision on the same float inputs; each bound below is 16 x the maximum
measured on the scenes of this file), the planted edge cases with the coverage
counters that show each branch ran, and the sequential loop against the closed
form the kernel selects by."""
import ctypes

import numpy as np
import pytest

import sim3_util as U

f32 = np.float32

# (ncorr, seed, s, fix_scale): 12 seeds (0..11) were tried per (s, fix_scale)
# row with 80 correspondences, 60 iterations and a quarter wrong; 12, 12 and 11
# qualified (the restatement hits and flags exactly the planted inliers); the
# first two qualifying seeds of each row are used
HIT_SCENES = ((80, 0, 1.0, True), (80, 1, 1.0, True), (80, 0, 0.7, False), (80, 1, 0.7, False),
              (80, 0, 1.4, False), (80, 1, 1.4, False))
# a scale that fix_scale cannot follow: no hypothesis gathers min_inliers
MISS_SCENES = ((80, 0, 0.7, True), (80, 3, 1.4, True))

# 16 x the maxima measured on HIT_SCENES + MISS_SCENES (printed by the tests;
# the measured values are in DESIGN §22)
QUAT_BOUND = 16 * 2.61e-6      # |q - q_eigh|, up to sign (432 of the 480 hypotheses: GAP_MIN)
R_BOUND = 16 * 5.42e-6         # |R12 - R(q_eigh)|, largest entry (the same 432)
ORTHO_BOUND = 16 * 7.49e-8     # |R R^T - I|, largest entry (all 480)
GAP_MIN = 0.05                 # relative gap of N's top two eigenvalues below which q is not compared
ATAN2_ULP_BOUND = 16 * 5.0     # ulps of double
SINCOS_ULP_BOUND = 16 * 1.0    # ulps of double; of 0.5 where the function is below 0.5


def _scene(ncorr, seed, s, fix):
    return U.scene(ncorr, seed, s=s, nit=60, fix_scale=fix)


def _ref(ncorr, seed, s, fix, **kw):
    return U.ref_solve(_scene(ncorr, seed, s, fix)[0], **kw)


@pytest.mark.parametrize("ncorr,seed,s,fix", HIT_SCENES)
def test_solver_hits_and_recovers_the_similarity(ncorr, seed, s, fix):
    pr, truth = _scene(ncorr, seed, s, fix)
    r = U.ref_solve(pr)
    assert r["it_hit"] >= 0 and r["it_best"] == r["it_hit"] and r["n_best"] > pr["min_inliers"]
    assert np.array_equal(r["inliers"], truth["planted"])  # a property of these seeds (see HIT_SCENES)
    assert r["n_best"] == int(truth["planted"].sum()) == int(r["inliers"].sum())
    # noise of 2 mm on points 3-15 m away, three of them per hypothesis
    assert abs(float(r["s12"]) - s) < 5e-3 * s
    assert np.abs(r["R12"] - truth["R"]).max() < 5e-3
    assert np.abs(r["t12"] - truth["t"]).max() < 5e-2
    if fix:
        assert r["s12"] == f32(1.0)
    # mT21i is the inverse of mT12i
    sR12 = np.float64(r["s12"]) * r["R12"].astype(np.float64)
    assert np.abs(r["sR21"].astype(np.float64) @ sR12 - np.eye(3)).max() < 1e-5
    assert np.abs(r["sR21"].astype(np.float64) @ r["t12"] + r["t21"]).max() < 1e-5


@pytest.mark.parametrize("ncorr,seed,s,fix", MISS_SCENES)
def test_fixed_scale_misses_a_scaled_scene(ncorr, seed, s, fix):
    r = _ref(ncorr, seed, s, fix)
    assert r["it_hit"] == -1 and r["it_best"] >= 0 and r["n_best"] <= 20
    assert r["counters"]["evaluated"] == 60 and r["counters"]["hits"] == 0


# --------------------------------------------------------------------------- numerics
def _horn_double(c, tri):
    """N and its top eigenvector in double from the float camera coordinates"""
    X1, X2 = c[list(tri), 0:3].astype(np.float64), c[list(tri), 3:6].astype(np.float64)
    P1, P2 = (X1 - X1.mean(0)).T, (X2 - X2.mean(0)).T
    M = P2 @ P1.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
    N = N + np.triu(N, 1).T
    w, V = np.linalg.eigh(N)
    return V[:, -1], (w[-1] - w[-2]) / max(abs(w[-1]), 1e-300)


def _rot_of_quat(q):
    ang = np.arctan2(np.linalg.norm(q[1:]), q[0])
    return U.rot(q[1:], 2 * ang)


def test_quaternion_and_rotation_against_double():
    dq = dr = do = 0.0
    sweeps_max = runs = total = 0
    for sc in HIT_SCENES + MISS_SCENES:
        pr, _ = _scene(*sc)
        r = U.ref_solve(pr, eval_all=True)
        assert r["counters"]["capped"] == 0  # every Jacobi run converged
        sweeps_max = max(sweeps_max, r["counters"]["sweeps_max"])
        for it, tri in enumerate(pr["triples"]):
            q64, gap = _horn_double(r["corr"], tri)
            q = r["quat"][it].astype(np.float64)
            R = r["hyp"][it, :9].reshape(3, 3).astype(np.float64)
            do = max(do, np.abs(R @ R.T - np.eye(3)).max())
            total += 1
            if gap < GAP_MIN:  # a triple with a wrong point can leave the top two eigenvalues close: no
                continue       # eigenvector to compare with
            dq = max(dq, min(np.abs(q - q64).max(), np.abs(q + q64).max()))
            dr = max(dr, np.abs(R - _rot_of_quat(q64)).max())
            runs += 1
    assert runs > total // 2
    print("sim3 numerics: %d of %d runs, |dq| %.3g, |dR| %.3g, |RRt - I| %.3g, sweeps max %d" % (runs, total, dq, dr, do, sweeps_max))
    assert dq <= QUAT_BOUND and dr <= R_BOUND and do <= ORTHO_BOUND
    assert sweeps_max < U.S3_SWEEPS


def _ulps(got, want):
    return np.abs(got - want) / np.spacing(np.abs(want))


def test_atan2_sin_cos_against_numpy():
    lib = U.ref_lib()
    # the reachable arguments: a unit quaternion's (|imaginary part|, real part),
    # to float rounding; the angle over the whole half circle, densely near both ends
    ang = np.concatenate([np.linspace(0, np.pi, 4001), np.geomspace(1e-12, 1e-2, 500), np.pi - np.geomspace(1e-12, 1e-2, 500)])
    worst = 0.0
    for a in ang:
        for scale in (1.0, 0.999999, 1.000001):
            y, x = float(np.sin(a) * scale), f32(np.cos(a) * scale)
            got = lib.s3_ref_atan2(y, x)
            want = np.arctan2(y, np.float64(x))
            if want != 0:
                worst = max(worst, float(_ulps(got, want)))
            else:
                assert got == 0
    print("sim3 numerics: atan2 worst %.3g ulp" % worst)
    assert worst <= ATAN2_ULP_BOUND
    # the IEEE special cases for y >= 0
    assert lib.s3_ref_atan2(0.0, f32(0.0)) == 0.0 and lib.s3_ref_atan2(0.0, f32(-0.0)) == np.pi
    assert lib.s3_ref_atan2(0.0, f32(2.0)) == 0.0 and lib.s3_ref_atan2(0.0, f32(-2.0)) == np.pi
    assert lib.s3_ref_atan2(3.0, f32(0.0)) == np.pi / 2 and lib.s3_ref_atan2(3.0, f32(-0.0)) == np.pi / 2
    assert np.isnan(lib.s3_ref_atan2(np.nan, f32(1.0))) and np.isnan(lib.s3_ref_atan2(1.0, f32(np.nan)))
    # sin and cos over Rodrigues' range: theta = 2 ang in [0, 2 pi]
    s, c = ctypes.c_double(), ctypes.c_double()
    ws = wc = 0.0
    for th in np.concatenate([np.linspace(0, 2 * np.pi + 1e-3, 8001), np.geomspace(1e-15, 1e-2, 400)]):
        lib.s3_ref_sincos(float(th), ctypes.byref(s), ctypes.byref(c))
        # near a zero of the function the error is the reduction's: measure against the larger of the two
        ws = max(ws, abs(s.value - np.sin(th)) / np.spacing(max(abs(np.sin(th)), 0.5)) if abs(np.sin(th)) < 0.5
                 else float(_ulps(s.value, np.sin(th))))
        wc = max(wc, abs(c.value - np.cos(th)) / np.spacing(max(abs(np.cos(th)), 0.5)) if abs(np.cos(th)) < 0.5
                 else float(_ulps(c.value, np.cos(th))))
    print("sim3 numerics: sin worst %.3g ulp, cos worst %.3g ulp" % (ws, wc))
    assert ws <= SINCOS_ULP_BOUND and wc <= SINCOS_ULP_BOUND


def test_bound_is_truncated_to_an_integer():
    lib = U.ref_lib()
    assert lib.s3_ref_max_error(f32(1.2)) == 11.0  # not 11.052
    assert lib.s3_ref_max_error(f32(0.1)) == 0.0
    assert lib.s3_ref_max_error(f32(1.0)) == 9.0 and lib.s3_ref_max_error(f32(1.44)) == 13.0
    assert lib.s3_ref_sigma2_ok(f32(0.0)) and lib.s3_ref_sigma2_ok(f32(2.3e8))
    for bad in (np.nan, np.inf, -1e-30, 2.4e8):
        assert not lib.s3_ref_sigma2_ok(f32(bad))


# --------------------------------------------------------------------------- planted cases
def _case(name, **kw):
    pr = U.planted_cases()[name]
    return pr, U.ref_solve(pr, **kw)


def test_planted_zero_bound():
    pr, r = _case("sigma_zero")
    nit = len(pr["triples"])
    assert r["counters"]["zero_bound"] == 40 and not r["inliers"].any()
    assert (r["counts"] == 0).all() and r["it_hit"] == -1 and r["it_best"] == nit - 1 and r["n_best"] == 0
    assert r["counters"]["pass_zero"] == nit == r["counters"]["replaced"]
    assert np.isfinite(r["R12"]).all()  # the last hypothesis is an ordinary one


def test_planted_truncation():
    pr, i, e2 = U.truncation_case()
    r = U.ref_solve(pr)
    assert 11.0 <= e2 < 9.210 * float(f32(1.2))
    assert r["inliers"][i] == 0 and r["inliers"].sum() == 23 and r["it_hit"] == 0
    # under the untruncated bound it would be an inlier: its other error is far below its own bound
    e1, _ = U.ref_errors(U.ref_solve(pr, eval_all=True)["hyp"][0], np.concatenate([pr["K1"], pr["K2"]]), r["corr"][i])
    assert e1 < 921.0


def test_planted_degenerate_triples():
    pr, r = _case("degenerate_triples", eval_all=True)
    assert r["it_hit"] == 3 and (r["counts"][:3] <= pr["min_inliers"]).all()
    c = r["corr"]
    for k in (0, 3):  # collinear in both camera frames, to rounding
        d1, d2 = c[1, k:k + 3] - c[0, k:k + 3], c[2, k:k + 3] - c[0, k:k + 3]
        assert np.linalg.norm(np.cross(d1, d2)) < 1e-5 * np.linalg.norm(d1) * np.linalg.norm(d2)


def test_planted_coincident_points():
    pr, r = _case("coincident_only")
    assert r["counters"]["nan_hyp"] == 1 and r["counts"][0] == 0 and r["counters"]["pass_zero"] == 1
    assert r["it_best"] == 0 and r["it_hit"] == -1 and np.isnan(r["R12"]).all() and np.isnan(r["s12"])
    assert not r["inliers"].any()
    pr, r = _case("coincident")  # followed by an ordinary hypothesis that also counts 0: the later tie replaces
    assert r["counters"]["nan_hyp"] == 1 and r["it_best"] == 1 and np.isfinite(r["R12"]).all()


def test_planted_depth_zero_and_behind():
    pr, r = _case("depth_zero_and_behind")
    assert r["counters"]["z_zero"] == 1 and r["counters"]["z_neg"] == 1
    assert r["corr"][6, 2] == 0 and r["corr"][8, 2] == -4
    assert not np.isfinite(r["corr"][6, 6:8]).all()  # 1 / 0: projected as it is
    assert r["inliers"][6] == 0 and r["inliers"][8] == 0 and r["it_hit"] == 0


def test_planted_loop_cases():
    pr, r = _case("equal_counts_no_hit", eval_all=True)
    assert list(r["counts"][[1, 3]]) == [pr["min_inliers"]] * 2 and r["it_hit"] == -1 and r["it_best"] == 3
    pr, r = _case("equal_counts_hit", eval_all=True)
    assert r["counts"][1] == r["counts"][2] > pr["min_inliers"] and r["it_hit"] == r["it_best"] == 1
    assert r["counters"]["evaluated"] == 2
    for name, hit, nit in (("hit_first", 0, 3), ("hit_last", 3, 4), ("no_hit", -1, 3)):
        pr, r = _case(name)
        assert r["it_hit"] == hit and len(pr["triples"]) == nit
        assert r["counters"]["evaluated"] == (hit + 1 if hit >= 0 else nit)
    pr, r = _case("best_in_above")
    assert r["it_best"] == -1 and r["it_hit"] == -1 and r["n_best"] == 41 and r["counters"]["replaced"] == 0
    assert not r["inliers"].any() and not r["R12"].any()
    pr, r = _case("best_in_between", eval_all=True)
    assert r["counts"][0] < pr["best_in"] <= r["counts"][2] and r["it_best"] == 2 and r["counters"]["replaced"] == 1


def test_planted_sizes():
    pr, r = _case("inert")
    assert r["counters"]["inert"] == 1 and r["it_hit"] == r["it_best"] == -1 and r["counters"]["evaluated"] == 0
    pr, r = _case("three_correspondences")
    assert r["ncorr"] == 3 and r["it_hit"] == 0 and r["n_best"] == 3 and r["inliers"].all()
    pr, r = _case("ncorr_equals_min_inliers")
    assert r["counters"]["inert"] == 0 and r["it_hit"] == -1 and r["counters"]["evaluated"] == 12  # > is never met
    pr, r = _case("nit0")
    assert r["it_hit"] == r["it_best"] == -1 and r["n_best"] == 0 and not r["inliers"].any()
    pr, r = _case("nit1")
    assert r["it_hit"] == r["it_best"] == 0
    pr, r = _case("fix_scale")
    assert r["s12"] == f32(1.0) and r["it_hit"] >= 0
    assert U.same_bits(r["sR21"], r["R12"].T)  # 1.0 / 1 = 1: sRinv is R^T itself


# --------------------------------------------------------------------------- the loop against the formula
def test_sequential_loop_equals_the_closed_form():
    rng = np.random.default_rng(12)
    hit = miss = none = 0
    for _ in range(3000):
        nit = int(rng.integers(0, 40))
        top = int(rng.integers(1, 12))
        counts = rng.integers(0, top + 1, nit)  # few distinct values: ties everywhere
        best_in = int(rng.integers(0, top + 2)) if rng.random() < 0.5 else 0
        min_inliers = int(rng.integers(0, top + 2))
        got = U.ref_loop(counts, best_in, min_inliers)
        assert got == U.closed_form(counts, best_in, min_inliers), (counts, best_in, min_inliers)
        hit += got[0] >= 0
        miss += got[0] < 0 <= got[1]
        none += got[1] < 0
    assert min(hit, miss, none) > 100
