"""The CPU restatement of Optimizer::PoseOptimization (tests/cpp/poseopt_ref.c,
DESIGN.md §19) against ground truth, planted outliers, its own sequential
order and hand-derived semantics.  No GPU: the device is compared with this
restatement bit for bit in test_poseopt_gpu.py."""
import numpy as np
import pytest

import poseopt_util as U

KINDS = ("mono", "stereo", "mixed")
GT_SCENES = [(n, s, k) for n in (30, 200, 1000) for s in (1, 2, 3, 4) for k in KINDS]
OUT_SCENES = [(n, s, k) for n in (64, 300, 1025) for s in (1, 2, 3, 4) for k in KINDS]

# Largest error of the returned pose over GT_SCENES, measured with this
# restatement (DEVICE order): 1.43e-8 rad and 2.70e-7 m.  What is left is the
# float rounding of the observations and of the output pose, which varies with
# the conditioning of the scene: the bound is 4 x the measured value.
GT_ROT_MEASURED, GT_TRANS_MEASURED = 1.4283862101524654e-08, 2.698313652072207e-07
GT_ROT_BOUND, GT_TRANS_BOUND = 4 * GT_ROT_MEASURED, 4 * GT_TRANS_MEASURED
# Largest |difference| of the final estimate in double (quaternion and
# translation entries) between SEQUENTIAL and DEVICE order over OUT_SCENES:
# 8.25e-10.  Rounding noise amplified by the conditioning of H: 16 x.
ORDER_MEASURED = 8.247494909241482e-10
ORDER_BOUND = 16 * ORDER_MEASURED


def nonzero(c):
    return {k: v for k, v in c.items() if v}


@pytest.mark.parametrize("n,seed,kind", GT_SCENES)
def test_ground_truth(n, seed, kind):
    _, _, truth = U.scene(n, seed, stereo=kind)
    r = U.scene_ref(n, seed, stereo=kind)
    assert r["ninliers"] == n and not r["outlier"].any()
    rot, trans = U.pose_error(r["Tcw"], truth["Tcw"])
    print("rot %.3e rad, trans %.3e m" % (rot, trans))
    assert rot <= GT_ROT_BOUND and trans <= GT_TRANS_BOUND, (rot, trans)


def test_ground_truth_bound_is_the_measured_one():
    errs = [U.pose_error(U.scene_ref(n, s, stereo=k)["Tcw"], U.scene(n, s, stereo=k)[2]["Tcw"]) for n, s, k in GT_SCENES]
    print("max rot %.17g max trans %.17g" % (max(e[0] for e in errs), max(e[1] for e in errs)))
    assert max(e[0] for e in errs) == GT_ROT_MEASURED and max(e[1] for e in errs) == GT_TRANS_MEASURED


@pytest.mark.parametrize("n,seed,kind", OUT_SCENES)
def test_planted_outliers(n, seed, kind):
    kw = dict(stereo=kind, **U.OUTLIER_SCENE)
    _, _, truth = U.scene(n, seed, **kw)
    r = U.scene_ref(n, seed, **kw)
    assert np.array_equal(r["outlier"], truth["planted"])
    assert r["ninliers"] == n - int(truth["planted"].sum())


@pytest.mark.parametrize("n,seed,kind", OUT_SCENES)
def test_sequential_and_device_order(n, seed, kind):
    kw = dict(stereo=kind, **U.OUTLIER_SCENE)
    d = U.scene_ref(n, seed, U.DEVICE, **kw)
    s = U.scene_ref(n, seed, U.SEQUENTIAL, **kw)
    assert np.array_equal(d["outlier"], s["outlier"]) and d["ninliers"] == s["ninliers"]
    diff = float(np.abs(d["pose7"] - s["pose7"]).max())
    print("pose difference %.3e" % diff)
    assert diff <= ORDER_BOUND, diff


def test_order_bound_is_the_measured_one():
    diffs = []
    for n, s, k in OUT_SCENES:
        kw = dict(stereo=k, **U.OUTLIER_SCENE)
        diffs.append(float(np.abs(U.scene_ref(n, s, U.DEVICE, **kw)["pose7"] -
                                  U.scene_ref(n, s, U.SEQUENTIAL, **kw)["pose7"]).max()))
    print("max difference %.17g" % max(diffs))
    assert max(diffs) == ORDER_MEASURED


@pytest.mark.parametrize("form", ("mask", "index"))
def test_point_forms_equal_the_plain_problem(form):
    """has_point and point_index select the same edges as a frame holding only
    those features would: the inliers, the flags of the features with a point
    and the pose follow the planted truth"""
    kw = dict(form=form, **U.OUTLIER_SCENE)
    _, obs, truth = U.scene(300, 6, **kw)
    r = U.scene_ref(300, 6, **kw)
    has = truth["has"] != 0
    assert np.array_equal(r["outlier"][has], truth["planted"][has]) and not r["outlier"][~has].any()
    assert r["ninliers"] == int(has.sum()) - int(truth["planted"][has].sum())
    assert r["counters"]["invalid"] == 0


# --------------------------------------------------------------------------- semantics
@pytest.mark.parametrize("n", (0, 2))
def test_fewer_than_three_correspondences(n):
    """Optimizer.cc:345-346: return 0, the pose is not written, the flags of
    the features with points are already cleared"""
    cam, obs, _ = U.scene(n, 3, **U.OUTLIER_SCENE)
    r = U.ref_optimize(cam, obs)
    assert r["ninliers"] == 0 and not r["outlier"].any() and r["counters"]["rounds"] == 0
    assert np.array_equal(r["Tcw"][:3], cam["Tcw"]) and np.array_equal(r["Tcw"][3], [0, 0, 0, 1])


def test_three_of_many_features_have_points():
    """the count is of correspondences, not of features: 2 of 40 return 0"""
    cam, obs, _ = U.scene(40, 3)
    has = np.zeros(40, np.uint8)
    has[[5, 17]] = 1
    r = U.ref_optimize(cam, dict(obs, has_point=has))
    assert r["ninliers"] == 0 and r["counters"]["rounds"] == 0
    has[30] = 1
    r = U.ref_optimize(cam, dict(obs, has_point=has))
    assert r["ninliers"] == 3 and r["counters"]["rounds"] == 1


def test_nine_correspondences_run_one_round():
    """Optimizer.cc:421-422: fewer than 10 edges break after the first round"""
    cam, obs, truth = U.scene(9, 5)
    r = U.ref_optimize(cam, obs)
    assert r["counters"]["rounds"] == 1 and r["ninliers"] == 9
    ends = sum(r["counters"][k] for k in ("end_iters", "end_qmax", "end_rho0", "end_small"))
    assert ends == 1  # one optimize() call
    assert U.scene_ref(10, 5)["counters"]["rounds"] == 4


def test_readmitted_feature():
    """a feature flagged after one round is classified again at the end of
    every later one (Optimizer.cc:369-372) and can come back"""
    kw = dict(noise=2.0, outliers=0.3, perturb=(0.08, 0.3))
    r = U.scene_ref(20, 4, **kw)
    assert r["counters"]["readmitted"] >= 1, nonzero(r["counters"])
    assert r["counters"]["rounds"] == 4


def _grid_points():
    """12 points spread over the view at depths 3 .. 14, seen exactly"""
    pts = [(0.3 * ((5 * i) % 7 - 3), 0.2 * ((3 * i) % 5 - 2), 3.0 + i) for i in range(12)]
    uv = [(512 * p[0] / p[2], 512 * p[1] / p[2]) for p in pts]
    return pts, uv


@pytest.mark.parametrize("point", ((0.25, 0.0, 0.0), (0.0, 0.0, 0.0)))
def test_point_at_zero_depth(point):
    """z == 0: the edge's error is infinite or NaN, information * error is NaN
    (0 * inf), so H, the step and every trial pose are NaN.  Each trial is
    rejected (rho is NaN: neither > 0 nor < 0, so one trial per iteration and no
    Terminate), all 10 iterations run, the estimate stays the input pose, and
    every chi2, left at the NaN trial pose, classifies as inlier (NaN > x is
    false)"""
    pts, uv = _grid_points()
    pts[4] = point
    cam, obs = U.axis_scene(pts, uv)
    r = U.ref_optimize(cam, obs)
    assert r["ninliers"] == 12 and not r["outlier"].any()
    assert np.array_equal(r["Tcw"], np.eye(4, dtype=np.float32))
    c = r["counters"]
    assert (c["rounds"], c["end_iters"], c["rejected"], c["accepted"]) == (4, 4, 40, 0), nonzero(c)


def test_point_behind_the_camera():
    """z < 0: g2o makes no depth test, the mirrored projection is an ordinary
    edge: consistent with the pose it is an inlier, else an outlier"""
    pts, uv = _grid_points()
    pts[4] = (0.2, 0.1, -2.0)
    uv[4] = (512 * 0.2 / -2.0, 512 * 0.1 / -2.0)
    cam, obs = U.axis_scene(pts, uv)
    r = U.ref_optimize(cam, obs)
    assert r["ninliers"] == 12 and not r["outlier"].any()
    rot, trans = U.pose_error(r["Tcw"], np.eye(4))
    assert rot < 1e-6 and trans < 1e-5, (rot, trans)
    uv[4] = (uv[4][0] + 40.0, uv[4][1])
    r = U.ref_optimize(*U.axis_scene(pts, uv))
    assert r["ninliers"] == 11 and r["outlier"].tolist() == [0, 0, 0, 0, 1] + [0] * 7


def test_mono_stereo_switch_is_uright_below_zero():
    """Optimizer.cc:267: mvuRight[i] < 0 is monocular; 0 itself is stereo.  A
    point whose right coordinate is planted 40 px off is an outlier only where
    the edge is stereo"""
    pts, uv = _grid_points()
    ur = [u - 32.0 / p[2] for (u, _), p in zip(uv, pts)]
    ur[3] = 0.0  # stereo, and far from u - bf / z = -1.53..
    ur[7] = -1.0  # mono: the right coordinate is not read
    r = U.ref_optimize(*U.axis_scene(pts, uv, uright=ur))
    assert r["outlier"].tolist() == [0, 0, 0, 1] + [0] * 8 and r["ninliers"] == 11


def test_bad_octave_and_index_are_dropped_and_counted():
    """the plan form's rule: such a feature has no point and is counted"""
    cam, obs, truth = U.scene(300, 6, form="index", **U.OUTLIER_SCENE)
    base = U.scene_ref(300, 6, form="index", **U.OUTLIER_SCENE)
    idx = obs["point_index"].copy()
    keys = obs["keys"].copy()
    live = np.flatnonzero(idx >= 0)
    idx[live[0]] = len(obs["pos"])
    idx[live[1]] = -2
    keys["octave"][live[2]] = 8
    keys["octave"][live[3]] = -1
    r = U.ref_optimize(cam, dict(obs, point_index=idx, keys=keys))
    assert r["counters"]["invalid"] == 4 and not r["outlier"][live[:4]].any()
    rest = np.ones(300, bool)
    rest[live[:4]] = False
    assert np.array_equal(r["outlier"][rest], base["outlier"][rest])


# --------------------------------------------------------------------------- branch coverage
def coverage_cases():
    """(name, camera, obs) of every case the GPU file runs through the ABI too"""
    cases = []
    for n in U.SIZES:
        cam, obs, _ = U.sweep_scene(n)
        cases.append(("sweep%d" % n, cam, obs))
    pts, uv = _grid_points()
    for name, p in (("z0", (0.25, 0.0, 0.0)), ("z0origin", (0.0, 0.0, 0.0))):
        q = list(pts)
        q[4] = p
        cases.append((name,) + U.axis_scene(q, uv))
    q, w = list(pts), list(uv)
    q[4] = (0.2, 0.1, -2.0)
    w[4] = (512 * 0.2 / -2.0 + 40.0, 512 * 0.1 / -2.0)
    cases.append(("zneg",) + U.axis_scene(q, w))
    cam, obs, _ = U.scene(20, 4, noise=2.0, outliers=0.3, perturb=(0.08, 0.3))
    cases.append(("readmit", cam, obs))
    for kind in KINDS:
        cam, obs, _ = U.scene(200, 2, stereo=kind, **U.OUTLIER_SCENE)
        cases.append((kind, cam, obs))
    # every point on the optical axis, observed there: b = 0, the step is 0 and rho == 0
    axis = [(0, 0, 2.0 + i) for i in range(12)]
    cases.append(("axis",) + U.axis_scene(axis, [(0, 0)] * 12))
    # fewer than 3 distinct points: H is singular, lambda alone makes it solvable
    two = [(0.1, 0.2, 4.0) if i % 2 else (-0.3, 0.1, 6.0) for i in range(12)]
    cases.append(("two",) + U.axis_scene(two, [(512 * p[0] / p[2] + 0.3, 512 * p[1] / p[2] - 0.2) for p in two]))
    # a negative information weight makes H negative definite: the solver fails
    cam, obs, _ = U.scene(30, 1)
    cases.append(("negweight", dict(cam, inv_level_sigma2=-cam["inv_level_sigma2"]), obs))
    # no level-0 edge is left after round 0: optimize() has nothing to do
    cam, obs, _ = U.scene(12, 1, noise=0.0, outliers=1.0)
    cases.append(("alloutliers", cam, obs))
    return cases


def test_branch_coverage():
    """Over the case set every exit of the Levenberg loop and both step kinds
    occur.  The solver-failure exit is reached only with a negative information
    weight: with weights >= 0, H + lambda I is positive semi-definite up to
    rounding, a NaN pivot is not negative, and no degenerate geometry tried
    (all points on the optical axis, one or two distinct points) produced a
    negative pivot."""
    total = {k: 0 for k in U.COUNTERS}
    by_case = {}
    for name, cam, obs in coverage_cases():
        c = U.ref_optimize(cam, obs)["counters"]
        by_case[name] = nonzero(c)
        for k, v in c.items():
            total[k] += v
    print(by_case)
    for k in ("accepted", "rejected", "end_small", "end_iters", "end_qmax", "end_rho0", "solver_fail", "readmitted"):
        assert total[k] >= 1, (k, by_case)
    assert by_case["negweight"].get("solver_fail", 0) >= 1
    assert by_case["axis"].get("end_rho0", 0) >= 1
    assert by_case["alloutliers"].get("no_active", 0) >= 1
    for name in ("axis", "two"):
        assert "solver_fail" not in by_case[name]
