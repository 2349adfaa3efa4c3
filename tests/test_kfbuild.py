"""Keyframe projection, the parts that need no GPU: the
argument checks of the C ABI that return before a device is looked at, and --
on the CPU restatement alone -- that the random scenes of the GPU tests reach
every branch and can tell the fused u, v from the unfused ones, and that the
planted edge cases come out as worked out by hand."""
import ctypes

import numpy as np
import pytest

import kfbuild_util as U
from kfbuild_util import B, f32

SEEDS = {U.FUSE: 200, U.SIM3: 201}


def _call(orbx_mod, form, cam, P, npts, th=3.0, nprob=1, q=True, level=True, nlive=True, cams=True, pts=True,
          counts=True, base=None):
    """orbm_keyframe_project with chosen arguments withheld; every refusal
    here comes before the device is looked at"""
    c = (orbx_mod.KfCamera * 1)(orbx_mod.kf_camera(cam))
    keep = {n: np.ascontiguousarray(P[n]) for n in U.POINT_FIELDS if P.get(n) is not None}
    pp = (orbx_mod.KfPoints * 1)(orbx_mod.KfPoints(*[None if n not in keep else keep[n].ctypes.data
                                                      for n in U.POINT_FIELDS]))
    n = np.array([npts], np.int32)
    qa = np.zeros(max(npts, 1), orbx_mod.KF_QUERY_DTYPE)
    la, na = np.zeros(max(npts, 1), np.int32), np.full(1, -7, np.int32)
    ba = None if base is None else np.array([base], np.int32)
    vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
    rc = orbx_mod.lib().orbm_keyframe_project(
        form, nprob, ctypes.cast(c, ctypes.c_void_p) if cams else None,
        ctypes.cast(pp, ctypes.c_void_p) if pts else None, vp(n) if counts else None, vp(ba), th, 0,
        vp(qa) if q else None, vp(la) if level else None, vp(na) if nlive else None)
    return rc, int(na[0])


def test_keyframe_project_argument_errors(orbx_mod):
    cam = U.planted_camera()
    P = U.make_points(4)
    E, OK = orbx_mod.ERR_ARG, orbx_mod.OK
    assert _call(orbx_mod, U.FUSE, cam, P, 4, nprob=0)[0] == OK  # nothing to do, nothing read
    assert _call(orbx_mod, U.SIM3, cam, P, 0) == (OK, 0)         # an empty problem needs no device
    assert _call(orbx_mod, U.FUSE, cam, P, 0, q=False, level=False) == (OK, 0)
    for form in (0, 3, -1):
        assert _call(orbx_mod, form, cam, P, 4)[0] == E
    assert _call(orbx_mod, U.FUSE, cam, P, 4, nprob=-1)[0] == E
    assert _call(orbx_mod, U.FUSE, cam, P, 4, nprob=70000)[0] == E
    assert _call(orbx_mod, U.FUSE, cam, P, -1)[0] == E
    for what in ("q", "level", "nlive", "cams", "pts", "counts"):
        assert _call(orbx_mod, U.FUSE, cam, P, 4, **{what: False})[0] == E, what
    for form in U.FORMS:
        for name in ("pos", "min_dist_inv", "max_dist_inv", "max_dist"):
            assert _call(orbx_mod, form, cam, dict(P, **{name: None}), 4)[0] == E, (form, name)
    assert _call(orbx_mod, U.FUSE, cam, P, 4, base=-1)[0] == E
    assert _call(orbx_mod, U.FUSE, cam, P, 4, base=2 ** 31 - 2)[0] == E  # base + npts past int32
    for lsf in (0.0, float("nan"), -1.0, 1e-8):
        assert _call(orbx_mod, U.FUSE, dict(cam, log_scale_factor=f32(lsf)), P, 4)[0] == E, lsf
    bad = orbx_mod.kf_camera(cam)
    for nl in (33, 0, -1):
        bad.nlevels = nl
        assert _call(orbx_mod, U.SIM3, bad, P, 4)[0] == E


def test_plan_argument_errors_before_the_device(orbx_mod):
    lib = orbx_mod.lib()
    E = orbx_mod.ERR_ARG
    h = ctypes.c_void_p()
    before, counts = np.zeros(4, np.int32), np.zeros(4, np.int32)
    assert lib.orbx_debug_live_resources(before.ctypes.data_as(ctypes.c_void_p)) == orbx_mod.OK
    assert lib.orbm_kf_plan_create(1, 100, 10, 0, None) == E
    for args in ((0, 100, 10), (1, 0, 10), (1, 100, -1)):
        assert lib.orbm_kf_plan_create(*args, 0, ctypes.byref(h)) == E and not h.value, args
    assert lib.orbm_kf_plan_create(1, orbx_mod.KFW_MAXN + 1, 10, 0, ctypes.byref(h)) == orbx_mod.ERR_UNSUPPORTED
    assert lib.orbm_kf_plan_create(65536, 100, 10, 0, ctypes.byref(h)) == orbx_mod.ERR_UNSUPPORTED
    assert lib.orbm_kf_plan_destroy(None) == orbx_mod.OK
    pb = (orbx_mod.KfProblem * 1)()
    assert lib.orbm_kf_plan_search(None, 1, ctypes.cast(pb, ctypes.c_void_p), None) == E
    assert lib.orbm_kf_plan_project(None, U.FUSE, 1, ctypes.cast(pb, ctypes.c_void_p), 3.0, None) == E
    assert lib.orbm_kf_plan_project_search(None, U.SIM3, 1, ctypes.cast(pb, ctypes.c_void_p), 3.0, None) == E
    assert lib.orbx_debug_live_resources(counts.ctypes.data_as(ctypes.c_void_p)) == orbx_mod.OK
    assert np.array_equal(counts, before)  # the refused creates left nothing behind


# --------------------------------------------------------------------------- non-vacuity, restatement alone
@pytest.mark.parametrize("form", U.FORMS)
def test_random_scenes_reach_every_branch(form):
    n, seed = 3000, SEEDS[form]
    differ = U.assert_not_vacuous(form, n, seed)
    assert differ >= 10
    r = U.scene_ref(form, n, seed)
    live = r["branch"] == B["live"]
    hist = np.bincount(r["branch"], minlength=len(U.BRANCHES))
    for name in U.REJECTIONS:  # skip, depth, the four bounds, below and above the range
        assert hist[B[name]] >= 1, (name, hist)
    q = r["q"]
    assert (q["desc"] == np.arange(n)).all()
    assert (q["radius"][~live] == -1).all() and (q["level"][~live] == -1).all()
    assert (q["x"][~live] == 0).all() and (q["y"][~live] == 0).all() and (r["level"] == q["level"]).all()
    sf = U.random_scene(form, n, seed)[0]["scale_factors"]
    assert (q["radius"][live] == f32(U.TH[form]) * sf[q["level"][live]]).all()


def test_restatement_predict_scale_is_the_library_table(orbx_mod):
    """thr[L] found by bisection over the restatement's own PredictScale is the
    table the kernels count over"""
    cam = U.planted_camera()
    thr = U.host_thresholds(cam["log_scale_factor"], 8)
    lib = orbx_mod.predict_scale_thresholds(cam["log_scale_factor"], 8)
    assert np.array_equal(thr.view(np.uint32), lib.view(np.uint32))


# --------------------------------------------------------------------------- planted edges, restatement alone
@pytest.mark.parametrize("form", U.FORMS)
@pytest.mark.parametrize("th", (3.0, 7.5))
def test_planted_edges_on_the_restatement(form, th):
    cam = U.planted_camera()
    thr = U.host_thresholds(cam["log_scale_factor"], 8)
    edges = U.planted_edges(thr)
    P, slots = U.planted_points(edges)
    assert {0, 63, 64, 255, 256} <= set(slots) and len(P["pos"]) > 256
    r = U.ref_project(form, cam, P, th)
    U.check_planted(edges, slots, r, th, cam)
    by = {e.name: s for e, s in zip(edges, slots)}
    q = r["q"]
    assert q["x"][by["u=min"]] == cam["min_x"] and q["y"][by["v=min"]] == cam["min_y"]
    assert q["x"][by["u<max"]] == U.down(cam["max_x"]) and q["y"][by["v<max"]] == U.down(cam["max_y"])
    # the two zero depths differ in sign: were Z=-0's depth +0, x = -0.25 / +0 = -inf would fail u >= min_x instead
    assert r["branch"][by["Z=+0"]] == r["branch"][by["Z=-0"]] == B["u_high"]
    flipped = dict(P, pos=P["pos"].copy())
    flipped["pos"][by["Z=-0"]] = (-0.25, 0.0, 0.0)
    assert U.ref_project(form, cam, flipped, th)["branch"][by["Z=-0"]] == B["u_low"]
    assert r["branch"][by["Z=-denorm"]] == B["depth"] and -1e-44 < P["pos"][by["Z=-denorm"]][2] < 0
    filler = [i for i in range(len(P["pos"])) if i not in slots]
    assert (r["branch"][filler] == B["live"]).all()
    assert (q["x"][filler] == f32(51.2)).all() and (q["y"][filler] == f32(25.6)).all()
    assert r["n_live"] == int((r["branch"] == B["live"]).sum()) and r["n_nonfinite"] == 0


@pytest.mark.parametrize("form", U.FORMS)
def test_non_finite_radius_on_the_restatement(form):
    cam = U.planted_camera()
    P, bad = U.nonfinite_scene()
    r = U.ref_project(form, cam, P, U.TH_OVERFLOW)
    assert r["n_nonfinite"] == len(bad) and all(r["branch"][b] == B["nonfinite"] for b in bad)
    assert r["n_live"] == len(P["pos"]) - len(bad)
    assert np.isfinite(r["q"]["radius"]).all()
