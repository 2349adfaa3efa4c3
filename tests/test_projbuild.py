"""Device-side projection, the parts that need no GPU: the
PredictScale threshold tables against the host's logf, the argument checks of
the C ABI, and -- on the CPU restatement alone -- that the random scenes of the
GPU tests reach every branch and that the planted edge cases come out as
worked out by hand."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import projbuild_util as U
from projbuild_util import B, f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXHAUSTIVE_SRC = os.path.join(ROOT, "tests", "cpp", "predict_scale_exhaustive.cpp")
INCLUDE = os.path.join(ROOT, "orb-slam-system_amd", "csrc")


def libm_level(ratio, lsf, nlevels):
    """PredictScale from the ratio on, with libm's logf through ctypes and the
    object's sequence: divide, ceil, truncate (INT_MIN out of range), clamp"""
    libm = ctypes.CDLL("libm.so.6")
    libm.logf.restype, libm.logf.argtypes = ctypes.c_float, [ctypes.c_float]
    with np.errstate(all="ignore"):
        c = np.ceil(f32(f32(libm.logf(float(ratio))) / f32(lsf)))
    s = int(c) if np.isfinite(c) and -2.0 ** 31 <= c < 2.0 ** 31 else -2 ** 31
    return max(0, min(s, nlevels - 1))


@pytest.mark.parametrize("scale,nlevels", U.SCALES)
def test_thresholds_sit_on_the_level_steps(orbx_mod, scale, nlevels):
    lsf = U.log_scale_factor(scale)
    thr = orbx_mod.predict_scale_thresholds(lsf, nlevels)
    assert thr.dtype == np.float32 and len(thr) == nlevels - 1
    assert (np.diff(thr) > 0).all() and np.isfinite(thr).all() and thr[0] > 1.0
    for L in range(nlevels - 1):
        assert libm_level(thr[L], lsf, nlevels) == L + 1, (L, thr[L])
        assert libm_level(U.down(thr[L]), lsf, nlevels) == L, (L, thr[L])
        # the restatement's PredictScale (ratio = max_dist / 1) agrees
        assert U.ref_lib().pb_predict_scale(float(thr[L]), 1.0, float(lsf), nlevels) == L + 1
        assert U.ref_lib().pb_predict_scale(float(U.down(thr[L])), 1.0, float(lsf), nlevels) == L
    if (scale, nlevels) == (1.2, 8):
        assert thr[1:2].view(np.uint32)[0] == 0x3F99999B


@pytest.fixture(scope="module")
def exhaustive(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pbx") / "predict_scale_exhaustive")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-pthread", "-I", INCLUDE, "-I", os.path.join(ROOT, "include"),
                           "-o", exe, EXHAUSTIVE_SRC, "-lm"])
    return exe


@pytest.mark.parametrize("scale,nlevels", U.SCALES)
def test_threshold_count_equals_libm_for_every_positive_float(exhaustive, scale, nlevels):
    """every positive finite float: the number of thresholds it reaches is the
    level libm's logf gives, and the level never steps down (a few seconds on
    16 threads)"""
    bits = np.array([U.log_scale_factor(scale)], np.float32).view(np.uint32)[0]
    out = subprocess.check_output([exhaustive, "%08x" % bits, str(nlevels)], text=True)
    last = out.strip().splitlines()[-1]
    assert last.startswith("checked 2139095039 ratios: 0 mismatches, 0 non-monotone steps"), out


def test_threshold_argument_errors(orbx_mod):
    lib = orbx_mod.lib()
    thr = np.zeros(32, np.float32)
    p = thr.ctypes.data_as(ctypes.c_void_p)
    ok = float(U.log_scale_factor(1.2))
    assert lib.orbm_predict_scale_thresholds(ok, 8, p) == orbx_mod.OK
    assert lib.orbm_predict_scale_thresholds(ok, 1, None) == orbx_mod.OK  # one level: no threshold
    for lsf in (0.0, -0.1, float("nan"), float("inf"), 1e-8):  # logf(FLT_MAX) / 1e-8 > 2^31
        assert lib.orbm_predict_scale_thresholds(lsf, 8, p) == orbx_mod.ERR_ARG, lsf
    for nl in (0, -1, 33):
        assert lib.orbm_predict_scale_thresholds(ok, nl, p) == orbx_mod.ERR_ARG, nl
    assert lib.orbm_predict_scale_thresholds(ok, 8, None) == orbx_mod.ERR_ARG
    assert lib.orbm_predict_scale_thresholds(4.2e-8, 8, p) == orbx_mod.OK  # 88.72 / 4.2e-8 < 2^31


def _call(orbx_mod, mode, cam, P, npts, prm=(1.0, 0.5, 0), nprob=1, q=True, level=True, niv=True, cams=True,
          pts=True, counts=True, params=True):
    """orbm_project_points with chosen arguments withheld; every refusal here
    comes before the device is looked at"""
    c = (orbx_mod.ProjCamera * 1)(orbx_mod.proj_camera(cam))
    keep = {n: np.ascontiguousarray(P[n]) for n in U.POINT_FIELDS if P.get(n) is not None}
    pp = (orbx_mod.ProjPoints * 1)(orbx_mod.ProjPoints(*[None if n not in keep else keep[n].ctypes.data
                                                          for n in U.POINT_FIELDS]))
    n = np.array([npts], np.int32)
    pr = orbx_mod.ProjParams(*prm)
    qa = np.zeros(max(npts, 1), orbx_mod.PROJ_QUERY_DTYPE)
    la, na = np.zeros(max(npts, 1), np.int32), np.zeros(1, np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    return orbx_mod.lib().orbm_project_points(
        mode, nprob, ctypes.cast(c, ctypes.c_void_p) if cams else None,
        ctypes.cast(pp, ctypes.c_void_p) if pts else None, vp(n) if counts else None,
        ctypes.byref(pr) if params else None, 0, vp(qa) if q else None, vp(la) if level else None, None,
        vp(na) if niv else None)


def test_project_points_argument_errors(orbx_mod):
    cam = U.planted_camera()
    P = U.make_points(4)
    E, OK = orbx_mod.ERR_ARG, orbx_mod.OK
    assert _call(orbx_mod, 1, cam, P, 4, nprob=0) == OK  # nothing to do, nothing read
    assert _call(orbx_mod, 1, cam, P, 0) == OK           # an empty problem needs no device
    assert _call(orbx_mod, 1, cam, P, 0, q=False, level=False) == OK
    for mode in (0, 4, -1):
        assert _call(orbx_mod, mode, cam, P, 4) == E
    assert _call(orbx_mod, 1, cam, P, 4, nprob=-1) == E
    assert _call(orbx_mod, 1, cam, P, -1) == E
    for what in ("q", "level", "niv", "cams", "pts", "counts", "params"):
        assert _call(orbx_mod, 1, cam, P, 4, **{what: False}) == E, what
    for mode, needed in ((1, ("pos", "normal", "min_dist_inv", "max_dist_inv", "max_dist")),
                         (2, ("pos", "octave", "angle")), (3, ("pos", "max_dist", "angle"))):
        for name in needed:
            assert _call(orbx_mod, mode, cam, dict(P, **{name: None}), 4) == E, (mode, name)
    assert _call(orbx_mod, 2, cam, P, 4, prm=(1.0, 0.5, 3)) == E  # level_rule
    assert _call(orbx_mod, 2, cam, P, 4, prm=(1.0, 0.5, -1)) == E
    for lsf in (0.0, float("nan"), -1.0, 1e-8):
        assert _call(orbx_mod, 1, dict(cam, log_scale_factor=f32(lsf)), P, 4) == E, lsf
    bad = orbx_mod.proj_camera(cam)
    bad.nlevels = 33
    assert _call(orbx_mod, 1, bad, P, 4) == E
    bad.nlevels = 0
    assert _call(orbx_mod, 1, bad, P, 4) == E


# --------------------------------------------------------------------------- non-vacuity, restatement alone
@pytest.mark.parametrize("mode", (1, 2, 3))
@pytest.mark.parametrize("n", [n for n in U.SIZES if n >= 1025])
def test_random_scenes_reach_every_branch(mode, n):
    r = U.scene_ref(mode, n, 100 + mode, **U.MODE_ARGS[mode])
    cam, _ = U.random_scene(mode, n, 100 + mode)
    nlevels = len(cam["scale_factors"])
    hist = np.bincount(r["branch"], minlength=len(U.BRANCHES))
    for name in U.MODE_BRANCHES[mode]:
        assert hist[B[name]] >= 1, (name, hist)
    assert hist[B["nonfinite"]] == 0 and r["n_nonfinite"] == 0
    assert sum(hist[B[k]] for k in U.BRANCHES if k not in U.MODE_BRANCHES[mode] + ("live",)) == 0
    live = r["branch"] == B["live"]
    assert r["n_in_view"] == int(live.sum()) and 0.2 * n <= live.sum() <= 0.8 * n, live.mean()
    assert set(r["level"][live].tolist()) == set(range(nlevels)), sorted(set(r["level"][live].tolist()))
    assert (r["level"][~live] == -1).all()
    inert = np.array([U.INERT], U.PROJ_QUERY_DTYPE)[0]
    assert (r["q"][~live] == inert).all() and (r["q"]["radius"][live] > 0).all()
    if mode == 1:  # both radius classes
        assert (r["view_cos"][live] > 0.998).any() and (r["view_cos"][live] <= 0.998).any()
        assert (r["view_cos"][~live] == 0).all()


# --------------------------------------------------------------------------- planted edges, restatement alone
PLANTED = [(1, dict(th=1.0, viewing_cos_limit=0.5)), (1, dict(th=3.0, viewing_cos_limit=0.5)),
           (2, dict(th=7.0, level_rule=U.RULE_NEITHER)), (2, dict(th=7.0, level_rule=U.RULE_FORWARD)),
           (2, dict(th=7.0, level_rule=U.RULE_BACKWARD)), (3, dict(th=5.0))]


@pytest.mark.parametrize("mode,kw", PLANTED, ids=lambda v: str(v) if isinstance(v, int) else "-".join(
    "%s%g" % (k[:2], x) for k, x in v.items()))
def test_planted_edges_on_the_restatement(orbx_mod, mode, kw):
    cam = U.planted_camera()
    thr = orbx_mod.predict_scale_thresholds(cam["log_scale_factor"], 8)
    edges = U.planted_edges(mode, thr, **kw)
    P, slots = U.planted_points(edges)
    assert {0, 63, 64, 255, 256} <= set(slots) and len(P["pos"]) > 256
    r = U.ref_project(mode, cam, P, **kw)
    for e, s in zip(edges, slots):
        assert U.BRANCHES[r["branch"][s]] == e.branch, (e.name, U.BRANCHES[r["branch"][s]])
        if e.level is not None:
            assert r["level"][s] == e.level, (e.name, r["level"][s])
        if e.radius is not None:
            assert r["q"]["radius"][s] == f32(e.radius), (e.name, r["q"]["radius"][s], e.radius)
        if e.levels is not None:
            assert (r["q"]["min_level"][s], r["q"]["max_level"][s]) == e.levels, e.name
    by = {e.name: s for e, s in zip(edges, slots)}
    q = r["q"]
    assert q["x"][by["u=min"]] == cam["min_x"] and q["x"][by["u=max"]] == cam["max_x"]
    assert q["y"][by["v=min"]] == cam["min_y"] and q["y"][by["v=max"]] == cam["max_y"]
    filler = [i for i in range(len(P["pos"])) if i not in slots]
    assert (r["branch"][filler] == B["live"]).all()
    if mode == 1:
        fac = 1.0 if kw["th"] == 1.0 else kw["th"]
        assert q["radius"][by["cos>0.998"]] == f32(2.5 * fac) and q["radius"][by["cos<=0.998"]] == f32(4.0 * fac)
        assert r["view_cos"][by["cos=limit"]] == f32(0.5)
        # xr = u - mbf / z at z = 1
        assert q["xr"][by["u=max"]] == f32(320.0 - 32.0)
    if mode == 3:
        s = by["z<0 in image"]
        assert (q["x"][s], q["y"][s]) == (f32(-25.6), f32(-12.8)) and q["angle"][s] == f32(7.0)
