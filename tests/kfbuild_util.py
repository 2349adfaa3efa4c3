"""Shared by the keyframe projection tests (csrc/kernels_kfbuild.hip, DESIGN.md
§18): the CPU restatement (tests/cpp/kfbuild_ref.c, built once per process with
gcc and loaded with ctypes), the random scenes and the planted edge cases.  No
GPU, no orbx import."""
import ctypes
import functools

import numpy as np

import native
from native import ROOT, ptr as _ptr  # noqa: F401
from kfwindow_util import H, KF_QUERY_DTYPE, W
from projbuild_util import _rotation, down, log_scale_factor, scale_factors, up

f32 = np.float32
MAX_LEVELS = 32
FUSE, SIM3 = 1, 2
FORMS = (FUSE, SIM3)
POINT_FIELDS = ("pos", "min_dist_inv", "max_dist_inv", "max_dist", "skip")
POINT_DTYPES = dict(pos=np.float32, min_dist_inv=np.float32, max_dist_inv=np.float32, max_dist=np.float32,
                    skip=np.uint8)
BRANCHES = ("live", "skip", "depth", "u_low", "u_high", "v_low", "v_high", "dist_low", "dist_high", "nonfinite")
B = {n: i for i, n in enumerate(BRANCHES)}
REJECTIONS = BRANCHES[1:9]  # the non-finite radius is the deviation, tested on its own
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 3000)
TH = {FUSE: 3.0, SIM3: 7.5}  # LocalMapping's Fuse default and LoopClosing's SearchBySim3
INT_MAX = 2 ** 31 - 1


class RefCamera(ctypes.Structure):
    _fields_ = [("Rcw", ctypes.c_float * 9), ("tcw", ctypes.c_float * 3), ("ow", ctypes.c_float * 3),
                ("sR21", ctypes.c_float * 9), ("t21", ctypes.c_float * 3),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("min_x", ctypes.c_float), ("max_x", ctypes.c_float), ("min_y", ctypes.c_float),
                ("max_y", ctypes.c_float), ("nlevels", ctypes.c_int), ("sf", ctypes.c_float * MAX_LEVELS),
                ("lsf", ctypes.c_float)]


class RefPoints(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in POINT_FIELDS]


@functools.lru_cache(maxsize=None)
def ref_lib():
    lib = native.ref_lib("kfbuild_ref.c")
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.kb_project.restype = None
    lib.kb_project.argtypes = [ci, ci, vp, vp, ci, ctypes.c_int32, cf, vp, vp, vp, vp]
    lib.kb_predict_scale.restype, lib.kb_predict_scale.argtypes = ci, [cf, cf, cf, ci]
    return lib


def make_camera(R, t, ow, sR21, t21, fx, fy, cx, cy, bounds, scale=1.2, nlevels=8):
    """a camera dict in the form orbx.kf_camera takes; bounds = (min_x, max_x, min_y, max_y)"""
    return dict(Rcw=np.asarray(R, np.float32).reshape(3, 3), tcw=np.asarray(t, np.float32).reshape(3),
                ow=np.asarray(ow, np.float32).reshape(3), sR21=np.asarray(sR21, np.float32).reshape(3, 3),
                t21=np.asarray(t21, np.float32).reshape(3), fx=f32(fx), fy=f32(fy), cx=f32(cx), cy=f32(cy),
                min_x=f32(bounds[0]), max_x=f32(bounds[1]), min_y=f32(bounds[2]), max_y=f32(bounds[3]),
                scale_factors=scale_factors(scale, nlevels), log_scale_factor=log_scale_factor(scale))


def _ref_camera(cam):
    c = RefCamera()
    for n in ("Rcw", "tcw", "ow", "sR21", "t21"):
        getattr(c, n)[:] = cam[n].reshape(-1).tolist()
    for n in ("fx", "fy", "cx", "cy", "min_x", "max_x", "min_y", "max_y"):
        setattr(c, n, float(cam[n]))
    sf = cam["scale_factors"]
    c.nlevels = len(sf)
    c.sf[:len(sf)] = sf.tolist()
    c.lsf = float(cam["log_scale_factor"])
    return c


def make_points(n, **arrays):
    P = dict(pos=np.zeros((n, 3), np.float32), min_dist_inv=np.zeros(n, np.float32),
             max_dist_inv=np.zeros(n, np.float32), max_dist=np.zeros(n, np.float32), skip=np.zeros(n, np.uint8))
    for k, v in arrays.items():
        P[k][...] = v
    return P


def ref_project(form, cam, P, th, desc_base=0, fused=True):
    """the restatement on one problem: dict(q, level, branch, n_live,
    n_nonfinite); the inputs are not modified"""
    arrs = {n: np.ascontiguousarray(P[n], POINT_DTYPES[n]) for n in POINT_FIELDS if P.get(n) is not None}
    n = len(arrs["pos"].reshape(-1, 3))
    pts = RefPoints(*[_ptr(arrs.get(k)) for k in POINT_FIELDS])
    c = _ref_camera(cam)
    q = np.zeros(max(n, 1), KF_QUERY_DTYPE)
    level = np.zeros(max(n, 1), np.int32)
    branch = np.zeros(max(n, 1), np.int32)
    counts = np.zeros(2, np.int32)
    ref_lib().kb_project(form, 1 if fused else 0, ctypes.byref(c), ctypes.byref(pts), n, int(desc_base), float(th),
                         _ptr(q), _ptr(level), _ptr(branch), _ptr(counts))
    out = dict(q=q[:n], level=level[:n], branch=branch[:n], n_live=int(counts[0]), n_nonfinite=int(counts[1]))
    for a in (out["q"], out["level"], out["branch"]):
        a.flags.writeable = False
    return out


def words(q):
    """query rows as uint32 words [n, 5]: the comparison is on bits"""
    return np.ascontiguousarray(q, KF_QUERY_DTYPE).view(np.uint32).reshape(-1, 5)


# --------------------------------------------------------------------------- random scenes
def random_camera(form, seed, scale=1.2, nlevels=8):
    """a camera over kfwindow_util's 640 x 480 keyframe with a random pose.
    FUSE: ow = -Rcw^T tcw in float32, as GetCameraCenter holds it.  SIM3: a
    second random similarity, sR21 = (1 / s12) R12^T and t21 = -sR21 t12 in
    float32, as the caller's cv::Mat expressions give them."""
    rng = np.random.default_rng(seed * 2 + form)
    R = _rotation(rng)
    t = rng.uniform(-2, 2, 3).astype(np.float32)
    ow = (-(R.T.astype(np.float32) @ t)).astype(np.float32)
    R12 = _rotation(rng)
    t12 = rng.uniform(-1, 1, 3).astype(np.float32)
    s12 = f32(rng.uniform(0.8, 1.25))
    sR21 = (f32(1.0 / float(s12)) * R12.T).astype(np.float32)
    t21 = (-(sR21 @ t12)).astype(np.float32)
    return make_camera(R, t, ow, sR21, t21, 517.306, 516.469, 318.643, 255.314, (0.0, W, 0.0, H), scale, nlevels)


@functools.lru_cache(maxsize=None)
def random_scene(form, n, seed, scale=1.2, nlevels=8):
    """(camera, points): n map points around the searched keyframe's frustum --
    a tenth behind it, projections over 1.3 x the image, distances from below
    to above the invariance region over every level, a twelfth skipped.  Built
    once, never modified."""
    cam = random_camera(form, seed, scale, nlevels)
    rng = np.random.default_rng(seed + 7919 * n + form)
    R, t = cam["Rcw"].astype(np.float64), cam["tcw"].astype(np.float64)
    z = np.where(rng.uniform(size=n) < 0.1, rng.uniform(-8, -0.5, n), rng.uniform(0.5, 40, n))
    u = rng.uniform(-0.15, 1.15, n) * W
    v = rng.uniform(-0.15, 1.15, n) * H
    Pc = np.stack([(u - float(cam["cx"])) / float(cam["fx"]) * z, (v - float(cam["cy"])) / float(cam["fy"]) * z, z], 1)
    dist = np.linalg.norm(Pc, axis=1) if n else np.zeros(0)  # |p - ow| = |Pc| (FUSE); |p3Dc2| (SIM3)
    if form == SIM3:  # Pc = sR21 Pc1 + t21
        Pc = np.linalg.solve(cam["sR21"].astype(np.float64), (Pc - cam["t21"].astype(np.float64)).T).T
    pos = ((Pc - t) @ R).astype(np.float32)  # R^T (Pc - t)
    top = nlevels - 1
    k = rng.uniform(-1.4, top + 1.6, n)  # ratio = scale^k: levels 0 .. top, and beyond both gates
    max_dist = (dist * scale ** k).astype(np.float32)
    P = make_points(n, pos=pos, min_dist_inv=f32(0.8) * (max_dist / cam["scale_factors"][top]),
                    max_dist_inv=f32(1.2) * max_dist, max_dist=max_dist, skip=rng.uniform(size=n) < 1 / 12)
    for a in P.values():
        a.flags.writeable = False
    return cam, P


_REF_CACHE = {}


def scene_ref(form, n, seed, fused=True):
    """ref_project of random_scene(form, n, seed) at TH[form], once per process"""
    key = (form, n, seed, fused)
    if key not in _REF_CACHE:
        cam, P = random_scene(form, n, seed)
        _REF_CACHE[key] = ref_project(form, cam, P, TH[form], fused=fused)
    return _REF_CACHE[key]


def assert_not_vacuous(form, n, seed, nlevels=8):
    """what the tests assert on the restatement of a random scene before they
    compare anything with it"""
    ref, unf = scene_ref(form, n, seed), scene_ref(form, n, seed, fused=False)
    taken = {BRANCHES[b] for b in set(ref["branch"].tolist())}
    assert set(REJECTIONS) <= taken, sorted(set(REJECTIONS) - taken)
    live = ref["branch"] == B["live"]
    assert 0.2 * n <= live.sum() <= 0.8 * n, live.sum()
    assert ref["n_live"] == live.sum() and ref["n_nonfinite"] == 0
    assert sorted(set(ref["level"][live].tolist())) == list(range(nlevels))
    both = live & (unf["branch"] == B["live"])
    differ = (ref["q"]["x"][both].view(np.uint32) != unf["q"]["x"][both].view(np.uint32)) | \
             (ref["q"]["y"][both].view(np.uint32) != unf["q"]["y"][both].view(np.uint32))
    assert differ.any(), "the scene cannot tell fma(x, fx, cx) from fx * x + cx"
    return int(differ.sum())


# --------------------------------------------------------------------------- planted edges
NEG0 = f32(-0.0)


def planted_camera(scale=1.2, nlevels=8):
    """identity rotations, translations of -0 (x + -0 = x for every x, and a
    sum of -0 terms stays -0), fx = fy = 512 and cx = cy = 0: the camera-frame
    point is the map point in both forms, u = 512 X / Z and v = 512 Y / Z hold
    exactly for Z a power of two, and the norm of a point on an axis is its
    coordinate"""
    z3 = np.full(3, NEG0, np.float32)
    return make_camera(np.eye(3), z3, np.zeros(3), np.eye(3), z3, 512.0, 512.0, 0.0, 0.0,
                       (-320.0, 320.0, -240.0, 240.0), scale, nlevels)


class Edge:
    """one planted point: its arrays' entries and what the restatement must
    give (branch name; for a live point optionally level)"""

    def __init__(self, name, branch, pos, level=None, **fields):
        self.name, self.branch, self.pos, self.level, self.fields = name, branch, pos, level, fields


WIDE = dict(min_dist_inv=0.0, max_dist_inv=3e38, max_dist=1.0)


def planted_edges(thr, nlevels=8):
    """the list of Edge under the planted camera, the same for both forms; thr =
    the PredictScale thresholds of its scale (float32[nlevels - 1])"""
    E = []
    xe, ye = f32(320.0 / 512.0), f32(240.0 / 512.0)  # u = +-320, v = +-240 exactly at Z = 1
    for name, x, y, br in (("u=min", -xe, 0.0, "live"), ("u<min", down(-xe), 0.0, "u_low"),
                           ("u=max", xe, 0.0, "u_high"), ("u<max", down(xe), 0.0, "live"),
                           ("v=min", 0.0, -ye, "live"), ("v<min", 0.0, down(-ye), "v_low"),
                           ("v=max", 0.0, ye, "v_high"), ("v<max", 0.0, down(ye), "live")):
        E.append(Edge(name, br, (x, y, 1.0), **WIDE))
    # Z == +0 and Z == -0 pass the depth test; x is +inf in both (0.25 / +0, -0.25 / -0), u too, and u < max_x fails
    E.append(Edge("Z=+0", "u_high", (0.25, 0.0, 0.0), **WIDE))
    E.append(Edge("Z=-0", "u_high", (-0.25, NEG0, NEG0), **WIDE))
    E.append(Edge("Z=-denorm", "depth", (0.0, 0.0, down(0.0)), **WIDE))
    d = f32(4.0)  # on the optical axis at a power of two: dist = 4 exactly
    E.append(Edge("dist=min", "live", (0, 0, d), min_dist_inv=d, max_dist_inv=3e38, max_dist=1.0))
    E.append(Edge("dist<min", "dist_low", (0, 0, d), min_dist_inv=up(d), max_dist_inv=3e38, max_dist=1.0))
    E.append(Edge("dist=max", "live", (0, 0, d), min_dist_inv=0.0, max_dist_inv=d, max_dist=1.0))
    E.append(Edge("dist>max", "dist_high", (0, 0, d), min_dist_inv=0.0, max_dist_inv=down(d), max_dist=1.0))
    # PredictScale at every threshold: dist = 1 on the axis, ratio = max_dist
    for L in range(nlevels - 1):
        E.append(Edge("thr[%d]" % L, "live", (0, 0, 1.0), level=L + 1, **dict(WIDE, max_dist=thr[L])))
        E.append(Edge("pred(thr[%d])" % L, "live", (0, 0, 1.0), level=L, **dict(WIDE, max_dist=down(thr[L]))))
    E.append(Edge("clamp low", "live", (0, 0, 1.0), level=0, **dict(WIDE, max_dist=1e-3)))
    E.append(Edge("clamp high", "live", (0, 0, 1.0), level=nlevels - 1, **dict(WIDE, max_dist=1e30)))
    E.append(Edge("skip", "skip", (0, 0, 1.0), skip=1, **WIDE))
    return E


def planted_points(edges):
    """(points, slot of each edge): the edges at the first and last lane of
    consecutive wavefronts (0, 63, 64, 127, .., so 63 | 64 straddles a wavefront
    and 255 | 256 a block boundary), plain live points in between"""
    waves = (len(edges) + 1) // 2
    n = 64 * max(waves, 5)
    P = make_points(n, pos=(0.1, 0.05, 1.0), **WIDE)
    slots = []
    for j, e in enumerate(edges):
        s = 64 * (j // 2) + (63 if j % 2 else 0)
        slots.append(s)
        P["pos"][s] = e.pos
        for k, v in e.fields.items():
            P[k][s] = v
    return P, slots


TH_OVERFLOW = 3e38  # th * mvScaleFactors[level] overflows from level 1 on


def nonfinite_scene():
    """(points, bad rows) under the planted camera: every point is live at
    level 0 (radius = th), the bad rows predict level 2, where TH_OVERFLOW *
    1.44 is infinite"""
    P, _ = planted_points([])
    bad = (64, 191)
    for b in bad:
        P["max_dist"][b] = 1.3
    return P, bad


def host_thresholds(lsf, nlevels):
    """thr[L] by the restatement's own PredictScale: the smallest positive
    float32 ratio whose level exceeds L (bisection over the bit patterns)"""
    lib = ref_lib()

    def level_of(bits):
        r = np.array([bits], np.uint32).view(np.float32)[0]
        return lib.kb_predict_scale(float(r), 1.0, float(lsf), nlevels)

    thr = np.zeros(nlevels - 1, np.float32)
    for L in range(nlevels - 1):
        lo, hi = 1, 0x7F7FFFFF
        assert level_of(lo) <= L < level_of(hi)
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if level_of(mid) > L:
                hi = mid
            else:
                lo = mid
        thr[L] = np.array([hi], np.uint32).view(np.float32)[0]
    return thr


def check_planted(edges, slots, out, th, cam):
    """the restatement's (or the device's) rows give what each edge names"""
    sf = cam["scale_factors"]
    for e, s in zip(edges, slots):
        assert BRANCHES[out["branch"][s]] == e.branch, (e.name, BRANCHES[out["branch"][s]])
        row = out["q"][s]
        if e.branch == "live":
            assert out["level"][s] == row["level"] >= 0, e.name
            if e.level is not None:
                assert row["level"] == e.level, (e.name, int(row["level"]))
            assert row["radius"] == f32(th) * sf[row["level"]], e.name
        else:
            assert (row["x"], row["y"], row["radius"], row["level"]) == (0.0, 0.0, -1.0, -1), e.name
            assert out["level"][s] == -1
