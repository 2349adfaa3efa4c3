"""Shared by the device-side projection tests (csrc/kernels_projbuild.hip,
DESIGN.md §17): the CPU restatement (tests/cpp/projbuild_ref.c, built once per
process with gcc and loaded with ctypes), the random scenes and the planted
edge cases.  No GPU, no orbx import."""
import ctypes
import functools

import numpy as np

import native
from native import ROOT, ptr as _ptr  # noqa: F401
from projection_util import PROJ_QUERY_DTYPE, geometry

f32 = np.float32
MAX_LEVELS = 32
POINT_FIELDS = ("pos", "normal", "min_dist_inv", "max_dist_inv", "max_dist", "octave", "angle", "skip")
POINT_DTYPES = dict(pos=np.float32, normal=np.float32, min_dist_inv=np.float32, max_dist_inv=np.float32,
                    max_dist=np.float32, octave=np.int32, angle=np.float32, skip=np.uint8)
BRANCHES = ("live", "skip", "depth", "u_low", "u_high", "v_low", "v_high", "dist_low", "dist_high", "view_cos",
            "nonfinite")
B = {n: i for i, n in enumerate(BRANCHES)}
# the rejection branches each mode has (the non-finite row is the deviation, tested on its own)
MODE_BRANCHES = {1: BRANCHES[1:10], 2: BRANCHES[1:7], 3: (BRANCHES[1],) + BRANCHES[3:7]}
INERT = (0.0, 0.0, -1.0, -1, -1, 0.0, 0.0)
RULE_NEITHER, RULE_FORWARD, RULE_BACKWARD = 0, 1, 2
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1025, 3000)
SCALES = ((1.2, 8), (2.0, 4), (1.05, 12))


class RefCamera(ctypes.Structure):
    _fields_ = [("Rcw", ctypes.c_float * 9), ("tcw", ctypes.c_float * 3), ("ow", ctypes.c_float * 3),
                ("fx", ctypes.c_float), ("fy", ctypes.c_float), ("cx", ctypes.c_float), ("cy", ctypes.c_float),
                ("mbf", ctypes.c_float), ("min_x", ctypes.c_float), ("max_x", ctypes.c_float),
                ("min_y", ctypes.c_float), ("max_y", ctypes.c_float), ("nlevels", ctypes.c_int),
                ("sf", ctypes.c_float * MAX_LEVELS), ("lsf", ctypes.c_float)]


class RefPoints(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in POINT_FIELDS]


@functools.lru_cache(maxsize=None)
def ref_lib():
    lib = native.ref_lib("projbuild_ref.c")
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.pb_project.restype = None
    lib.pb_project.argtypes = [ci, vp, vp, ci, cf, cf, ci, vp, vp, vp, vp, vp]
    lib.pb_predict_scale.restype, lib.pb_predict_scale.argtypes = ci, [cf, cf, cf, ci]
    return lib


def scale_factors(scale, nlevels):
    """mvScaleFactor as ORBextractor builds it: repeated float32 products"""
    sf = [f32(1.0)]
    for _ in range(1, nlevels):
        sf.append(f32(sf[-1] * f32(scale)))
    return np.array(sf, np.float32)


def log_scale_factor(scale):
    return f32(np.log(f32(scale)))  # Frame.cc: mfLogScaleFactor = log(mfScaleFactor), a float


def make_camera(R, t, ow, fx, fy, cx, cy, mbf, bounds, scale=1.2, nlevels=8):
    """a camera dict in the form orbx.proj_camera takes; bounds = (min_x, max_x, min_y, max_y)"""
    return dict(Rcw=np.asarray(R, np.float32).reshape(3, 3), tcw=np.asarray(t, np.float32).reshape(3),
                ow=np.asarray(ow, np.float32).reshape(3), fx=f32(fx), fy=f32(fy), cx=f32(cx), cy=f32(cy),
                mbf=f32(mbf), min_x=f32(bounds[0]), max_x=f32(bounds[1]), min_y=f32(bounds[2]),
                max_y=f32(bounds[3]), scale_factors=scale_factors(scale, nlevels),
                log_scale_factor=log_scale_factor(scale))


def _ref_camera(cam):
    c = RefCamera()
    c.Rcw[:] = cam["Rcw"].reshape(9).tolist()
    c.tcw[:] = cam["tcw"].tolist()
    c.ow[:] = cam["ow"].tolist()
    for n in ("fx", "fy", "cx", "cy", "mbf", "min_x", "max_x", "min_y", "max_y"):
        setattr(c, n, float(cam[n]))
    sf = cam["scale_factors"]
    c.nlevels = len(sf)
    c.sf[:len(sf)] = sf.tolist()
    c.lsf = float(cam["log_scale_factor"])
    return c


def make_points(n, **arrays):
    """the point dict of n entries: every array a mode may read, zeros where not given"""
    P = dict(pos=np.zeros((n, 3), np.float32), normal=np.zeros((n, 3), np.float32),
             min_dist_inv=np.zeros(n, np.float32), max_dist_inv=np.zeros(n, np.float32),
             max_dist=np.zeros(n, np.float32), octave=np.zeros(n, np.int32), angle=np.zeros(n, np.float32),
             skip=np.zeros(n, np.uint8))
    for k, v in arrays.items():
        P[k][...] = v
    return P


def ref_project(mode, cam, P, th=1.0, viewing_cos_limit=0.5, level_rule=RULE_NEITHER):
    """the restatement on one problem: dict(q, level, view_cos, branch,
    n_in_view, n_nonfinite); the inputs are not modified"""
    arrs = {n: np.ascontiguousarray(P[n], POINT_DTYPES[n]) for n in POINT_FIELDS if P.get(n) is not None}
    n = len(arrs["pos"].reshape(-1, 3))
    pts = RefPoints(*[_ptr(arrs.get(k)) for k in POINT_FIELDS])
    c = _ref_camera(cam)
    q = np.zeros(max(n, 1), PROJ_QUERY_DTYPE)
    level = np.zeros(max(n, 1), np.int32)
    vc = np.zeros(max(n, 1), np.float32)
    branch = np.zeros(max(n, 1), np.int32)
    counts = np.zeros(2, np.int32)
    ref_lib().pb_project(mode, ctypes.byref(c), ctypes.byref(pts), n, float(th), float(viewing_cos_limit),
                         int(level_rule), _ptr(q), _ptr(level), _ptr(vc), _ptr(branch), _ptr(counts))
    out = dict(q=q[:n], level=level[:n], view_cos=vc[:n] if mode == 1 else None, branch=branch[:n],
               n_in_view=int(counts[0]), n_nonfinite=int(counts[1]))
    for a in (out["q"], out["level"], out["branch"]):
        a.flags.writeable = False
    return out


# --------------------------------------------------------------------------- random scenes
def _rotation(rng):
    a = rng.uniform(-0.3, 0.3, 3)
    cx, cy, cz = np.cos(a)
    sx, sy, sz = np.sin(a)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return (Rz @ Ry @ Rx).astype(np.float32)


def random_camera(seed, scale=1.2, nlevels=8):
    """a KITTI-like camera over projection_util's "plain" frame (1241 x 376)
    with a random pose; ow = -Rcw^T tcw in float32, as the caller computes it"""
    rng = np.random.default_rng(seed)
    g = geometry("plain")
    R = _rotation(rng)
    t = rng.uniform(-2, 2, 3).astype(np.float32)
    ow = (-(R.T.astype(np.float32) @ t)).astype(np.float32)
    return make_camera(R, t, ow, 718.856, 718.856, 607.19, 185.22, 386.1448,
                       (g["min_x"], g["max_x"], g["min_y"], g["max_y"]), scale, nlevels)


@functools.lru_cache(maxsize=None)
def random_scene(mode, n, seed, scale=1.2, nlevels=8):
    """(camera, points): n map points around the frustum -- a tenth behind the
    camera, projections over 1.2 x the image, distances from below to above
    the invariance region over every level, viewing angles to both sides of
    the limit 0.5 and of 0.998, a twelfth skipped.  Built once, never modified."""
    cam = random_camera(seed, scale, nlevels)
    rng = np.random.default_rng(seed + 7919 * n + mode)
    R, t, ow = cam["Rcw"].astype(np.float64), cam["tcw"].astype(np.float64), cam["ow"].astype(np.float64)
    z = np.where(rng.uniform(size=n) < 0.1, rng.uniform(-8, -0.5, n), rng.uniform(0.5, 40, n))
    w, h = float(cam["max_x"] - cam["min_x"]), float(cam["max_y"] - cam["min_y"])
    u = float(cam["min_x"]) + rng.uniform(-0.1, 1.1, n) * w
    v = float(cam["min_y"]) + rng.uniform(-0.1, 1.1, n) * h
    Pc = np.stack([(u - float(cam["cx"])) / float(cam["fx"]) * z, (v - float(cam["cy"])) / float(cam["fy"]) * z, z], 1)
    pos = ((Pc - t) @ R).astype(np.float32)  # R^T (Pc - t)
    PO = pos.astype(np.float64) - ow
    dist = np.linalg.norm(PO, axis=1) if n else np.zeros(0)
    top = nlevels - 1
    k = rng.uniform(-1.4, top + 1.6, n)  # ratio = scale^k: levels 0 .. top, and beyond both gates
    max_dist = (dist * scale ** k).astype(np.float32)
    c = np.where(rng.uniform(size=n) < 0.2, rng.uniform(0.9975, 1.0, n), rng.uniform(0.35, 0.9975, n))
    perp = np.cross(PO, rng.normal(size=(n, 3)))
    perp /= np.maximum(np.linalg.norm(perp, axis=1, keepdims=True), 1e-30)
    normal = (c[:, None] * PO / np.maximum(dist[:, None], 1e-30) + np.sqrt(1 - c * c)[:, None] * perp).astype(np.float32)
    P = make_points(n, pos=pos, normal=normal, min_dist_inv=f32(0.8) * (max_dist / cam["scale_factors"][top]),
                    max_dist_inv=f32(1.2) * max_dist, max_dist=max_dist, octave=rng.integers(0, nlevels, n),
                    angle=rng.uniform(0, 360, n), skip=rng.uniform(size=n) < 1 / 12)
    for a in P.values():
        a.flags.writeable = False
    return cam, P


_REF_CACHE = {}


def scene_ref(mode, n, seed, **kw):
    """ref_project of random_scene(mode, n, seed), computed once per process"""
    key = (mode, n, seed, tuple(sorted(kw.items())))
    if key not in _REF_CACHE:
        cam, P = random_scene(mode, n, seed)
        _REF_CACHE[key] = ref_project(mode, cam, P, **kw)
    return _REF_CACHE[key]


MODE_ARGS = {1: dict(th=3.0, viewing_cos_limit=0.5), 2: dict(th=15.0, level_rule=RULE_NEITHER), 3: dict(th=10.0)}


# --------------------------------------------------------------------------- planted edges
def up(v):
    return np.nextafter(f32(v), f32(np.inf))


def down(v):
    return np.nextafter(f32(v), f32(-np.inf))


def planted_camera(scale=1.2, nlevels=8):
    """the camera at the origin with identity rotation, fx = fy = 512 and
    cx = cy = 0: Pc = P, u = 512 X / Z and v = 512 Y / Z hold exactly for Z a
    power of two, and the norm of a point on an axis is its coordinate"""
    return make_camera(np.eye(3), np.zeros(3), np.zeros(3), 512.0, 512.0, 0.0, 0.0, 32.0,
                       (-320.0, 320.0, -240.0, 240.0), scale, nlevels)


def first_above_0998():
    """the smallest float32 that is > 0.998 as a double"""
    c = f32(0.998)
    while float(c) > 0.998:
        c = down(c)
    while not float(c) > 0.998:
        c = up(c)
    return c


class Edge:
    """one planted point: its arrays' entries and what the restatement must
    give (branch name; for a live point optionally level, radius, levels)"""

    def __init__(self, name, branch, pos, level=None, radius=None, levels=None, **fields):
        self.name, self.branch, self.pos, self.level, self.radius, self.levels = name, branch, pos, level, radius, levels
        self.fields = fields


WIDE = dict(min_dist_inv=0.0, max_dist_inv=3e38)


def planted_edges(mode, thr, th=1.0, viewing_cos_limit=0.5, level_rule=RULE_NEITHER, nlevels=8):
    """the list of Edge for `mode` under the planted camera; thr = the
    PredictScale thresholds of its scale (float32[nlevels - 1])"""
    sf = scale_factors(1.2, nlevels)
    E = []
    xe, ye = f32(320.0 / 512.0), f32(240.0 / 512.0)  # u = +-320, v = +-240 exactly at Z = 1
    m1 = dict(WIDE, normal=(0.0, 0.0, 1.0), max_dist=1.0) if mode == 1 else dict(max_dist=1.0)
    for name, x, y, br in (("u=min", -xe, 0.0, "live"), ("u=max", xe, 0.0, "live"),
                           ("u<min", down(-xe), 0.0, "u_low"), ("u>max", up(xe), 0.0, "u_high"),
                           ("v=min", 0.0, -ye, "live"), ("v=max", 0.0, ye, "live"),
                           ("v<min", 0.0, down(-ye), "v_low"), ("v>max", 0.0, up(ye), "v_high")):
        E.append(Edge(name, br, (x, y, 1.0), **m1))
    if mode == 1:
        d = f32(3.0)  # on the optical axis: dist = 3 exactly, view_cos = the normal's z exactly
        axis = dict(normal=(0.0, 0.0, 1.0), max_dist=1.0)
        E.append(Edge("dist=min", "live", (0, 0, d), min_dist_inv=d, max_dist_inv=3e38, **axis))
        E.append(Edge("dist<min", "dist_low", (0, 0, d), min_dist_inv=up(d), max_dist_inv=3e38, **axis))
        E.append(Edge("dist=max", "live", (0, 0, d), min_dist_inv=0.0, max_dist_inv=d, **axis))
        E.append(Edge("dist>max", "dist_high", (0, 0, d), min_dist_inv=0.0, max_dist_inv=down(d), **axis))
        lim = f32(viewing_cos_limit)
        E.append(Edge("cos=limit", "live", (0, 0, d), normal=(0, 0, lim), max_dist=1.0, **WIDE))
        E.append(Edge("cos<limit", "view_cos", (0, 0, d), normal=(0, 0, down(lim)), max_dist=1.0, **WIDE))
        c1 = first_above_0998()
        fac = f32(th) if th != 1.0 else f32(1.0)
        E.append(Edge("cos>0.998", "live", (0, 0, d), normal=(0, 0, c1), max_dist=1.0, level=0,
                      radius=f32(f32(2.5) * fac) * sf[0], **WIDE))
        E.append(Edge("cos<=0.998", "live", (0, 0, d), normal=(0, 0, down(c1)), max_dist=1.0, level=0,
                      radius=f32(f32(4.0) * fac) * sf[0], **WIDE))
        # PcZ == 0 passes the depth test; u is infinite and the bounds reject it
        E.append(Edge("PcZ=0", "u_high", (0.25, 0.0, 0.0), **m1))
        # a position of -0 is +0 once the row sum has added 0 * X: the same outcome
        E.append(Edge("PcZ=-0", "u_high", (0.25, 0.0, -0.0), **m1))
        E.append(Edge("PcZ<0", "depth", (0.0, 0.0, down(0.0)), **m1))
    if mode == 2:
        E.append(Edge("z=0", "depth", (0.1, 0.1, 0.0)))
        E.append(Edge("z<0", "depth", (0.1, 0.1, -1.0)))
        for o in (0, nlevels - 1):
            lv = {RULE_FORWARD: (o, -1), RULE_BACKWARD: (0, o), RULE_NEITHER: (o - 1, o + 1)}[level_rule]
            E.append(Edge("octave=%d" % o, "live", (0.1, 0.05, 1.0), octave=o, angle=33.0 + o, level=o,
                          radius=f32(th) * sf[o], levels=lv))
    if mode == 3:
        # no depth test: behind the camera, the mirrored projection is inside the image
        E.append(Edge("z<0 in image", "live", (0.1, 0.05, -2.0), max_dist=1.0, angle=7.0))
    if mode != 2:
        # PredictScale at every threshold: dist = 1 on the axis, ratio = max_dist
        for L in range(nlevels - 1):
            for nm, md, lv in (("thr[%d]" % L, thr[L], L + 1), ("pred(thr[%d])" % L, down(thr[L]), L)):
                r = f32(th) * sf[lv] if mode == 3 else None
                E.append(Edge(nm, "live", (0, 0, 1.0), level=lv, radius=r,
                              levels=(lv - 1, lv) if mode == 1 else (lv - 1, lv + 1), **dict(m1, max_dist=md)))
        E.append(Edge("level 0", "live", (0, 0, 1.0), level=0, levels=(-1, 0) if mode == 1 else (-1, 1),
                      **dict(m1, max_dist=0.5)))
    return E


def planted_points(edges):
    """(points, slot of each edge): the edges at the first and last lane of
    consecutive wavefronts (0, 63, 64, 127, .., so 255 | 256 straddles a block
    boundary), plain live points in between"""
    waves = (len(edges) + 1) // 2
    n = 64 * max(waves, 5)
    P = make_points(n, pos=(0.1, 0.05, 1.0), normal=(0.0, 0.0, 1.0), min_dist_inv=0.0, max_dist_inv=3e38,
                    max_dist=1.0, octave=1, angle=11.0)
    slots = []
    for j, e in enumerate(edges):
        s = 64 * (j // 2) + (63 if j % 2 else 0)
        slots.append(s)
        P["pos"][s] = e.pos
        for k, v in e.fields.items():
            P[k][s] = v
    return P, slots
