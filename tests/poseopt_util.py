"""Shared by the pose-optimisation tests (csrc/kernels_poseopt.hip, DESIGN.md
§19): the CPU restatement (tests/cpp/poseopt_ref.c, built once per process
with gcc and loaded with ctypes), the seeded scene generator and the planted
cases.  No GPU, no orbx import."""
import ctypes
import functools

import numpy as np

import native
from native import KEYPOINT_DTYPE, ROOT, same_bits, ptr as _ptr  # noqa: F401

f32 = np.float32
SEQUENTIAL, DEVICE = 0, 1
PO_T = 256  # csrc/poseopt_math.h
COUNTERS = ("accepted", "rejected", "solver_fail", "end_iters", "end_qmax", "end_rho0", "end_small", "rounds",
            "no_active", "readmitted", "invalid")
# n of the size sweep: the return-0 sizes, the one-round sizes, wavefront and
# workgroup edges, and 2 * PO_T + 77 = 589 (above 2 T, no multiple of T)
SIZES = (0, 2, 3, 9, 10, 63, 64, 65, 255, 256, 257, 1025, 2 * PO_T + 77)
FX, FY, CX, CY, MBF = 718.856, 718.856, 607.19, 185.22, 386.1448
WIDTH, HEIGHT = 1241, 376


@functools.lru_cache(maxsize=None)
def ref_lib():
    lib = native.ref_lib("poseopt_ref.c")
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.po_pose_optimization.restype = ci
    lib.po_pose_optimization.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp, vp, vp, ci, ci, vp, vp, vp, vp, vp, vp, vp]
    return lib


def inv_level_sigma2(scale=1.2, nlevels=8):
    """mvInvLevelSigma2 as ORBextractor builds it, in float32"""
    sf = [f32(1.0)]
    for _ in range(1, nlevels):
        sf.append(f32(sf[-1] * f32(scale)))
    return np.array([f32(1.0) / f32(s * s) for s in sf], np.float32)


def make_camera(Tcw, fx=FX, fy=FY, cx=CX, cy=CY, mbf=MBF, sigma=None):
    """a camera dict in the form orbx.pose_camera takes"""
    return dict(Tcw=np.asarray(Tcw, np.float32).reshape(-1, 4)[:3].copy(), fx=f32(fx), fy=f32(fy), cx=f32(cx),
                cy=f32(cy), mbf=f32(mbf), inv_level_sigma2=inv_level_sigma2() if sigma is None else sigma)


def make_keys(u, v, octave):
    k = np.zeros(len(u), KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"] = u, v, octave
    k["size"], k["angle"], k["class_id"] = 31.0, 0.0, -1
    return k


def ref_optimize(cam, obs, order=DEVICE):
    """the restatement on one problem: dict(Tcw float32[4, 4], outlier uint8[n],
    ninliers, pose7: the estimate in double (q.xyzw, t; NaN on the return-0
    path), counters: dict over COUNTERS); the inputs are not modified"""
    keys = np.ascontiguousarray(obs["keys"], KEYPOINT_DTYPE).reshape(-1)
    n = len(keys)
    pos = np.ascontiguousarray(obs["pos"], np.float32).reshape(-1, 3)
    opt = {k: (None if obs.get(k) is None else np.ascontiguousarray(obs[k], t))
           for k, t in (("uright", np.float32), ("point_index", np.int32), ("has_point", np.uint8))}
    Tcw = np.ascontiguousarray(np.asarray(cam["Tcw"], np.float32).reshape(-1, 4)[:3])
    intr = np.array([cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["mbf"]], np.float32)
    sg = np.ascontiguousarray(cam["inv_level_sigma2"], np.float32)
    T = np.zeros((4, 4), np.float32)
    outlier = np.zeros(max(n, 1), np.uint8)
    counters = np.zeros(len(COUNTERS), np.int32)
    edges = np.zeros(max(n, 1) * 8, np.float64)  # po_edge: 7 doubles and an int
    has = np.zeros(max(n, 1), np.uint8)
    ever = np.zeros(max(n, 1), np.uint8)
    pose7 = np.full(7, np.nan)
    nin = ref_lib().po_pose_optimization(_ptr(Tcw), _ptr(intr), len(sg), _ptr(sg), n, _ptr(keys), _ptr(opt["uright"]),
                                         _ptr(pos), _ptr(opt["point_index"]), _ptr(opt["has_point"]), len(pos),
                                         int(order), _ptr(T), _ptr(outlier), _ptr(counters), _ptr(edges), _ptr(has),
                                         _ptr(ever), _ptr(pose7))
    out = dict(Tcw=T, outlier=outlier[:n], ninliers=int(nin), pose7=pose7,
               counters={k: int(counters[i]) for i, k in enumerate(COUNTERS)})
    T.flags.writeable = False
    out["outlier"].flags.writeable = False
    return out


# --------------------------------------------------------------------------- scenes
def rotation(a):
    """Rz(a[2]) Ry(a[1]) Rx(a[0]) in double"""
    cx, cy, cz = np.cos(a)
    sx, sy, sz = np.sin(a)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def pose_matrix(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


@functools.lru_cache(maxsize=None)
def scene(n, seed, stereo="mixed", noise=0.0, outliers=0.0, perturb=(0.03, 0.05), form="plain"):
    """(camera, obs, truth): n features with map points 2-30 m in front of a
    random pose, projected in double and rounded to float keypoints, an octave
    per feature.  stereo: "mono" | "stereo" | "mixed" (every third feature
    mono).  noise: uniform pixel noise of the inliers; outliers: the share of
    features displaced by 30-60 px.  The start pose is the true one perturbed
    by up to perturb[0] rad per axis and perturb[1] m.  form: "plain" (pos[i]
    is feature i's point), "mask" (has_point clears a fifth) or "index" (a
    shuffled pool of 2 n + 5 positions with -1 for a fifth).  truth: dict(Tcw
    4x4 double, planted uint8[n], has uint8[n]).  Built once, never modified."""
    rng = np.random.default_rng(1000003 * seed + n)
    R = rotation(rng.uniform(-0.3, 0.3, 3))
    t = rng.uniform(-2, 2, 3)
    z = rng.uniform(2, 30, n)
    u = rng.uniform(20, WIDTH - 20, n)
    v = rng.uniform(20, HEIGHT - 20, n)
    Pc = np.stack([(u - CX) / FX * z, (v - CY) / FY * z, z], 1)
    pos = ((Pc - t) @ R).astype(np.float32)  # R^T (Pc - t), rounded: the map is float
    Pc = pos.astype(np.float64) @ R.T + t      # the observation is that of the float point
    u = Pc[:, 0] / Pc[:, 2] * FX + CX
    v = Pc[:, 1] / Pc[:, 2] * FY + CY
    ur = u - MBF / Pc[:, 2]
    planted = (rng.uniform(size=n) < outliers).astype(np.uint8)
    du = rng.uniform(-noise, noise, (n, 3))
    ang = rng.uniform(0, 2 * np.pi, n)
    mag = rng.uniform(30, 60, n)
    u = u + du[:, 0] + planted * mag * np.cos(ang)
    v = v + du[:, 1] + planted * mag * np.sin(ang)
    ur = ur + du[:, 2] + planted * mag * np.cos(ang) * 1.5
    octave = rng.integers(0, 8, n)
    if stereo == "mono":
        is_mono = np.ones(n, bool)
    elif stereo == "stereo":
        is_mono = np.zeros(n, bool)
    else:
        is_mono = np.arange(n) % 3 == 0
    uright = np.where(is_mono, -1.0, ur).astype(np.float32)
    dR = rotation(rng.uniform(-perturb[0], perturb[0], 3))
    dt = rng.uniform(-perturb[1], perturb[1], 3)
    T_true = pose_matrix(R, t)
    T0 = pose_matrix(dR, dt) @ T_true
    cam = make_camera(T0)
    obs = dict(keys=make_keys(u, v, octave), uright=uright, pos=pos, point_index=None, has_point=None)
    has = np.ones(n, np.uint8)
    if form == "mask":
        has = (rng.uniform(size=n) >= 0.2).astype(np.uint8)
        obs["has_point"] = has
    elif form == "index":
        has = (rng.uniform(size=n) >= 0.2).astype(np.uint8)
        pool = rng.uniform(-50, 50, (2 * n + 5, 3)).astype(np.float32)
        where = rng.permutation(2 * n + 5)[:n].astype(np.int32)
        pool[where] = pos
        obs["pos"] = pool
        obs["point_index"] = np.where(has != 0, where, -1).astype(np.int32)
    for a in obs.values():
        if a is not None:
            a.flags.writeable = False
    truth = dict(Tcw=T_true, planted=planted, has=has)
    return cam, obs, truth


_REF_CACHE = {}


def scene_ref(n, seed, order=DEVICE, **kw):
    """ref_optimize of scene(n, seed, **kw), computed once per process"""
    key = (n, seed, order, tuple(sorted(kw.items())))
    if key not in _REF_CACHE:
        cam, obs, _ = scene(n, seed, **kw)
        _REF_CACHE[key] = ref_optimize(cam, obs, order)
    return _REF_CACHE[key]


def pose_error(T, T_true):
    """(rotation angle in rad, translation distance in m) between two poses"""
    T = np.asarray(T, np.float64)
    dR = T[:3, :3] @ np.asarray(T_true)[:3, :3].T
    c = min(1.0, max(-1.0, (np.trace(dR) - 1) / 2))
    # the small angle from the skew part: arccos loses it below 1e-8
    s = 0.5 * np.linalg.norm([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]])
    return float(np.arctan2(s, c)), float(np.linalg.norm(T[:3, 3] - np.asarray(T_true)[:3, 3]))


OUTLIER_SCENE = dict(noise=0.5, outliers=0.2)


def sweep_scene(n, seed=11):
    """the GPU size sweep's problem of n features: mixed, planted outliers"""
    return scene(n, seed + n, **OUTLIER_SCENE)


# --------------------------------------------------------------------------- semantics cases
def axis_scene(points, obs_uv, uright=None, octave=0, Tcw=None):
    """the camera at the origin (or Tcw) with fx = fy = 512, cx = cy = 0,
    mbf = 32 and hand-placed points / observations"""
    n = len(points)
    cam = make_camera(np.eye(4) if Tcw is None else Tcw, 512.0, 512.0, 0.0, 0.0, 32.0)
    uv = np.asarray(obs_uv, np.float64).reshape(n, 2)
    ur = -np.ones(n, np.float32) if uright is None else np.asarray(uright, np.float32)
    obs = dict(keys=make_keys(uv[:, 0], uv[:, 1], octave), uright=ur, pos=np.asarray(points, np.float32).reshape(n, 3),
               point_index=None, has_point=None)
    return cam, obs
