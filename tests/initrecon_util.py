"""Shared by the initializer-reconstruction tests (csrc/kernels_initrecon.hip,
DESIGN.md §21): the CPU restatement (tests/cpp/initrecon_ref.c, built once per
process with gcc and loaded with ctypes), two-view scenes with a known R, t and
points, and the planted cases.  No GPU, no orbx import."""
import ctypes
import functools

import numpy as np

import native
from native import ROOT, ptr as _ptr  # noqa: F401
from initransac_util import KEYPOINT_DTYPE, KSTRIDE, make_keys, match_list, same_bits  # noqa: F401

f32 = np.float32
H, F, AUTO = 0, 1, 2  # ORBX_RECON_*
SIGMA, MIN_PARALLAX, MIN_TRIANGULATED = 1.0, 1.0, 50  # Initialize :74-76
K64 = np.array([[500.0, 0, 320.0], [0, 500.0, 240.0], [0, 0, 1.0]])
RANSAC_RESULT_DTYPE = np.dtype([("H21", "<f4", (3, 3)), ("F21", "<f4", (3, 3)), ("SH", "<f4"), ("SF", "<f4"),
                                ("RH", "<f4"), ("it_H", "<i4"), ("it_F", "<i4"), ("nmatch", "<i4")])
RECON_RESULT_DTYPE = np.dtype([("ok", "<i4"), ("model_used", "<i4"), ("R21", "<f4", (3, 3)), ("t21", "<f4", (3,)),
                               ("best", "<i4"), ("ncand", "<i4"), ("nGood", "<i4", (8,)), ("parallax", "<f4", (8,)),
                               ("n_inliers", "<i4")])
assert RECON_RESULT_DTYPE.itemsize == 33 * 4
BRANCHES = ("nonfinite", "behind1", "behind2", "err1", "err2", "counted", "good")  # RC_* of initrecon_math.h
NONFINITE, BEHIND1, BEHIND2, ERR1, ERR2, COUNTED, GOOD = range(7)
H_OUT = ("h_ok", "h_similar", "h_parallax", "h_mintri", "h_inliers")
F_OUT = ("f_ok0", "f_ok1", "f_ok2", "f_ok3", "f_mingood", "f_similar", "f_fallthrough")
COUNTERS = (("absent", "early_exit") + BRANCHES + H_OUT + F_OUT +
            ("nan_cos", "j4_sweeps_max", "j4_capped", "j3_sweeps_max", "j3_capped", "winner_counted_not_good"))


@functools.lru_cache(maxsize=None)
def ref_lib():
    lib = native.ref_lib("initrecon_ref.c")
    vp, ci, cf, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double
    lib.rc_ref_reconstruct.restype = ci
    lib.rc_ref_reconstruct.argtypes = [ci, vp, ci, vp, ci, vp, vp, ci, ci, vp, vp, cf, cf, ci] + [vp] * 7
    lib.rc_ref_ncounters.restype = ci
    lib.rc_ref_choose_model.restype = ci
    lib.rc_ref_choose_model.argtypes = [cf]
    lib.rc_ref_acos.restype = cd
    lib.rc_ref_acos.argtypes = [cd]
    lib.rc_ref_parallax.restype = cf
    lib.rc_ref_parallax.argtypes = [cf]
    lib.rc_ref_th2.restype = cf
    lib.rc_ref_th2.argtypes = [cf]
    lib.rc_ref_key.restype = ctypes.c_uint32
    lib.rc_ref_key.argtypes = [cf]
    lib.rc_ref_unkey.restype = cf
    lib.rc_ref_unkey.argtypes = [ctypes.c_uint32]
    assert lib.rc_ref_ncounters() == len(COUNTERS)
    return lib


def ransac_record(H21=None, F21=None, RH=0.5, nmatch=0):
    """one orbx_ransac_result as orbm_initializer_ransac leaves it; a matrix
    that is None is absent (it = -1, zeros)"""
    r = np.zeros((), RANSAC_RESULT_DTYPE)
    r["it_H"] = r["it_F"] = -1
    if H21 is not None:
        r["H21"], r["it_H"], r["SH"] = np.asarray(H21, np.float32), 0, 1.0
    if F21 is not None:
        r["F21"], r["it_F"], r["SF"] = np.asarray(F21, np.float32), 0, 1.0
    r["RH"], r["nmatch"] = RH, nmatch
    return r


def resolve_model(pair):
    """the model the pair is taken through: AUTO by the restated :73"""
    m = int(pair["model"])
    if m == AUTO:
        m = ref_lib().rc_ref_choose_model(float(pair["ransac"]["RH"]))
    return m


def ref_reconstruct(pair, sigma=SIGMA, min_parallax=MIN_PARALLAX, min_triangulated=MIN_TRIANGULATED):
    """the restatement on one pair dict(keys1, keys2, match12, K float32[3, 3],
    model, ransac (RANSAC_RESULT_DTYPE record), inliers_H, inliers_F uint8[nmatch]
    or None): the fields of orbx_recon_result, P3D float32[n1, 3], triangulated
    uint8[n1], counters, cand float32[8, 27], branches uint8[8, N], cosv
    float32[8, N]; the inputs are not modified"""
    k1 = np.ascontiguousarray(pair["keys1"], KEYPOINT_DTYPE).reshape(-1)
    k2 = np.ascontiguousarray(pair["keys2"], KEYPOINT_DTYPE).reshape(-1)
    m12 = np.ascontiguousarray(pair["match12"], np.int32).reshape(-1)
    assert len(m12) == len(k1)
    K = np.ascontiguousarray(pair["K"], np.float32).reshape(9)
    model = resolve_model(pair)
    rs = pair["ransac"]
    M = np.ascontiguousarray(rs["F21" if model else "H21"], np.float32).reshape(9)
    present = int(rs["it_F" if model else "it_H"]) >= 0
    flags = np.ascontiguousarray(pair["inliers_F" if model else "inliers_H"], np.uint8).reshape(-1)
    nm = int((m12 >= 0).sum())
    assert len(flags) >= nm and int(rs["nmatch"]) == nm
    N = int((flags[:nm] != 0).sum())
    n1 = len(k1)
    res = np.zeros((), RECON_RESULT_DTYPE)
    P3D = np.zeros((max(n1, 1), 3), np.float32)
    tri = np.zeros(max(n1, 1), np.uint8)
    counters = np.zeros(len(COUNTERS), np.int32)
    cand = np.zeros((8, 27), np.float32)
    branches = np.zeros((8, max(N, 1)), np.uint8)
    cosv = np.zeros((8, max(N, 1)), np.float32)
    flags_c = flags if len(flags) else np.zeros(1, np.uint8)
    rc = ref_lib().rc_ref_reconstruct(n1, _ptr(k1), len(k2), _ptr(k2), KSTRIDE, _ptr(m12), _ptr(K), model, int(present),
                                      _ptr(M), _ptr(flags_c), float(sigma), float(min_parallax), int(min_triangulated),
                                      _ptr(res), _ptr(P3D), _ptr(tri), _ptr(counters), _ptr(cand), _ptr(branches),
                                      _ptr(cosv))
    if rc < 0:
        raise ValueError("ref_reconstruct: an index out of range")
    assert rc == N
    out = {k: res[k].copy() if res[k].shape else res[k].item() for k in RECON_RESULT_DTYPE.names}
    # the C side packs [8][N]
    br = branches.reshape(-1)[:8 * N].reshape(8, N) if N else np.zeros((8, 0), np.uint8)
    cs = cosv.reshape(-1)[:8 * N].reshape(8, N) if N else np.zeros((8, 0), np.float32)
    out.update(P3D=P3D[:n1], triangulated=tri[:n1], cand=cand, branches=br, cosv=cs,
               counters={k: int(counters[i]) for i, k in enumerate(COUNTERS)})
    for a in (out["P3D"], out["triangulated"], out["R21"], out["t21"], out["nGood"], out["parallax"]):
        a.flags.writeable = False
    return out


def same_recon(got, ref):
    """every output word of one pair against the restatement; returns the names
    that differ"""
    bad = [k for k in ("R21", "t21", "parallax", "P3D") if not same_bits(got[k], ref[k])]
    bad += [k for k in ("ok", "model_used", "best", "ncand", "n_inliers") if int(got[k]) != int(ref[k])]
    bad += [k for k in ("nGood", "triangulated") if not np.array_equal(got[k], ref[k])]
    return bad


# --------------------------------------------------------------------------- scenes
def _rot(ax, ay):
    cx, sx, cy, sy = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    return Ry @ Rx


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


# oblique enough that the twin solution of the homography decomposition counts
# clearly fewer points than the planted one
PLANE_N = np.array([1.0, 0.1, 1.0]) / np.linalg.norm([1.0, 0.1, 1.0])
PLANE_D = 5.0


@functools.lru_cache(maxsize=None)
def scene(kind, ninl, seed, nout=None, extra1=11, extra2=7, noise=0.0, tscale=1.0, model=None, rh=None):
    """(pair, truth): two views of ninl points with a known motion and exact
    model matrices.  Camera K64; frame 2 is X2 = R X + t with R a rotation of
    0.03 rad about y and 0.01 about x, t = tscale * (0.4, 0.05, 0.02).
    "planar": the points lie on the plane PLANE_N . X = PLANE_D and the pair is
    taken through H21 = K (R + t n^T / d) K^-1; "general": depths 3 .. 10 m,
    through F21 = K^-T [t]x R K^-1 (unit Frobenius norm).  nout further matches
    (default ninl // 4 + 3) are displaced by 30-60 px in frame 2 and carry flag
    0; extra1 / extra2 unmatched keys, all interleaved at random; uniform noise
    of +-noise px on the inliers.  truth: R, t (float64), X float64[ninl, 3] in
    frame 1, first int[ninl] (the inliers' keys in frame 1), inl int[ninl]
    (their positions in the match list), second.  Built once, never modified."""
    rng = np.random.default_rng(104729 * seed + 31 * ninl + (0 if kind == "planar" else 1))
    if nout is None:
        nout = ninl // 4 + 3
    nm = ninl + nout
    u1 = rng.uniform(30, 610, nm)
    v1 = rng.uniform(30, 450, nm)
    rays = np.stack([(u1 - K64[0, 2]) / K64[0, 0], (v1 - K64[1, 2]) / K64[1, 1], np.ones(nm)], 1)
    if kind == "planar":
        X = rays * (PLANE_D / (rays @ PLANE_N))[:, None]
    else:
        X = rays * rng.uniform(3.0, 10.0, nm)[:, None]
    R = _rot(0.01, 0.03)
    t = tscale * np.array([0.4, 0.05, 0.02])
    X2 = X @ R.T + t
    u2 = K64[0, 0] * X2[:, 0] / X2[:, 2] + K64[0, 2]
    v2 = K64[1, 1] * X2[:, 1] / X2[:, 2] + K64[1, 2]
    bad = np.zeros(nm, bool)
    bad[rng.permutation(nm)[:nout]] = True
    nz = rng.uniform(-noise, noise, (nm, 4)) if noise else np.zeros((nm, 4))
    ang = rng.uniform(0, 2 * np.pi, nm)
    mag = rng.uniform(30, 60, nm)
    u1, v1 = u1 + nz[:, 0], v1 + nz[:, 1]
    u2 = u2 + nz[:, 2] + bad * mag * np.cos(ang)
    v2 = v2 + nz[:, 3] + bad * mag * np.sin(ang)
    n1, n2 = nm + extra1, nm + extra2
    slot1 = np.sort(rng.permutation(n1)[:nm])
    slot2 = rng.permutation(n2)[:nm]
    x1, y1 = rng.uniform(0, 640, n1), rng.uniform(0, 480, n1)
    x2, y2 = rng.uniform(0, 640, n2), rng.uniform(0, 480, n2)
    x1[slot1], y1[slot1], x2[slot2], y2[slot2] = u1, v1, u2, v2
    match12 = np.full(n1, -1, np.int32)
    match12[slot1] = slot2
    Ki = np.linalg.inv(K64)
    Hm = K64 @ (R + np.outer(t, PLANE_N) / PLANE_D) @ Ki if kind == "planar" else None
    Fm = Ki.T @ _skew(t / np.linalg.norm(t)) @ R @ Ki
    Fm = Fm / np.linalg.norm(Fm)
    flags = (~bad).astype(np.uint8)
    if model is None:
        model = H if kind == "planar" else F
    if rh is None:
        rh = 0.5 if kind == "planar" else 0.2
    pair = dict(keys1=make_keys(x1, y1), keys2=make_keys(x2, y2), match12=match12, K=K64.astype(np.float32),
                model=model, ransac=ransac_record(Hm, Fm, rh, nm), inliers_H=flags, inliers_F=flags.copy())
    inl = np.nonzero(~bad)[0]
    truth = dict(R=R, t=t, X=X[inl], first=slot1[inl], second=slot2[inl], inl=inl)
    for d in (pair, truth):
        for a in d.values():
            if isinstance(a, np.ndarray) and a.shape:
                a.flags.writeable = False
    return pair, truth


_REF_CACHE = {}


def scene_ref(*a, **kw):
    """ref_reconstruct of scene(...), computed once per process"""
    key = (a, tuple(sorted(kw.items())))
    if key not in _REF_CACHE:
        _REF_CACHE[key] = ref_reconstruct(scene(*a, **kw)[0])
    return _REF_CACHE[key]


# --------------------------------------------------------------------------- a float64 port
def numpy_check_rt(R, t, k1, k2, K, th2):
    """Triangulate (:654-667) and CheckRT's loop (:763-830) in float64 numpy with
    numpy.linalg.svd, written from the reference text: k1, k2 float[N, 2] the
    inlier matches' points.  Returns (branch int[N] as BRANCHES, p3d [N, 3], cos)"""
    R, t, K = np.asarray(R, np.float64), np.asarray(t, np.float64).reshape(3), np.asarray(K, np.float64)
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    P1 = np.zeros((3, 4))
    P1[:, :3] = K
    P2 = K @ np.concatenate([R, t[:, None]], 1)
    O2 = -R.T @ t
    n = len(k1)
    branch, p3d, cos = np.zeros(n, int), np.zeros((n, 3)), np.zeros(n)
    for i in range(n):
        A = np.stack([k1[i, 0] * P1[2] - P1[0], k1[i, 1] * P1[2] - P1[1], k2[i, 0] * P2[2] - P2[0],
                      k2[i, 1] * P2[2] - P2[1]])
        vt = np.linalg.svd(A)[2]
        with np.errstate(all="ignore"):
            x = vt[3, :3] / vt[3, 3]
        p3d[i] = x
        if not np.isfinite(x).all():
            branch[i] = NONFINITE
            continue
        n1, n2 = x, x - O2
        c = n1 @ n2 / (np.linalg.norm(n1) * np.linalg.norm(n2))
        cos[i] = c
        if x[2] <= 0 and c < 0.99998:
            branch[i] = BEHIND1
            continue
        x2 = R @ x + t
        if x2[2] <= 0 and c < 0.99998:
            branch[i] = BEHIND2
            continue
        e1 = (fx * x[0] / x[2] + cx - k1[i, 0]) ** 2 + (fy * x[1] / x[2] + cy - k1[i, 1]) ** 2
        if e1 > th2:
            branch[i] = ERR1
            continue
        e2 = (fx * x2[0] / x2[2] + cx - k2[i, 0]) ** 2 + (fy * x2[1] / x2[2] + cy - k2[i, 1]) ** 2
        if e2 > th2:
            branch[i] = ERR2
            continue
        branch[i] = GOOD if c < 0.99998 else COUNTED
    return branch, p3d, cos


def inlier_points(pair):
    """the inlier matches' points of the model used: (k1 float32[N, 2], k2)"""
    first, second = match_list(pair["match12"])
    fl = np.asarray(pair["inliers_F" if resolve_model(pair) else "inliers_H"])[:len(first)] != 0
    a, b = pair["keys1"][first[fl]], pair["keys2"][second[fl]]
    return np.stack([a["x"], a["y"]], 1), np.stack([b["x"], b["y"]], 1)


# --------------------------------------------------------------------------- planted cases
def _moved(pair, truth, j, du=0.0, dv=0.0, to=None):
    """the pair with the frame-2 key of inlier j moved by (du, dv), or to `to`"""
    k2 = pair["keys2"].copy()
    s = truth["second"][j]
    if to is not None:
        k2["x"][s], k2["y"][s] = to
    else:
        k2["x"][s] += f32(du)
        k2["y"][s] += f32(dv)
    return dict(pair, keys2=k2)


def _winner_branch(pair, j):
    r = ref_reconstruct(pair)
    return r, (int(r["branches"][r["best"], j]) if r["best"] >= 0 else -1)


@functools.lru_cache(maxsize=None)
def err2_case():
    """(pair, j): a general scene in which inlier j's frame-2 key is moved off
    its epipolar line just far enough that, under the winning candidate, the
    reprojection error passes in image 1 and fails in image 2 (:818).  Found by
    a deterministic scan of the displacement: the two errors share it almost
    evenly, so the window is narrow; the camera in which the point is nearer
    takes the larger share, so the inlier nearest to camera 2 relative to
    camera 1 is used."""
    pair, truth = scene("general", 60, 11)
    X2 = truth["X"] @ truth["R"].T + truth["t"]
    j = int(np.argmax(truth["X"][:, 2] - X2[:, 2]))
    for dv in np.arange(3.6, 4.6, 0.002):
        p = _moved(pair, truth, j, dv=dv)
        _, b = _winner_branch(p, j)
        if b == ERR2:
            return p, j
    raise AssertionError("err2_case: no displacement fails in image 2 alone")


def planted_cases():
    """name -> (pair, kwargs of ref_reconstruct): the edge cases of DESIGN §21,
    each small; tests/test_initrecon.py asserts the branch each one reaches"""
    c = {}
    gen, gt = scene("general", 60, 11)
    pla, pt = scene("planar", 60, 12)
    c["h_identity"] = (dict(pla, ransac=ransac_record(np.eye(3), None, 0.5, int(pla["ransac"]["nmatch"]))), {})
    # a shorter baseline: the parallax lies between the 0.36 degrees of cos =
    # 0.99998 and the minimum of 1 degree
    c["low_parallax_h"] = (scene("planar", 60, 13, tscale=0.5)[0], {})
    c["fall_through_f"] = (scene("general", 60, 14, tscale=0.125)[0], {})
    # a baseline of 2 mm: every cosine is >= 0.99998, so the depth tests are
    # skipped, the matches are counted under several candidates and none is
    # flagged
    c["similar_h"] = (scene("planar", 60, 15, tscale=0.005)[0], {})
    c["similar_f"] = (scene("general", 60, 16, tscale=0.005)[0], {})
    c["few_inliers_h"] = (scene("planar", 40, 17)[0], {})
    # 8 of 60 flagged matches are wrong: the best candidate counts 52 > 50 but
    # not more than 0.9 * 60
    p8 = pla
    for j in range(8):
        p8 = _moved(p8, pt, 4 + 6 * j, dv=12.0)
    c["under_0_9_inliers_h"] = (p8, {})
    c["few_inliers_f"] = (scene("general", 30, 18)[0], {})
    z = np.zeros(len(gen["inliers_F"]), np.uint8)
    c["all_flags_zero_f"] = (dict(gen, inliers_F=z), {})
    c["all_flags_zero_h"] = (dict(pla, inliers_H=np.zeros(len(pla["inliers_H"]), np.uint8)), {})
    # inlier 3's frame-2 key moved along its epipolar line past the image of the
    # point at infinity: the rays meet behind both cameras
    Ki = np.linalg.inv(K64)
    j = 3
    x1 = np.array([gen["keys1"]["x"][gt["first"][j]], gen["keys1"]["y"][gt["first"][j]], 1.0])
    xinf = K64 @ gt["R"] @ Ki @ x1
    xinf = xinf[:2] / xinf[2]
    now = np.array([gen["keys2"]["x"][gt["second"][j]], gen["keys2"]["y"][gt["second"][j]]], np.float64)
    c["behind_camera"] = (_moved(gen, gt, j, to=xinf - 1.5 * (now - xinf)), {})
    c["over_th2_image1"] = (_moved(gen, gt, 5, dv=12.0), {})
    c["over_th2_image2"] = (err2_case()[0], {})
    # the frame-2 key exactly at the image of the point at infinity under the
    # planted rotation: the fourth homogeneous coordinate is 0 up to rounding
    c["point_at_infinity"] = (_moved(gen, gt, 9, to=_inf_image(gen, gt, 9)), {})
    # a calibration matrix without focal length: K.inv() is the zero matrix and
    # every triangulated point is NaN
    K0 = gen["K"].copy()
    K0[0, 0] = 0.0
    c["nonfinite_points"] = (dict(pla, K=K0), {})
    far = _far_point(gen, gt, 21)
    c["cos_at_least_0_99998"] = (far, {})
    c["absent_model_h"] = (dict(gen, model=H), {})  # the general scene carries no H21
    c["absent_model_f"] = (dict(pla, model=F, ransac=ransac_record(pla["ransac"]["H21"], None, 0.5,
                                                                  int(pla["ransac"]["nmatch"]))), {})
    # (double)0.4f = 0.4000000059... > 0.40: the float nearest 0.40 still takes H
    for name, rh in (("auto_rh_0_41", 0.41), ("auto_rh_0_40", 0.40), ("auto_rh_0_39", 0.39), ("auto_rh_nan", np.nan)):
        rs = pla["ransac"].copy()
        rs["RH"] = rh
        c[name] = (dict(pla, model=AUTO, ransac=rs), {})
    # a sigma so small that th2 rejects every rounding-size error
    c["sigma_tiny"] = (gen, dict(sigma=1e-4))
    return c


def _inf_image(pair, truth, j):
    Ki = np.linalg.inv(K64)
    x1 = np.array([pair["keys1"]["x"][truth["first"][j]], pair["keys1"]["y"][truth["first"][j]], 1.0])
    x = K64 @ truth["R"] @ Ki @ x1
    return x[:2] / x[2]


def _far_point(pair, truth, j):
    """inlier j seen as a point 2 km away: a finite point with cos > 0.99998"""
    Ki = np.linalg.inv(K64)
    x1 = np.array([pair["keys1"]["x"][truth["first"][j]], pair["keys1"]["y"][truth["first"][j]], 1.0])
    X = Ki @ x1 * 2000.0
    x = K64 @ (truth["R"] @ X + truth["t"])
    return _moved(pair, truth, j, to=x[:2] / x[2])
