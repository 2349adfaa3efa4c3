"""Shared by the Sim3Solver tests (csrc/kernels_sim3.hip): the
CPU restatement (tests/cpp/sim3_ref.c, built once per process with gcc and
loaded with ctypes), the seeded scene generator, the triple draw, the closed
form of the sequential loop and the planted cases.  No GPU, no orbx import."""
import ctypes
import functools

import numpy as np

import native
from native import ROOT, same_bits, ptr as _ptr  # noqa: F401

native.REF_FLAGS.setdefault("sim3_ref.c", ("-fno-strict-aliasing",))

f32 = np.float32
COUNTERS = ("sweeps", "sweeps_max", "capped", "converged", "rotations", "skipped", "rod_identity", "nan_hyp",
            "replaced", "pass_zero", "hits", "evaluated", "zero_bound", "z_zero", "z_neg", "inert")
S3_HYP = 34  # csrc/sim3_math.h: R12 t12 s12 sR12 sR21 t21
S3_SWEEPS = 16
K = (500.0, 500.0, 320.0, 240.0)  # fx fy cx cy of both keyframes
WIDTH, HEIGHT = 640, 480
CHI2 = 9.210
INT_FIELDS = ("it_hit", "it_best", "n_best", "ncorr")
FLOAT_FIELDS = ("R12", "t12", "s12", "sR21", "t21")


@functools.lru_cache(maxsize=None)
def ref_lib():
    lib = native.ref_lib("sim3_ref.c")
    vp, ci, cf, cd = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_double
    lib.s3_ref_solve.restype = ci
    lib.s3_ref_solve.argtypes = [ci, vp, vp, vp, vp, vp, vp, ci, vp, ci, ci, ci, ci] + [vp] * 8
    lib.s3_ref_loop.restype = None
    lib.s3_ref_loop.argtypes = [vp, ci, ci, ci, vp]
    lib.s3_ref_atan2.restype = cd
    lib.s3_ref_atan2.argtypes = [cd, cf]
    lib.s3_ref_sincos.restype = None
    lib.s3_ref_sincos.argtypes = [cd, vp, vp]
    lib.s3_ref_max_error.restype = cf
    lib.s3_ref_max_error.argtypes = [cf]
    lib.s3_ref_sigma2_ok.restype = ci
    lib.s3_ref_sigma2_ok.argtypes = [cf]
    lib.s3_ref_errors.restype = None
    lib.s3_ref_errors.argtypes = [vp, vp, vp, vp]
    lib.s3_ref_horn.restype = None
    lib.s3_ref_horn.argtypes = [vp, vp, ci, vp, vp, vp]
    return lib


def _arrays(pr):
    """the contiguous arrays of a problem dict: pos1, pos2, sig1, sig2, pose[24], cams[8], triples"""
    pos1 = np.ascontiguousarray(pr["pos1"], np.float32).reshape(-1, 3)
    pos2 = np.ascontiguousarray(pr["pos2"], np.float32).reshape(-1, 3)
    s1 = np.ascontiguousarray(pr["sigma2_1"], np.float32).reshape(-1)
    s2 = np.ascontiguousarray(pr["sigma2_2"], np.float32).reshape(-1)
    pose = np.concatenate([np.asarray(pr[k], np.float32).reshape(-1) for k in ("Rcw1", "tcw1", "Rcw2", "tcw2")])
    cams = np.concatenate([np.asarray(pr[k], np.float32).reshape(-1) for k in ("K1", "K2")])
    tri = np.ascontiguousarray(pr["triples"], np.int32).reshape(-1, 3)
    assert len(pos2) == len(s1) == len(s2) == len(pos1) and len(pose) == 24 and len(cams) == 8
    return pos1, pos2, s1, s2, pose, cams, tri


def ref_solve(pr, eval_all=False, best_in=None, triples=None):
    """the restatement on one problem dict (as orbx.sim3_solve takes it): dict(
    it_hit, it_best, n_best, ncorr, R12, t12, s12, sR21, t21, inliers
    uint8[ncorr], counters, counts int32[nit] (-1 where the loop did not run;
    with eval_all every iteration), hyp float32[nit, 34], quat float32[nit, 4],
    corr float32[ncorr, 12]); the inputs are not modified"""
    if triples is not None:
        pr = dict(pr, triples=triples)
        pr.pop("nit", None)
    pos1, pos2, s1, s2, pose, cams, tri = _arrays(pr)
    n, nit = len(pos1), int(pr.get("nit", len(tri)))
    ires, fres = np.zeros(4, np.int32), np.zeros(25, np.float32)
    inl = np.zeros(max(n, 1), np.uint8)
    counters = np.zeros(len(COUNTERS), np.int32)
    counts = np.zeros(max(nit, 1), np.int32)
    hyp = np.zeros((max(nit, 1), S3_HYP), np.float32)
    quat = np.zeros((max(nit, 1), 4), np.float32)
    corr = np.zeros((max(n, 1), 12), np.float32)
    tri_c = tri if len(tri) else np.zeros((1, 3), np.int32)
    rc = ref_lib().s3_ref_solve(n, _ptr(pos1), _ptr(pos2), _ptr(s1), _ptr(s2), _ptr(pose), _ptr(cams), nit, _ptr(tri_c),
                                int(pr["min_inliers"]), 1 if pr["fix_scale"] else 0,
                                int(pr.get("best_in", 0) if best_in is None else best_in), 1 if eval_all else 0,
                                _ptr(ires), _ptr(fres), _ptr(inl), _ptr(counters), _ptr(counts), _ptr(hyp), _ptr(quat),
                                _ptr(corr))
    if rc < 0:
        raise ValueError("ref_solve: an index out of range")
    out = dict(it_hit=int(ires[0]), it_best=int(ires[1]), n_best=int(ires[2]), ncorr=int(ires[3]),
               R12=fres[:9].reshape(3, 3), t12=fres[9:12], s12=fres[12], sR21=fres[13:22].reshape(3, 3), t21=fres[22:25],
               inliers=inl[:n], counts=counts[:nit], hyp=hyp[:nit], quat=quat[:nit], corr=corr[:n],
               counters={k: int(counters[i]) for i, k in enumerate(COUNTERS)})
    for a in (fres, out["inliers"], out["counts"], out["hyp"], out["quat"], out["corr"]):
        a.flags.writeable = False
    return out


def ref_loop(counts, best_in, min_inliers):
    """the restatement's sequential loop alone: (it_hit, it_best, n_best)"""
    c = np.ascontiguousarray(counts, np.int32)
    out = np.zeros(3, np.int32)
    ref_lib().s3_ref_loop(_ptr(c if len(c) else np.zeros(1, np.int32)), len(c), int(best_in), int(min_inliers), _ptr(out))
    return tuple(int(v) for v in out)


def closed_form(counts, best_in, min_inliers):
    """it_hit, it_best, n_best by the formula of include/orbx.h: with m_i =
    max(best_in, c_j for j < i), it_hit = the first i with c_i >= m_i and c_i >
    min_inliers; it_best = the last i <= it_hit (nit - 1 without one) with c_i
    >= m_i"""
    c = np.asarray(counts, np.int64)
    if len(c) == 0:
        return -1, -1, int(best_in)
    m = np.maximum.accumulate(np.concatenate([[best_in], c[:-1]]))
    ok = c >= m
    hits = np.nonzero(ok & (c > min_inliers))[0]
    it_hit = int(hits[0]) if len(hits) else -1
    e = it_hit if it_hit >= 0 else len(c) - 1
    pas = np.nonzero(ok[:e + 1])[0]
    it_best = int(pas[-1]) if len(pas) else -1
    return it_hit, it_best, int(c[it_best]) if it_best >= 0 else int(best_in)


def ref_errors(hyp, cams, corr):
    """(err1, err2) of CheckInliers for one hypothesis row and one correspondence row"""
    err = np.zeros(2, np.float32)
    ref_lib().s3_ref_errors(_ptr(np.ascontiguousarray(hyp, np.float32)), _ptr(np.ascontiguousarray(cams, np.float32)),
                            _ptr(np.ascontiguousarray(corr, np.float32)), _ptr(err))
    return err


def ref_horn(P1, P2, fix_scale):
    """ComputeSim3 alone on three point pairs float32[3, 3] (a row per point):
    (hyp float32[34], quaternion float32[4], sweeps, capped)"""
    hyp, q, sw = np.zeros(S3_HYP, np.float32), np.zeros(4, np.float32), np.zeros(2, np.int32)
    ref_lib().s3_ref_horn(_ptr(np.ascontiguousarray(P1, np.float32)), _ptr(np.ascontiguousarray(P2, np.float32)),
                          1 if fix_scale else 0, _ptr(hyp), _ptr(q), _ptr(sw))
    return hyp, q, int(sw[0]), int(sw[1])


def draw_triples(ncorr, nit, rand):
    """the draw of iterate (:143-157): rand() -> int in [0, RAND_MAX];
    RandomInt(0, k - 1) = int(rand() / (RAND_MAX + 1.0) * k)"""
    RAND_MAX = 2147483647
    tri = np.zeros((nit, 3), np.int32)
    for it in range(nit):
        avail = list(range(ncorr))
        for j in range(3):
            randi = int((float(rand()) / (RAND_MAX + 1.0)) * len(avail))
            tri[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return tri


def rng_triples(ncorr, nit, seed):
    rng = np.random.default_rng(7919 * seed + ncorr + 31 * nit)
    return draw_triples(ncorr, nit, lambda: int(rng.integers(0, 2147483648)))


# --------------------------------------------------------------------------- scenes
def rot(axis, angle):
    """Rodrigues in double"""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx @ Kx


@functools.lru_cache(maxsize=None)
def scene(ncorr, seed, s=1.0, nit=60, fix_scale=False, min_inliers=20, outliers=0.25, noise=0.002):
    """(problem, truth).  Keyframe 1 sees ncorr points at 3-15 m depth on its
    640 x 480 image (fx = fy = 500); the true similarity X1c = s R X2c + t puts
    them in keyframe 2's camera frame, R 0.1 rad about a seeded axis, t a few
    decimetres; both keyframes have seeded world poses, so pos1 / pos2 are world
    positions in two drifted maps.  Gaussian noise of `noise` m on pos2; a share
    `outliers` of the correspondences replaced by wrong points in map 2;
    sigma2 = 1.44^level with seeded levels 0..3.  truth: dict(planted uint8[
    ncorr]: 1 = inlier, s, R, t).  Built once, never modified."""
    rng = np.random.default_rng(100003 * seed + 17 * ncorr + int(round(s * 10)))
    z = rng.uniform(3.0, 15.0, ncorr)
    u = rng.uniform(40, WIDTH - 40, ncorr)
    v = rng.uniform(40, HEIGHT - 40, ncorr)
    X1 = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], 1)
    R = rot(rng.normal(size=3), 0.1)
    t = rng.uniform(-0.3, 0.3, 3)
    X2 = (X1 - t) @ R / s  # row form of (1 / s) R^T (X1 - t)
    X2 = X2 + rng.normal(scale=noise, size=X2.shape)
    nout = int(round(outliers * ncorr))
    bad = np.zeros(ncorr, bool)
    bad[rng.permutation(ncorr)[:nout]] = True
    zb = rng.uniform(3.0, 15.0, ncorr)
    wrong = np.stack([rng.uniform(-0.5, 0.5, ncorr) * zb, rng.uniform(-0.4, 0.4, ncorr) * zb, zb], 1)
    X2[bad] = wrong[bad]
    R1, R2 = rot(rng.normal(size=3), rng.uniform(0.2, 1.0)), rot(rng.normal(size=3), rng.uniform(0.2, 1.0))
    t1, t2 = rng.uniform(-2, 2, 3), rng.uniform(-2, 2, 3)
    pos1 = (X1 - t1) @ R1  # R1^T (X1 - t1)
    pos2 = (X2 - t2) @ R2
    lv1, lv2 = rng.integers(0, 4, ncorr), rng.integers(0, 4, ncorr)
    pr = dict(pos1=pos1.astype(np.float32), pos2=pos2.astype(np.float32),
              sigma2_1=(1.44 ** lv1).astype(np.float32), sigma2_2=(1.44 ** lv2).astype(np.float32),
              Rcw1=R1.astype(np.float32), tcw1=t1.astype(np.float32), Rcw2=R2.astype(np.float32),
              tcw2=t2.astype(np.float32), K1=np.array(K, np.float32), K2=np.array(K, np.float32),
              triples=rng_triples(ncorr, nit, seed), min_inliers=min_inliers, fix_scale=bool(fix_scale), best_in=0)
    for a in pr.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    planted = (~bad).astype(np.uint8)
    planted.flags.writeable = False
    return pr, dict(planted=planted, s=s, R=R, t=t)


_REF_CACHE = {}


def scene_ref(*args, **kw):
    """ref_solve of scene(...), computed once per process"""
    key = (args, tuple(sorted(kw.items())))
    if key not in _REF_CACHE:
        _REF_CACHE[key] = ref_solve(scene(*args, **kw)[0])
    return _REF_CACHE[key]


def same_result(got, ref):
    """every output word of one problem against the restatement; the names that differ"""
    bad = [k for k in FLOAT_FIELDS if not same_bits(got[k], ref[k])]
    bad += [k for k in INT_FIELDS if int(got[k]) != int(ref[k])]
    if not np.array_equal(got["inliers"], ref["inliers"]):
        bad.append("inliers")
    return bad


# --------------------------------------------------------------------------- planted cases
def _with(pr, **kw):
    d = dict(pr)
    d.pop("nit", None)
    d.update(kw)
    return d


@functools.lru_cache(maxsize=None)
def truncation_case():
    """(problem, i): a noise-free scene with sigma2 = 1.2 throughout (bound 11,
    not 11.052), one hypothesis from three exact pairs, and correspondence i
    moved sideways in map 2 until its err2 lies in [11, 11.052): an outlier, and
    an inlier under the untruncated bound.  Its sigma2_1 is 100, so err1 never
    decides.  Found by bisection on the shift."""
    base, _ = scene(24, 3, nit=1, outliers=0.0, noise=0.0)
    n = 24
    s1 = np.full(n, 1.2, np.float32)
    s2 = np.full(n, 1.2, np.float32)
    i = 5
    s1[i] = 100.0
    tri = np.array([[0, 1, 2]], np.int32)
    R2 = np.asarray(base["Rcw2"], np.float64)
    side = R2.T @ np.array([1.0, 0.0, 0.0])  # a step along camera 2's x axis, in world coordinates
    lo, hi = 0.0, 0.5
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        pos2 = np.array(base["pos2"], np.float64)
        pos2[i] += mid * side
        pr = _with(base, pos2=pos2.astype(np.float32), sigma2_1=s1, sigma2_2=s2, triples=tri, min_inliers=3)
        r = ref_solve(pr, eval_all=True)
        e1, e2 = ref_errors(r["hyp"][0], np.concatenate([pr["K1"], pr["K2"]]), r["corr"][i])
        if 11.0 <= e2 < f32(CHI2) * f32(1.2) and e2 < np.float64(CHI2) * np.float64(f32(1.2)):
            assert e1 < 921.0
            return pr, i, float(e2)
        if e2 < 11.0:
            lo = mid
        else:
            hi = mid
    raise AssertionError("truncation_case: no shift puts err2 between the two bounds")


@functools.lru_cache(maxsize=None)
def planted_cases():
    """name -> problem dict: the edge cases of DESIGN §22, each small"""
    cases = {}
    base, truth = scene(40, 5, nit=12, min_inliers=20)
    full = ref_solve(base, eval_all=True)
    order = np.argsort(-full["counts"], kind="stable")
    good, poor = int(order[0]), int(order[-1])  # the iterations with the most and the fewest inliers
    tg, tp = base["triples"][good], base["triples"][poor]
    cg, cp = int(full["counts"][good]), int(full["counts"][poor])
    assert cg > 20 > cp, (cg, cp)
    mid = [int(i) for i in order if cp < full["counts"][i] < cg]
    # a bound of 0: nothing is ever an inlier, every iteration passes with count 0
    cases["sigma_zero"] = _with(base, sigma2_1=np.full(40, 0.1, np.float32), sigma2_2=np.full(40, 0.1, np.float32))
    cases["truncation"] = truncation_case()[0]
    # a repeated index (rank-deficient N) and three collinear points
    pos1, pos2 = np.array(base["pos1"]), np.array(base["pos2"])
    for arr in (pos1, pos2):
        arr[2] = arr[0] + f32(0.5) * (arr[1] - arr[0])
    cases["degenerate_triples"] = _with(base, pos1=pos1, pos2=pos2,
                                        triples=np.array([[3, 3, 7], [0, 1, 2], [9, 7, 9], tg], np.int32))
    # three coincident points: N = 0, the angle-axis 0 / 0, a NaN transformation
    cases["coincident"] = _with(base, triples=np.array([[4, 4, 4], tp], np.int32), min_inliers=30)
    cases["coincident_only"] = _with(base, triples=np.array([[4, 4, 4]], np.int32))
    # a point at depth 0 and one behind camera 1 (identity pose): projected as they are
    pos1 = np.array(base["pos1"], np.float64) @ np.asarray(base["Rcw1"], np.float64).T + np.asarray(base["tcw1"], np.float64)
    pos1 = pos1.astype(np.float32)
    pos1[6] = (0.3, 0.2, 0.0)
    pos1[8] = (0.5, 0.1, -4.0)
    cases["depth_zero_and_behind"] = _with(base, pos1=pos1, Rcw1=np.eye(3, dtype=np.float32),
                                           tcw1=np.zeros(3, np.float32), triples=np.array([tg, tp, tg], np.int32))
    # equal counts: below the return the last one stays; above it the first returns
    cases["equal_counts_no_hit"] = _with(base, triples=np.array([tp, tg, tp, tg, tp], np.int32), min_inliers=cg)
    cases["equal_counts_hit"] = _with(base, triples=np.array([tp, tg, tg, tp], np.int32), min_inliers=cg - 1)
    cases["hit_first"] = _with(base, triples=np.array([tg, tp, tg], np.int32))
    cases["hit_last"] = _with(base, triples=np.array([tp, tp, tp, tg], np.int32))
    cases["no_hit"] = _with(base, triples=np.array([tp, tp, tp], np.int32))
    cases["best_in_above"] = _with(base, best_in=41)
    tm = base["triples"][mid[0]] if mid else tp
    cases["best_in_between"] = _with(base, triples=np.array([tp, tm, tg, tp], np.int32), min_inliers=40,
                                     best_in=int(full["counts"][mid[0]]) if mid else cp + 1)
    cases["inert"] = _with(base, min_inliers=41)
    three, _ = scene(3, 2, nit=4, outliers=0.0, min_inliers=2)
    cases["three_correspondences"] = three
    cases["ncorr_equals_min_inliers"] = _with(base, min_inliers=40)
    cases["nit0"] = _with(base, triples=np.zeros((0, 3), np.int32))
    cases["nit1"] = _with(base, triples=np.array([tg], np.int32))
    cases["fix_scale"] = _with(base, fix_scale=True)
    return cases
