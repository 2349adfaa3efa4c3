"""Shared by the initializer-RANSAC tests (csrc/kernels_initransac.hip,
DESIGN.md §20): the CPU restatement (tests/cpp/initransac_ref.c, built once per
process with gcc and loaded with ctypes), the seeded scene generator, the set
draw and the planted cases.  No GPU, no orbx import."""
import ctypes
import functools

import numpy as np

import native
from native import KEYPOINT_DTYPE, ROOT, same_bits, ptr as _ptr  # noqa: F401

f32 = np.float32
KSTRIDE = KEYPOINT_DTYPE.itemsize // 4
COUNTERS = ("h_sweeps", "h_sweeps_max", "h_capped", "h_converged", "f_sweeps", "f_sweeps_max", "f_capped",
            "f_converged", "f3_sweeps", "f3_sweeps_max", "f3_capped", "f3_converged", "rotations", "skipped_orth",
            "skipped_floor", "h_replaced", "f_replaced")
FX = FY = 500.0
CX, CY = 320.0, 240.0
WIDTH, HEIGHT = 640, 480
SIGMA = 1.0
TH_H = f32(5.991)  # CheckHomography's th
IR_SWEEPS = 30  # csrc/initransac_math.h


@functools.lru_cache(maxsize=None)
def ref_lib():
    lib = native.ref_lib("initransac_ref.c")
    vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.ir_ref_initialize.restype = ci
    lib.ir_ref_initialize.argtypes = [ci, vp, ci, vp, ci, vp, ci, vp, cf] + [vp] * 9
    lib.ir_ref_dlt.restype = ci
    lib.ir_ref_dlt.argtypes = [vp, ci, vp, vp]
    lib.ir_ref_normalize.restype = None
    lib.ir_ref_normalize.argtypes = [vp, ci, ci, vp, vp]
    lib.ir_ref_inv3.restype = None
    lib.ir_ref_inv3.argtypes = [vp, vp]
    return lib


def make_keys(u, v):
    k = np.zeros(len(u), KEYPOINT_DTYPE)
    k["x"], k["y"] = u, v
    k["size"], k["angle"], k["class_id"] = 31.0, -1.0, -1
    return k


def match_list(match12):
    """mvMatches12: (first, second) of the rows with match12[i] >= 0, ascending i"""
    m = np.asarray(match12, np.int32)
    first = np.nonzero(m >= 0)[0].astype(np.int32)
    return first, m[first]


def ref_normalize(keys):
    """Normalize of the restatement: (points float32[n, 2], T float32[3, 3])"""
    keys = np.ascontiguousarray(keys, KEYPOINT_DTYPE)
    out = np.zeros((max(len(keys), 1), 2), np.float32)
    T = np.zeros((3, 3), np.float32)
    ref_lib().ir_ref_normalize(_ptr(keys), KSTRIDE, len(keys), _ptr(out), _ptr(T))
    return out[:len(keys)], T


def ref_dlt(pn, model):
    """the DLT matrix of 8 normalised pairs pn float32[8, 4] = (u1, v1, u2, v2)
    and the header's null vector: (A float32[m, 9], h float32[9], sweeps)"""
    pn = np.ascontiguousarray(pn, np.float32).reshape(8, 4)
    m = 8 if model else 16
    A = np.zeros((m, 9), np.float32)
    h = np.zeros(9, np.float32)
    sweeps = ref_lib().ir_ref_dlt(_ptr(pn), int(model), _ptr(A), _ptr(h))
    return A, h, sweeps


def ref_inv3(M):
    M = np.ascontiguousarray(M, np.float32).reshape(3, 3)
    R = np.zeros((3, 3), np.float32)
    ref_lib().ir_ref_inv3(_ptr(M), _ptr(R))
    return R


def ref_initialize(pair, nit, sigma=SIGMA):
    """the restatement on one pair dict(keys1, keys2, match12, sets): dict(H21,
    F21 float32[3, 3], SH, SF, RH float32, it_H, it_F, nmatch, inliers_H,
    inliers_F uint8[nmatch], counters, hyp float32[nit, 27] = H21i H12i F21i,
    it_scores float32[nit, 2]); the inputs are not modified"""
    k1 = np.ascontiguousarray(pair["keys1"], KEYPOINT_DTYPE).reshape(-1)
    k2 = np.ascontiguousarray(pair["keys2"], KEYPOINT_DTYPE).reshape(-1)
    m12 = np.ascontiguousarray(pair["match12"], np.int32).reshape(-1)
    assert len(m12) == len(k1)
    sets = np.ascontiguousarray(pair["sets"], np.int32).reshape(-1, 8)[:nit]
    assert len(sets) == nit
    nm = int((m12 >= 0).sum())
    H, F = np.zeros((3, 3), np.float32), np.zeros((3, 3), np.float32)
    scores, its = np.zeros(3, np.float32), np.zeros(2, np.int32)
    inlH, inlF = np.zeros(max(nm, 1), np.uint8), np.zeros(max(nm, 1), np.uint8)
    counters = np.zeros(len(COUNTERS), np.int32)
    hyp = np.zeros((max(nit, 1), 27), np.float32)
    its_sc = np.zeros((max(nit, 1), 2), np.float32)
    sets_c = np.ascontiguousarray(sets) if nit else np.zeros((1, 8), np.int32)
    rc = ref_lib().ir_ref_initialize(len(k1), _ptr(k1), len(k2), _ptr(k2), KSTRIDE, _ptr(m12), nit, _ptr(sets_c),
                                     float(sigma), _ptr(H), _ptr(F), _ptr(scores), _ptr(its), _ptr(inlH), _ptr(inlF),
                                     _ptr(counters), _ptr(hyp), _ptr(its_sc))
    if rc < 0:
        raise ValueError("ref_initialize: an index out of range")
    assert rc == nm
    out = dict(H21=H, F21=F, SH=scores[0], SF=scores[1], RH=scores[2], it_H=int(its[0]), it_F=int(its[1]), nmatch=nm,
               inliers_H=inlH[:nm], inliers_F=inlF[:nm], hyp=hyp[:nit], it_scores=its_sc[:nit],
               counters={k: int(counters[i]) for i, k in enumerate(COUNTERS)})
    for a in (H, F, out["inliers_H"], out["inliers_F"], out["hyp"], out["it_scores"]):
        a.flags.writeable = False
    return out


def draw_sets(nmatch, nit, rand):
    """the index draw of Initialize (:36-63): rand() -> int in [0, RAND_MAX];
    RandomInt(0, k - 1) = int(rand() / (RAND_MAX + 1.0) * k)"""
    RAND_MAX = 2147483647
    sets = np.zeros((nit, 8), np.int32)
    for it in range(nit):
        avail = list(range(nmatch))
        for j in range(8):
            randi = int((float(rand()) / (RAND_MAX + 1.0)) * len(avail))
            sets[it, j] = avail[randi]
            avail[randi] = avail[-1]
            avail.pop()
    return sets


def rng_sets(nmatch, nit, seed):
    """draw_sets over a seeded numpy generator instead of rand()"""
    rng = np.random.default_rng(7919 * seed + nmatch + 31 * nit)
    return draw_sets(nmatch, nit, lambda: int(rng.integers(0, 2147483648)))


# --------------------------------------------------------------------------- scenes
@functools.lru_cache(maxsize=None)
def scene(kind, nmatch, seed, nit=60, extra1=17, extra2=29, outliers=0.2):
    """(pair, truth): a two-view scene.  Camera fx = fy = 500, cx = 320, cy =
    240; nmatch points seen on the 640 x 480 image of frame 1 at depth 5 m,
    either "planar" (a slightly tilted plane) or "general" (depth spread -2 ..
    +5 m around it); frame 2 is rotated 0.03 rad about y and moved by (0.4,
    0.05, 0.02); uniform noise of +-0.3 px on both observations; `outliers` of
    the matches displaced by 30-60 px in frame 2; extra1 / extra2 unmatched
    keys in the frames, interleaved at random.  pair: dict(keys1, keys2,
    match12, sets (nit, 8)); truth: dict(planted uint8[nmatch]: 1 = inlier, in
    match-list order).  Built once, never modified."""
    rng = np.random.default_rng(100003 * seed + 17 * nmatch + (0 if kind == "planar" else 1))
    u1 = rng.uniform(20, WIDTH - 20, nmatch)
    v1 = rng.uniform(20, HEIGHT - 20, nmatch)
    if kind == "planar":
        z = 5.0 + 0.3 * (u1 - CX) / CX + 0.1 * (v1 - CY) / CY
    else:
        z = 5.0 + rng.uniform(-2.0, 5.0, nmatch)
    X = np.stack([(u1 - CX) / FX * z, (v1 - CY) / FY * z, z], 1)
    a = 0.03
    R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
    X2 = X @ R.T + np.array([0.4, 0.05, 0.02])
    u2 = FX * X2[:, 0] / X2[:, 2] + CX
    v2 = FY * X2[:, 1] / X2[:, 2] + CY
    noise = rng.uniform(-0.3, 0.3, (nmatch, 4))
    nout = int(round(outliers * nmatch))
    bad = np.zeros(nmatch, bool)
    bad[rng.permutation(nmatch)[:nout]] = True
    ang = rng.uniform(0, 2 * np.pi, nmatch)
    mag = rng.uniform(30, 60, nmatch)
    u1, v1 = u1 + noise[:, 0], v1 + noise[:, 1]
    u2 = u2 + noise[:, 2] + bad * mag * np.cos(ang)
    v2 = v2 + noise[:, 3] + bad * mag * np.sin(ang)
    n1, n2 = nmatch + extra1, nmatch + extra2
    slot1 = np.sort(rng.permutation(n1)[:nmatch])  # ascending: match-list order = point order
    slot2 = rng.permutation(n2)[:nmatch]
    x1 = rng.uniform(0, WIDTH, n1)
    y1 = rng.uniform(0, HEIGHT, n1)
    x2 = rng.uniform(0, WIDTH, n2)
    y2 = rng.uniform(0, HEIGHT, n2)
    x1[slot1], y1[slot1], x2[slot2], y2[slot2] = u1, v1, u2, v2
    match12 = np.full(n1, -1, np.int32)
    match12[slot1] = slot2
    pair = dict(keys1=make_keys(x1, y1), keys2=make_keys(x2, y2), match12=match12, sets=rng_sets(nmatch, nit, seed))
    for arr in pair.values():
        arr.flags.writeable = False
    planted = (~bad).astype(np.uint8)
    planted.flags.writeable = False
    return pair, dict(planted=planted)


_REF_CACHE = {}


def scene_ref(kind, nmatch, seed, nit=60, **kw):
    """ref_initialize of scene(...), computed once per process"""
    key = (kind, nmatch, seed, nit, tuple(sorted(kw.items())))
    if key not in _REF_CACHE:
        pair, _ = scene(kind, nmatch, seed, nit, **kw)
        _REF_CACHE[key] = ref_initialize(pair, nit)
    return _REF_CACHE[key]


def same_result(got, ref):
    """every output word of one pair against the restatement; returns the names
    that differ"""
    bad = [k for k in ("H21", "F21", "SH", "SF", "RH") if not same_bits(got[k], ref[k])]
    bad += [k for k in ("it_H", "it_F", "nmatch") if int(got[k]) != int(ref[k])]
    bad += [k for k in ("inliers_H", "inliers_F") if not np.array_equal(got[k], ref[k])]
    return bad


# --------------------------------------------------------------------------- planted cases
def simple_pair(u1, v1, u2, v2, sets, match12=None):
    """frames whose key i of frame 1 matches key i of frame 2 (or match12)"""
    n = len(u1)
    m = np.arange(n, dtype=np.int32) if match12 is None else np.asarray(match12, np.int32)
    return dict(keys1=make_keys(np.asarray(u1, np.float64), np.asarray(v1, np.float64)),
                keys2=make_keys(np.asarray(u2, np.float64), np.asarray(v2, np.float64)), match12=m,
                sets=np.asarray(sets, np.int32).reshape(-1, 8))


def planted_cases():
    """name -> (pair, nit, sigma): the edge cases of DESIGN §20, each small"""
    cases = {}
    base, _ = scene("general", 40, 5, nit=6)
    nm = 40
    k1, k2, m12 = base["keys1"], base["keys2"], base["match12"]
    # a set with a repeated point (rank-deficient DLT) and ordinary ones around it
    s = base["sets"].copy()
    s[1] = [3, 3, 5, 7, 9, 11, 13, 15]
    cases["repeated_point"] = (dict(keys1=k1, keys2=k2, match12=m12, sets=s), 6)
    # eight collinear points: matches 0..7 lie on one line in both frames
    n = 24
    rng = np.random.default_rng(77)
    u1 = rng.uniform(50, 590, n)
    v1 = rng.uniform(50, 430, n)
    u1[:8] = 100.0 + 40.0 * np.arange(8)
    v1[:8] = 80.0 + 20.0 * np.arange(8)
    u2, v2 = u1 + 12.0 + rng.uniform(-0.3, 0.3, n), v1 + 3.0 + rng.uniform(-0.3, 0.3, n)
    sets = np.stack([np.arange(8), np.arange(8, 16), np.arange(16, 24), np.arange(0, 24, 3)]).astype(np.int32)
    cases["collinear"] = (simple_pair(u1, v1, u2, v2, sets), 4)
    # a singular H21i: eight times the same point leaves a DLT matrix of rank 2
    # whose chosen null vector has two zero rows, so det(H21i) is exactly 0, the
    # inverse the zero matrix and the score NaN (1 / 0 * 0); it never wins
    s = base["sets"][:3].copy()
    s[0] = [2] * 8
    cases["singular_h"] = (dict(keys1=k1, keys2=k2, match12=m12, sets=s), 3)
    # no hypothesis scores above 0: unrelated point clouds and a sigma so small
    # that even the eight sampled points (exact to rounding only) fail the test
    un = 16
    cases["no_winner"] = (simple_pair(rng.uniform(0, 640, un), rng.uniform(0, 480, un), rng.uniform(0, 640, un),
                                      rng.uniform(0, 480, un), [np.arange(8), np.arange(8, 16)]), 2, 1e-6)
    # two iterations with equal scores, the largest of their model: set 1 (F's
    # best of the base scene) at iterations 1 and 3, set 0 (H's best) at 2 and 4
    b = base["sets"]
    s = np.stack([b[2], b[1], b[0], b[1], b[0], b[3]])
    cases["equal_scores"] = (dict(keys1=k1, keys2=k2, match12=m12, sets=s), 6)
    cases["nit0"] = (dict(keys1=k1, keys2=k2, match12=m12, sets=np.zeros((0, 8), np.int32)), 0)
    cases["nit1"] = (dict(keys1=k1, keys2=k2, match12=m12, sets=base["sets"][:1].copy()), 1)
    e8, _ = scene("general", 8, 3, nit=5, outliers=0.0)
    cases["eight_matches"] = (e8, 5)
    # n1 != n2, keys that no match references, -1 rows interleaved
    i5, _ = scene("planar", 33, 9, nit=7, extra1=40, extra2=3)
    cases["interleaved"] = (i5, 7)
    # two unmatched keys near FLT_MAX: Normalize's sums overflow, every
    # normalised point is NaN, no pair ever tests orthogonal and the Jacobi runs
    # to its sweep cap; all scores are NaN
    kh = np.concatenate([k1, make_keys([3e38, 3e38], [1.0, 2.0])])
    mh = np.concatenate([m12, np.full(2, -1, np.int32)])
    cases["capped"] = (dict(keys1=kh, keys2=k2, match12=mh, sets=base["sets"][:2].copy()), 2)
    assert nm == int((m12 >= 0).sum())
    return {k: (v[0], v[1], v[2] if len(v) > 2 else SIGMA) for k, v in cases.items()}


def h_square_dists(H21, H12, u1, v1, u2, v2):
    """squareDist1 and squareDist2 of CheckHomography (:294-311) in numpy
    float32, term by term as initransac_math.h writes them"""
    h, g = np.asarray(H21, np.float32).reshape(9), np.asarray(H12, np.float32).reshape(9)
    u1, v1, u2, v2 = (np.asarray(a, np.float32) for a in (u1, v1, u2, v2))
    one = f32(1.0)
    w2 = one / (g[6] * u2 + g[7] * v2 + g[8])
    a, b = (g[0] * u2 + g[1] * v2 + g[2]) * w2, (g[3] * u2 + g[4] * v2 + g[5]) * w2
    sd1 = (u1 - a) * (u1 - a) + (v1 - b) * (v1 - b)
    w1 = one / (h[6] * u1 + h[7] * v1 + h[8])
    a, b = (h[0] * u1 + h[1] * v1 + h[2]) * w1, (h[3] * u1 + h[4] * v1 + h[5]) * w1
    sd2 = (u2 - a) * (u2 - a) + (v2 - b) * (v2 - b)
    return sd1, sd2


def inv_sigma2(sigma):
    s = f32(sigma)
    return f32(1.0 / np.float64(f32(s * s)))


@functools.lru_cache(maxsize=None)
def chi_exact_case():
    """(pair, nit = 1, sigma_at, sigma_above, i): one hypothesis fitted to eight
    planted inliers of a planar scene, and two adjacent-in-effect values of sigma
    for which match i's chiSquare1 is exactly th (inlier, adds 0) and the next
    float above th (outlier); its chiSquare2 is below th at both.  Found by a
    deterministic scan of sigma's neighbouring floats; squareDist does not
    depend on sigma, so the hypothesis is the same throughout."""
    base, truth = scene("planar", 40, 4, nit=1)
    good = np.nonzero(truth["planted"])[0][:8].astype(np.int32)
    pair = dict(base, sets=good.reshape(1, 8).copy())
    ref = ref_initialize(pair, 1)
    first, second = match_list(pair["match12"])
    k1, k2 = pair["keys1"][first], pair["keys2"][second]
    sd1, sd2 = h_square_dists(ref["hyp"][0, :9], ref["hyp"][0, 9:18], k1["x"], k1["y"], k2["x"], k2["y"])
    for i in np.argsort(-sd1):
        if not truth["planted"][i] or sd1[i] <= sd2[i] * f32(1.01) or sd1[i] == 0:
            continue
        s0 = f32(np.sqrt(np.float64(sd1[i]) / np.float64(TH_H)))
        cand = [s0]
        up = dn = s0
        for _ in range(4000):
            up, dn = np.nextafter(up, f32(np.inf)), np.nextafter(dn, f32(0))
            cand += [up, dn]
        at = [s for s in cand if f32(sd1[i] * inv_sigma2(s)) == TH_H]
        if not at:
            continue
        s = min(at)  # the smallest sigma still at th; below it chi grows past th
        above = s
        while f32(sd1[i] * inv_sigma2(above)) <= TH_H:
            above = np.nextafter(above, f32(0))
        return pair, 1, float(s), float(above), int(i)
    raise AssertionError("chi_exact_case: no sigma puts a chi exactly at th")
