"""Shared by the SearchForTriangulation tests: the CPU restatement
(tests/cpp/triangulation_ref.c, built once per process with gcc and loaded
with ctypes) and the planted inputs (two synthetic poses, descriptors in
clusters, keypoints = projections + noise).  No GPU, no orbx import."""
import ctypes
import functools

import numpy as np

import native
from native import KEYPOINT_DTYPE, ROOT, ptr as _ptr  # noqa: F401

NLEVELS = 8
FX, FY, CX, CY = 500.0, 500.0, 320.0, 240.0


class Frame(ctypes.Structure):  # tri_frame == orbx_tri_frame
    _fields_ = [("n", ctypes.c_int), ("keys", ctypes.c_void_p), ("desc", ctypes.c_void_p),
                ("has_mp", ctypes.c_void_p), ("nnodes", ctypes.c_int), ("node_id", ctypes.c_void_p),
                ("node_off", ctypes.c_void_p), ("feat", ctypes.c_void_p),
                ("level_sigma2", ctypes.c_void_p), ("nlevels", ctypes.c_int)]


@functools.lru_cache(maxsize=None)
def ref_lib():
    lib = native.ref_lib("triangulation_ref.c")
    f32, vp, ci = ctypes.c_float, ctypes.c_void_p, ctypes.c_int
    for name in ("tri_check_epipolar", "tri_check_epipolar_written"):
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = ci, [f32, f32, f32, f32, vp, f32]
    lib.tri_descriptor_distance.restype, lib.tri_descriptor_distance.argtypes = ci, [vp, vp]
    lib.tri_three_maxima.restype, lib.tri_three_maxima.argtypes = None, [vp, ci, vp]
    lib.tri_search.restype, lib.tri_search.argtypes = ci, [vp, vp, vp, ci, ci, ci, vp, vp]
    return lib


def _struct(k, keep):
    keys = np.ascontiguousarray(k["keys"], KEYPOINT_DTYPE)
    desc = np.ascontiguousarray(k["desc"], np.uint8).reshape(-1, 32)
    mp = None if k.get("has_mp") is None else np.ascontiguousarray(k["has_mp"], np.uint8)
    nid = np.ascontiguousarray(k["node_id"], np.uint32)
    off = np.ascontiguousarray(k["off"], np.uint32)
    feat = np.ascontiguousarray(k["feat"], np.uint32)
    s2 = None if k.get("level_sigma2") is None else np.ascontiguousarray(k["level_sigma2"], np.float32)
    keep.extend([keys, desc, mp, nid, off, feat, s2])
    return Frame(len(keys), _ptr(keys), _ptr(desc), _ptr(mp), len(nid), _ptr(nid), _ptr(off),
                 _ptr(feat), _ptr(s2), 0 if s2 is None else len(s2))


def epipolar(x1, y1, x2, y2, F12, sigma2, written=False):
    F = np.ascontiguousarray(F12, np.float32).reshape(9)
    fn = ref_lib().tri_check_epipolar_written if written else ref_lib().tri_check_epipolar
    return bool(fn(float(x1), float(y1), float(x2), float(y2), _ptr(F), float(sigma2)))


def three_maxima(sizes):
    s = np.ascontiguousarray(sizes, np.int32)
    ind = np.zeros(3, np.int32)
    ref_lib().tri_three_maxima(_ptr(s), len(s), _ptr(ind))
    return ind.tolist()


def ref_search(kf1, kf2, F12, only_stereo=False, check_ori=True, contracted=True):
    """The restatement on one (KF1, KF2, F12): (match12 int32[N1], nmatches,
    stats dict)."""
    keep = []
    a, b = _struct(kf1, keep), _struct(kf2, keep)
    F = np.ascontiguousarray(F12, np.float32).reshape(9)
    m = np.full(max(a.n, 1), -7, np.int32)
    st = np.zeros(4, np.int32)
    nm = ref_lib().tri_search(ctypes.byref(a), ctypes.byref(b), _ptr(F), int(bool(only_stereo)),
                              int(bool(check_ori)), int(bool(contracted)), _ptr(m), _ptr(st))
    return m[:a.n].copy(), nm, dict(multi=int(st[0]), flips=int(st[1]), evals=int(st[2]),
                                    accepted=int(st[3]))


def ref_batch(kf1, kf2_list, F12_list, only_stereo=False, check_ori=True):
    """The neighbour loop: (match12 [nkf2, N1], nmatches [nkf2], list of stats)."""
    out = [ref_search(kf1, k, F, only_stereo, check_ori) for k, F in zip(kf2_list, F12_list)]
    n1 = len(kf1["keys"])
    m = np.array([o[0] for o in out], np.int32).reshape(len(out), n1)
    return m, np.array([o[1] for o in out], np.int32), [o[2] for o in out]


# --------------------------------------------------------------------------- planted inputs
def level_sigma2():
    """mvLevelSigma2 of ORBextractor(.., 1.2, 8, ..) (float arithmetic)"""
    sf = np.ones(NLEVELS, np.float32)
    for i in range(1, NLEVELS):
        sf[i] = np.float32(sf[i - 1] * np.float32(1.2))
    return (sf * sf).astype(np.float32)


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def _skew(t):
    return np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])


K = np.array([[FX, 0, CX], [0, FY, CY], [0, 0, 1.0]])


def fundamental(R1w, t1w, R2w, t2w):
    """LocalMapping::ComputeF12: x1^T F12 x2 = 0, float32 3x3"""
    R12 = R1w @ R2w.T
    t12 = -R12 @ t2w + t1w
    Ki = np.linalg.inv(K)
    return (Ki.T @ _skew(t12) @ R12 @ Ki).astype(np.float32)


def _project(R, t, X):
    Xc = R @ X + t
    return FX * Xc[0] / Xc[2] + CX, FY * Xc[1] / Xc[2] + CY


def _flip(rng, d, k):
    d = d.copy()
    for b in rng.choice(256, size=k, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _flatten(n, lists, rng):
    """node lists of feature indices -> (node_id, off, feat)"""
    ids = sorted(lists)
    off, feat = [0], []
    for i in ids:
        feat.extend(lists[i])
        off.append(len(feat))
    return np.array(ids, np.uint32), np.array(off, np.uint32), np.array(feat, np.uint32)


def make_case(seed, nodes1, kf2_nodes, mp1=0.25, mp2=0.25, fscale=1.0):
    """nodes1: {node id: rows}; kf2_nodes: one {node id: list length} per
    neighbour.  Returns (kf1, [kf2], [F12]) as dicts of numpy arrays.

    Every node has a base descriptor; a KF1 feature is the base with up to 28
    bits flipped and observes its own 3-D point.  A KF2 list entry is, by
    draw: a second observation of a KF1 point of the node (few bits flipped,
    the relative rotation of the pair plus noise), a decoy on the same
    viewing ray at another depth (on the epipolar line, any angle), an exact
    copy of an earlier entry (a tie at equal distance), or an unrelated point
    of the node.  So distances <= 50, exact ties and 50 / 51 pairs occur, and
    a real share of candidates passes and a real share fails the epipolar
    test."""
    rng = np.random.RandomState(seed)
    s2 = level_sigma2()
    base = {}

    def node_base(i):
        if i not in base:
            base[i] = np.random.RandomState(1000003 * (seed % 1000) + i).randint(0, 256, 32).astype(np.uint8)
        return base[i]

    def point():
        z = rng.uniform(4.0, 12.0)
        return np.array([rng.uniform(-0.5, 0.5) * z, rng.uniform(-0.38, 0.38) * z, z])

    def key(u, v, ang, octv):
        k = np.zeros((), KEYPOINT_DTYPE)
        k["x"], k["y"], k["angle"], k["octave"] = u, v, ang % 360.0, octv
        k["size"], k["class_id"] = 31.0 * np.sqrt(s2[octv]), -1
        return k

    n1 = sum(nodes1.values())
    perm = rng.permutation(n1)
    keys1 = np.zeros(n1, KEYPOINT_DTYPE)
    desc1 = np.zeros((n1, 32), np.uint8)
    X1 = np.zeros((n1, 3))
    lists1, at = {}, 0
    R1, t1 = np.eye(3), np.zeros(3)
    for nid in sorted(nodes1):
        lists1[nid] = []
        for _ in range(nodes1[nid]):
            i = int(perm[at]); at += 1
            X1[i] = point()
            octv = int(rng.randint(0, NLEVELS))
            u, v = _project(R1, t1, X1[i])
            sd = 0.5 * np.sqrt(s2[octv])
            keys1[i] = key(u + rng.normal(0, sd), v + rng.normal(0, sd), rng.uniform(0, 360), octv)
            desc1[i] = _flip(rng, node_base(nid), int(rng.randint(0, 29)))
            lists1[nid].append(i)
    nid1, off1, feat1 = _flatten(n1, lists1, rng)
    kf1 = dict(keys=keys1, desc=desc1, has_mp=(rng.uniform(size=n1) < mp1).astype(np.uint8),
               node_id=nid1, off=off1, feat=feat1, level_sigma2=s2)

    kf2s, Fs = [], []
    for spec in kf2_nodes:
        R2 = _rot(rng.uniform(-0.03, 0.03), rng.uniform(-0.08, 0.08), rng.uniform(-0.05, 0.05))
        t2 = np.array([rng.choice([-1, 1]) * rng.uniform(0.3, 1.0), rng.uniform(-0.1, 0.1),
                       rng.uniform(-0.1, 0.1)])
        delta = rng.uniform(20.0, 70.0)  # the pair's relative in-plane rotation, degrees
        n2 = sum(spec.values())
        perm2 = rng.permutation(n2)
        keys2 = np.zeros(n2, KEYPOINT_DTYPE)
        desc2 = np.zeros((n2, 32), np.uint8)
        lists2, at = {}, 0
        for nid in sorted(spec):
            lists2[nid] = []
            for _ in range(spec[nid]):
                i = int(perm2[at]); at += 1
                octv = int(rng.randint(0, NLEVELS))
                sd = 1.1 * np.sqrt(s2[octv])
                r = rng.uniform()
                rows = lists1.get(nid, [])
                if r < 0.12 and lists2[nid]:  # exact copy of an earlier entry: a tie
                    j = lists2[nid][int(rng.randint(len(lists2[nid])))]
                    keys2[i], desc2[i] = keys2[j], desc2[j]
                elif r < 0.75 and rows:
                    g = rows[int(rng.randint(len(rows)))]
                    if r < 0.5:  # the same point seen from KF2
                        X, ang = X1[g], keys1[g]["angle"] - delta + rng.normal(0, 6.0)
                        d = _flip(rng, desc1[g], int(rng.randint(0, 7)))
                    else:  # decoy: same viewing ray of KF1, another depth
                        X, ang = X1[g] * rng.uniform(0.6, 1.6), rng.uniform(0, 360)
                        d = _flip(rng, desc1[g], int(rng.randint(0, 12)))
                    u, v = _project(R2, t2, X)
                    keys2[i] = key(u + rng.normal(0, sd), v + rng.normal(0, sd), ang, octv)
                    desc2[i] = d
                else:
                    u, v = _project(R2, t2, point())
                    keys2[i] = key(u, v, rng.uniform(0, 360), octv)
                    desc2[i] = _flip(rng, node_base(nid), int(rng.randint(0, 29)))
                lists2[nid].append(i)
        nid2, off2, feat2 = _flatten(n2, lists2, rng)
        kf2s.append(dict(keys=keys2, desc=desc2, has_mp=(rng.uniform(size=n2) < mp2).astype(np.uint8),
                         node_id=nid2, off=off2, feat=feat2, level_sigma2=s2))
        Fs.append((fundamental(R1, t1, R2, t2).astype(np.float64) * fscale).astype(np.float32))
    return kf1, kf2s, Fs


def _step(x, k):
    """the float32 k representable steps away from x"""
    return (np.float32(x).view(np.int32) + np.int32(k)).view(np.float32)


def boundary_point(x1, y1, x2, y2, F12, sigma2, span=400):
    """A float32 (x2', y2') close to (x2, y2), at the epipolar threshold of
    (x1, y1) under F12, where CheckDistEpipolarLine's decision differs between
    the reference object's fused form and the source-order form; None if the
    scan finds none."""
    F = np.asarray(F12, np.float32).reshape(3, 3).astype(np.float64)
    a = x1 * F[0, 0] + y1 * F[1, 0] + F[2, 0]
    b = x1 * F[0, 1] + y1 * F[1, 1] + F[2, 1]
    c = x1 * F[0, 2] + y1 * F[1, 2] + F[2, 2]
    nrm = np.hypot(a, b)
    if not nrm > 0:
        return None
    d = (a * x2 + b * y2 + c) / nrm
    r = np.sqrt(3.84 * float(sigma2))
    side = 1.0 if d >= 0 else -1.0
    bx = np.float32(x2 - (d - side * r) * a / nrm)
    by = np.float32(y2 - (d - side * r) * b / nrm)
    for ky in (0, 1, -1, 2, -2):
        yy = _step(by, ky)
        for kx in range(-span, span + 1):
            xx = _step(bx, kx)
            if epipolar(x1, y1, xx, yy, F12, sigma2) != epipolar(x1, y1, xx, yy, F12, sigma2, True):
                return float(xx), float(yy)
    return None


def plant_boundary(kf1, kf2, F12, count=8):
    """Moves up to `count` KF2 keypoints that are close candidates (distance
    <= 20) of a KF1 row without a MapPoint onto such a boundary point; returns
    how many were planted."""
    lib = ref_lib()
    done = 0
    common = set(kf1["node_id"].tolist()) & set(kf2["node_id"].tolist())
    for nid in sorted(common):
        j1 = int(np.searchsorted(kf1["node_id"], nid))
        j2 = int(np.searchsorted(kf2["node_id"], nid))
        rows = kf1["feat"][kf1["off"][j1]:kf1["off"][j1 + 1]]
        cols = kf2["feat"][kf2["off"][j2]:kf2["off"][j2 + 1]]
        for i2 in cols:
            if done >= count:
                return done
            if kf2["has_mp"][i2]:
                continue
            for i1 in rows:
                if kf1["has_mp"][i1]:
                    continue
                d = lib.tri_descriptor_distance(_ptr(np.ascontiguousarray(kf1["desc"][i1])),
                                                _ptr(np.ascontiguousarray(kf2["desc"][i2])))
                if d > 20:
                    continue
                k1, k2 = kf1["keys"][i1], kf2["keys"][i2]
                p = boundary_point(float(k1["x"]), float(k1["y"]), float(k2["x"]), float(k2["y"]), F12,
                                   float(kf2["level_sigma2"][k2["octave"]]), span=120)
                if p is not None:
                    kf2["keys"]["x"][i2], kf2["keys"]["y"][i2] = p
                    done += 1
                break
    return done
