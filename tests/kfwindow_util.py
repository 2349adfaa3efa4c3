"""Shared by the keyframe window search tests (ORBmatcher::Fuse /
SearchBySim3): the CPU restatement (tests/cpp/kfwindow_ref.c, built once per
process with gcc and loaded with ctypes) and the planted inputs (queries =
a keyframe's own features plus noise with descriptors a few bits off, decoys,
exact duplicates, border and off-gate queries).  No GPU, no orbx import."""
import ctypes
import functools

import numpy as np

import native
from native import KEYPOINT_DTYPE, ROOT, ptr as _ptr  # noqa: F401

KF_QUERY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("radius", "<f4"), ("level", "<i4"),
                           ("desc", "<i4")])
INT_MAX = 2 ** 31 - 1
NLEVELS = 8
W, H = 640, 480
COLS, ROWS = 64, 48


class Frame(ctypes.Structure):  # kfw_frame == orbx_kf_frame
    _fields_ = [("n", ctypes.c_int), ("keys", ctypes.c_void_p), ("desc", ctypes.c_void_p),
                ("min_x", ctypes.c_float), ("min_y", ctypes.c_float),
                ("grid_w_inv", ctypes.c_float), ("grid_h_inv", ctypes.c_float)]


@functools.lru_cache(maxsize=None)
def ref_lib():
    lib = native.ref_lib("kfwindow_ref.c")
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.kfw_grid_create.restype, lib.kfw_grid_create.argtypes = vp, [vp]
    lib.kfw_grid_free.restype, lib.kfw_grid_free.argtypes = None, [vp]
    lib.kfw_search_grid.restype, lib.kfw_search_grid.argtypes = None, [vp, vp, ci, vp, vp, vp, vp]
    lib.kfw_search.restype, lib.kfw_search.argtypes = None, [vp, vp, ci, vp, vp, vp, vp]
    lib.kfw_grid_cell_of.restype, lib.kfw_grid_cell_of.argtypes = None, [vp, ci, vp]
    lib.kfw_descriptor_distance.restype, lib.kfw_descriptor_distance.argtypes = ci, [vp, vp]
    return lib


def _struct(k, keep):
    keys = np.ascontiguousarray(k["keys"], KEYPOINT_DTYPE)
    desc = np.ascontiguousarray(k["desc"], np.uint8).reshape(-1, 32)
    keep.extend([keys, desc])
    return Frame(len(keys), _ptr(keys), _ptr(desc), k["min_x"], k["min_y"], k["grid_w_inv"],
                 k["grid_h_inv"])


STAT_NAMES = ("visited", "boxed", "gated", "at_best", "lower_loser")


def ref_search(kf, queries, qdesc):
    """The restatement on one keyframe: (best_idx int32[nq], best_dist
    int32[nq], stats dict of int32[nq]: cell entries visited, indices.size(),
    candidates past the gate, gated candidates at the best distance, whether a
    tied loser has a lower index than the winner)."""
    keep = []
    f = _struct(kf, keep)
    q = np.ascontiguousarray(queries, KF_QUERY_DTYPE).reshape(-1)
    qd = np.ascontiguousarray(qdesc, np.uint8).reshape(-1, 32)
    nq = len(q)
    bi = np.full(max(nq, 1), -7, np.int32)
    bd = np.full(max(nq, 1), -7, np.int32)
    st = np.zeros((max(nq, 1), 5), np.int32)
    ref_lib().kfw_search(ctypes.byref(f), _ptr(q), nq, _ptr(qd), _ptr(bi), _ptr(bd), _ptr(st))
    return bi[:nq].copy(), bd[:nq].copy(), {n: st[:nq, i].copy() for i, n in enumerate(STAT_NAMES)}


def ref_cells(kf):
    """(ix, iy, position in the cell) of every feature, -1s outside the grid"""
    keep = []
    f = _struct(kf, keep)
    lib = ref_lib()
    g = lib.kfw_grid_create(ctypes.byref(f))
    out = np.zeros((f.n, 3), np.int32)
    for i in range(f.n):
        lib.kfw_grid_cell_of(g, i, _ptr(out[i]))
    lib.kfw_grid_free(g)
    return out


def ref_batch(kfs, queries, qdesc):
    return [ref_search(k, q, qdesc) for k, q in zip(kfs, queries)]


# --------------------------------------------------------------------------- planted inputs
def scale_factors():
    """mvScaleFactors of ORBextractor(.., 1.2, 8, ..) (float arithmetic)"""
    sf = np.ones(NLEVELS, np.float32)
    for i in range(1, NLEVELS):
        sf[i] = np.float32(sf[i - 1] * np.float32(1.2))
    return sf


def flip(rng, d, k):
    d = d.copy()
    for b in rng.choice(256, size=k, replace=False):
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def frame_dict(keys, desc, width=W, height=H):
    """mnMinX = mnMinY = 0 and the grid constants of Frame.cc:80-81"""
    return dict(keys=np.ascontiguousarray(keys, KEYPOINT_DTYPE),
                desc=np.ascontiguousarray(desc, np.uint8).reshape(-1, 32), min_x=0.0, min_y=0.0,
                grid_w_inv=float(np.float32(COLS) / np.float32(width)),
                grid_h_inv=float(np.float32(ROWS) / np.float32(height)))


def make_keys(xs, ys, octaves):
    k = np.zeros(len(xs), KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"] = xs, ys, octaves
    k["size"], k["angle"], k["class_id"] = 31.0, 0.0, -1
    return k


def make_frame(rng, n, xmax=W, dup=0.15):
    """n features over [-8, xmax + 8) x [-8, H + 8) (a few outside the grid),
    every octave; a share `dup` of them repeats an earlier feature's
    descriptor and octave 0.5 to 9 px away from it: equal distances to any
    query, in the same cell, in a later row or in another column."""
    xs = rng.uniform(-8.0, xmax + 8.0, n).astype(np.float32)
    ys = rng.uniform(-8.0, H + 8.0, n).astype(np.float32)
    octv = rng.randint(0, NLEVELS, n).astype(np.int32)
    if n >= NLEVELS:
        octv[rng.permutation(n)[:NLEVELS]] = np.arange(NLEVELS)
    desc = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    for i in range(1, n):
        if rng.uniform() < dup:
            j = int(rng.randint(i))
            xs[i] = xs[j] + np.float32(rng.choice([-1, 1]) * rng.uniform(0.5, 9.0))
            ys[i] = ys[j] + np.float32(rng.uniform(-3.0, 3.0))
            octv[i], desc[i] = octv[j], desc[j]
    return frame_dict(make_keys(xs, ys, octv), desc)


def make_queries(rng, kf, nq, th=3.0, levels=None, border=0.1):
    """nq queries into kf and their descriptors (row i belongs to query i):
    by draw a feature's own projection plus noise with 0 to 8 bits flipped, at
    its octave or the one above (in the gate) or three above (a non-empty
    window whose every feature fails the gate); a decoy at a feature's place
    with a random descriptor; a random place; or a place within the radius of
    an image edge or beyond it.  `levels`: half of the queries draw their level
    from this list instead (-1 = no gate)."""
    sf = scale_factors()
    n = len(kf["keys"])
    q = np.zeros(nq, KF_QUERY_DTYPE)
    qd = rng.randint(0, 256, (nq, 32)).astype(np.uint8)
    for i in range(nq):
        r = rng.uniform()
        level = int(rng.randint(0, NLEVELS))
        x, y = rng.uniform(0, W), rng.uniform(0, H)
        if r < border or n == 0:
            side = int(rng.randint(4))
            off = rng.uniform(-12.0, 12.0)
            if side == 0:
                x = off
            elif side == 1:
                x = W + off
            elif side == 2:
                y = off
            else:
                y = H + off
        elif r < 0.8:
            g = int(rng.randint(n))
            k = kf["keys"][g]
            o = int(k["octave"])
            u = rng.uniform()
            level = o if u < 0.45 else min(o + 1, NLEVELS - 1) if u < 0.8 else min(o + 3, NLEVELS - 1) \
                if u < 0.93 else -1
            s = 0.8 * float(sf[max(level, 0)])
            x, y = float(k["x"]) + rng.normal(0, s), float(k["y"]) + rng.normal(0, s)
            if rng.uniform() < 0.85:
                qd[i] = flip(rng, kf["desc"][g], int(rng.randint(0, 9)))
        if levels is not None and rng.uniform() < 0.5:
            level = int(levels[int(rng.randint(len(levels)))])
        q[i] = (x, y, np.float32(th) * sf[max(level, 0)], level, i)
    return q, qd


def vacuity(kf, bi, bd, st):
    """what the GPU cases assert on the restatement before they compare"""
    nq = max(len(bi), 1)
    return dict(matched=float((bd <= 50).sum()) / nq,
                tied=int((st["at_best"] >= 2).sum()),
                tied_lower=int((st["lower_loser"] > 0).sum()),
                gate_empty=int(((st["boxed"] > 0) & (st["gated"] == 0)).sum()),
                window_empty=int((st["boxed"] == 0).sum()),
                octaves=sorted(set(kf["keys"]["octave"].tolist())))


def assert_not_vacuous(kf, bi, bd, st):
    v = vacuity(kf, bi, bd, st)
    assert 0.2 <= v["matched"] <= 0.9, v
    assert v["tied"] > 0 and v["tied_lower"] > 0, v
    assert v["gate_empty"] > 0 and v["window_empty"] > 0, v
    assert v["octaves"] == list(range(NLEVELS)), v
    assert ((bi == -1) == (bd == INT_MAX)).all()
    return v


def brute_force(kf, q, qd):
    """GetFeaturesInArea + the gate + the first strict minimum, without a
    grid: every feature the grid holds is a candidate, in the visiting order
    (ix, iy, index) of its own cell; the cell bounds only prune"""
    keys = kf["keys"]
    f32 = np.float32
    wi, hi = f32(kf["grid_w_inv"]), f32(kf["grid_h_inv"])
    mx, my = f32(kf["min_x"]), f32(kf["min_y"])
    def c_round(v):  # round(): halves away from zero (exact in double)
        v = v.astype(np.float64)
        return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5)).astype(np.int64)

    px = c_round((keys["x"] - mx) * wi)
    py = c_round((keys["y"] - my) * hi)
    ingrid = (px >= 0) & (px < COLS) & (py >= 0) & (py < ROWS)
    order = [i for i in np.lexsort((np.arange(len(keys)), py, px)) if ingrid[i]]
    bi = np.full(len(q), -1, np.int32)
    bd = np.full(len(q), INT_MAX, np.int32)
    for j in range(len(q)):
        x, y, r, level = f32(q["x"][j]), f32(q["y"][j]), f32(q["radius"][j]), int(q["level"][j])
        x0 = max(0, int(np.floor((x - mx - r) * wi)))
        x1 = min(COLS - 1, int(np.ceil((x - mx + r) * wi)))
        y0 = max(0, int(np.floor((y - my - r) * hi)))
        y1 = min(ROWS - 1, int(np.ceil((y - my + r) * hi)))
        if x0 >= COLS or x1 < 0 or y0 >= ROWS or y1 < 0:
            continue
        for i in order:
            if not (x0 <= px[i] <= x1 and y0 <= py[i] <= y1):
                continue
            if not (abs(f32(keys["x"][i]) - x) < r and abs(f32(keys["y"][i]) - y) < r):
                continue
            o = int(keys["octave"][i])
            if level >= 0 and (o < level - 1 or o > level):
                continue
            d = int(np.unpackbits(kf["desc"][i] ^ qd[q["desc"][j]]).sum())
            if d < bd[j]:
                bd[j], bi[j] = d, i
    return bi, bd
