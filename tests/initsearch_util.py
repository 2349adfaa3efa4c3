"""Shared by the ORBmatcher::SearchForInitialization tests: the CPU restatement
(tests/cpp/initsearch_ref.c, built once per process with gcc and loaded with
ctypes), an independent brute force in numpy and the planted frames.  No GPU,
no orbx import."""
import ctypes
import functools

import numpy as np

import native
from native import ROOT  # noqa: F401
from kfwindow_util import COLS, H, KEYPOINT_DTYPE, ROWS, W, Frame, flip, frame_dict, _ptr

TH_LOW = 50
INT_MAX = 2 ** 31 - 1
STAT_NAMES = ("accepted", "displaced", "filter_changed", "ratio_rejected", "rot_removed", "stale", "nlow")


@functools.lru_cache(maxsize=None)
def ref_lib():
    lib = native.ref_lib("initsearch_ref.c")
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.ini_search.restype = ci
    lib.ini_search.argtypes = [vp, vp, vp, vp, ci, ctypes.c_float, ci, ci, vp, vp]
    lib.ini_descriptor_distance.restype, lib.ini_descriptor_distance.argtypes = ci, [vp, vp]
    return lib


def cut_distance(nnratio):
    """the smallest bestDist2 > TH_LOW that passes the ratio test for every
    bestDist <= TH_LOW, in float arithmetic; 257 where there is none"""
    r = np.float32(nnratio)
    for d in range(TH_LOW + 1, 257):
        if np.float32(TH_LOW) < np.float32(np.float32(d) * r):
            return d
    return 257


def _struct(k, keep):
    keys = np.ascontiguousarray(k["keys"], KEYPOINT_DTYPE)
    desc = np.ascontiguousarray(k["desc"], np.uint8).reshape(-1, 32)
    keep.extend([keys, desc])
    return Frame(len(keys), _ptr(keys), _ptr(desc), k.get("min_x", 0.0), k.get("min_y", 0.0),
                 k.get("grid_w_inv", 0.0), k.get("grid_h_inv", 0.0))


def ref_search(pair, window_size=100, nnratio=0.9, check_ori=True):
    """The restatement on one pair dict(f1, f2, prev_matched, match12): (rc,
    match12, prev_matched, nmatches, stats dict of int32[n1]); the inputs are
    copied.  rc = -1 where the reference would read past F2.mvKeysUn."""
    keep = []
    f1, f2 = _struct(pair["f1"], keep), _struct(pair["f2"], keep)
    prev = np.array(pair["prev_matched"], np.float32).reshape(-1, 2)
    m12 = np.array(pair["match12"], np.int32).reshape(-1)
    assert len(prev) == f1.n and len(m12) == f1.n
    st = np.zeros((max(f1.n, 1), len(STAT_NAMES)), np.int32)
    nm = ctypes.c_int(0)
    rc = ref_lib().ini_search(ctypes.byref(f1), ctypes.byref(f2), _ptr(prev), _ptr(m12), int(window_size),
                              float(nnratio), 1 if check_ori else 0, cut_distance(nnratio), ctypes.byref(nm),
                              _ptr(st))
    return rc, m12, prev, nm.value, {n: st[:f1.n, i].copy() for i, n in enumerate(STAT_NAMES)}


# --------------------------------------------------------------------------- brute force
def _c_round(v):  # round(): halves away from zero (exact in double)
    v = np.asarray(v, np.float64)
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5)).astype(np.int64)


def brute_force(pair, window_size=100, nnratio=0.9, check_ori=True):
    """The same function without a grid: every F2 feature the grid holds is a
    candidate in the order (ix, iy, index) of its own cell, the cell bounds
    only prune; then the same walk.  (match12, prev_matched, nmatches)"""
    f32 = np.float32
    f1, f2 = pair["f1"], pair["f2"]
    k1, k2 = f1["keys"], f2["keys"]
    n1, n2 = len(k1), len(k2)
    wi, hi, mx, my = f32(f2["grid_w_inv"]), f32(f2["grid_h_inv"]), f32(f2["min_x"]), f32(f2["min_y"])
    px = _c_round((k2["x"] - mx) * wi)
    py = _c_round((k2["y"] - my) * hi)
    ingrid = (px >= 0) & (px < COLS) & (py >= 0) & (py < ROWS)
    order = [i for i in np.lexsort((np.arange(n2), py, px)) if ingrid[i]]
    prev = np.array(pair["prev_matched"], np.float32).reshape(-1, 2)
    m12 = np.array(pair["match12"], np.int32).reshape(-1)
    bits1 = np.unpackbits(np.asarray(f1["desc"], np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    bits2 = np.unpackbits(np.asarray(f2["desc"], np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    r = f32(window_size)
    ratio = f32(nnratio)
    md = [INT_MAX] * n2
    m21 = [-1] * n2
    hist = [[] for _ in range(30)]
    nm = 0
    for i1 in range(n1):
        o1 = int(k1["octave"][i1])
        if o1 > 0:
            continue
        x, y = prev[i1]
        x0 = max(0, int(np.floor((x - mx - r) * wi)))
        x1 = min(COLS - 1, int(np.ceil((x - mx + r) * wi)))
        y0 = max(0, int(np.floor((y - my - r) * hi)))
        y1 = min(ROWS - 1, int(np.ceil((y - my + r) * hi)))
        if x0 >= COLS or x1 < 0 or y0 >= ROWS or y1 < 0:
            continue
        best, best2, bidx = INT_MAX, INT_MAX, -1
        for i2 in order:
            if not (x0 <= px[i2] <= x1 and y0 <= py[i2] <= y1):
                continue
            if o1 == 0 and int(k2["octave"][i2]) != 0:
                continue
            if not (abs(f32(k2["x"][i2]) - x) < r and abs(f32(k2["y"][i2]) - y) < r):
                continue
            d = int(np.abs(bits1[i1] - bits2[i2]).sum())
            if d < md[i2]:
                if d < best:
                    best2, best, bidx = best, d, i2
                elif d < best2:
                    best2 = d
        if best <= TH_LOW and f32(best) < f32(f32(best2) * ratio):
            if m21[bidx] >= 0:
                m12[m21[bidx]] = -1
                nm -= 1
            m12[i1], m21[bidx], md[bidx] = bidx, i1, best
            nm += 1
            if check_ori:
                rot = f32(k1["angle"][i1]) - f32(k2["angle"][bidx])
                if rot < 0:
                    rot = f32(rot + f32(360.0))
                b = int(_c_round(f32(rot * f32(f32(1.0) / f32(30)))))
                hist[0 if b == 30 else b].append(i1)
    if check_ori:
        top = [(-1, 0)] * 3  # ComputeThreeMaxima: strict >, earlier bins first
        for i, h in enumerate(hist):
            s = len(h)
            for j in range(3):
                if s > top[j][1]:
                    top = top[:j] + [(i, s)] + top[j:2]
                    break
        ind = [t[0] for t in top]
        if top[1][1] < f32(0.1) * f32(top[0][1]):
            ind[1] = ind[2] = -1
        elif top[2][1] < f32(0.1) * f32(top[0][1]):
            ind[2] = -1
        for i, h in enumerate(hist):
            if i in ind:
                continue
            for i1 in h:
                if m12[i1] >= 0:
                    m12[i1] = -1
                    nm -= 1
    for i1 in range(n1):
        if 0 <= m12[i1] < n2:
            prev[i1] = (k2["x"][m12[i1]], k2["y"][m12[i1]])
    return m12, prev, nm


# --------------------------------------------------------------------------- planted frames
def make_keys(xs, ys, octaves, angles):
    k = np.zeros(len(xs), KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"], k["angle"] = xs, ys, octaves, angles
    k["size"], k["class_id"] = 31.0, -1
    return k


def make_f1(rng, n, level0=0.6, dup=0.25):
    """n features on W x H: a share `level0` at octave 0, a few at -1, the rest
    above; a share `dup` repeats an earlier row within 20 px with its octave
    and its descriptor 0 to 6 bits off (rows that contend for one F2 feature)"""
    xs = rng.uniform(5, W - 5, n).astype(np.float32)
    ys = rng.uniform(5, H - 5, n).astype(np.float32)
    u = rng.uniform(size=n)
    octv = np.where(u < level0, 0, np.where(u < level0 + 0.03, -1, rng.randint(1, 8, n))).astype(np.int32)
    ang = rng.uniform(0, 360, n).astype(np.float32)
    desc = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    for i in range(1, n):
        if rng.uniform() < dup:
            j = int(rng.randint(i))
            xs[i] = np.clip(xs[j] + rng.uniform(-20, 20), 0, W - 1)
            ys[i] = np.clip(ys[j] + rng.uniform(-20, 20), 0, H - 1)
            octv[i] = octv[j]
            desc[i] = flip(rng, desc[j], int(rng.randint(0, 7)))
    return frame_dict(make_keys(xs, ys, octv, ang), desc)


def make_f2(rng, f1, n, random_share=0.25, sigma=15.0, maxflip=70, rot=40.0, plants=()):
    """n features: copies of F1 rows, shuffled, moved by N(0, sigma) and with 0
    to maxflip bits flipped, their angle turned by `rot` (a fifth: random); a
    share `random_share` of random features; and the plants, rows of (x, y,
    octave, angle, descriptor), placed at random positions of the order"""
    k1, d1 = f1["keys"], f1["desc"]
    n1 = len(k1)
    nrand = int(round(n * random_share))
    ncopy = max(n - nrand - len(plants), 0)
    rows = []
    for j in rng.permutation(n1)[:ncopy] if n1 else []:
        a = (float(k1["angle"][j]) - rot) % 360.0 if rng.uniform() < 0.8 else rng.uniform(0, 360)
        rows.append((k1["x"][j] + rng.normal(0, sigma), k1["y"][j] + rng.normal(0, sigma), int(k1["octave"][j]),
                     a, flip(rng, d1[j], int(rng.randint(0, maxflip + 1)))))
    while len(rows) < n - len(plants):
        rows.append((rng.uniform(0, W), rng.uniform(0, H), int(rng.randint(0, 8)) if rng.uniform() < 0.5 else 0,
                     rng.uniform(0, 360), rng.randint(0, 256, 32).astype(np.uint8)))
    rows += list(plants)
    rows = [rows[i] for i in rng.permutation(len(rows))]
    keys = make_keys([np.float32(r[0]) for r in rows], [np.float32(r[1]) for r in rows], [r[2] for r in rows],
                     [np.float32(r[3]) for r in rows])
    desc = np.array([r[4] for r in rows], np.uint8).reshape(-1, 32)
    return frame_dict(keys, desc)


CLUSTERS = (7, 8, 9, 17)  # around the kernel's list length (IN_T = 8)


def plant_rows(rng, f1, ntwins=8):
    """plants for make_f2 around level-0 rows of F1 that are nobody's
    near-duplicate source: `ntwins` rows get two F2 features 3 bits off each
    (bestDist2 == bestDist: the ratio test rejects); one row per entry of
    CLUSTERS gets that many features 8 to 40 bits off (all below the cut
    distance at nnratio 0.9).  Returns (plants, twin rows, cluster rows)"""
    k1, d1 = f1["keys"], f1["desc"]
    bits = np.unpackbits(d1, axis=1).astype(np.int16)
    dist = (bits[:, None, :] != bits[None, :, :]).sum(axis=2) + 1000 * np.eye(len(k1), dtype=np.int64)
    alone = dist.min(axis=1) > 90  # neither a near-duplicate nor the source of one
    lvl0 = [i for i in range(len(k1)) if alone[i] and k1["octave"][i] == 0 and 120 < k1["x"][i] < W - 120
            and 120 < k1["y"][i] < H - 120]
    pick = [lvl0[i] for i in rng.permutation(len(lvl0))[:ntwins + len(CLUSTERS)]]
    twins, clusters = pick[:ntwins], pick[ntwins:]
    plants = []
    for i in twins:
        for _ in range(2):
            plants.append((k1["x"][i] + rng.uniform(-30, 30), k1["y"][i] + rng.uniform(-30, 30), 0,
                           float(k1["angle"][i]), flip(rng, d1[i], 3)))
    for i, c in zip(clusters, CLUSTERS):
        for _ in range(c):
            plants.append((k1["x"][i] + rng.uniform(-60, 60), k1["y"][i] + rng.uniform(-60, 60), 0,
                           float(k1["angle"][i]), flip(rng, d1[i], int(rng.randint(8, 41)))))
    return plants, twins, clusters


def first_pair(f1, f2):
    """the pair of the initializer's first search: vbPrevMatched = F1's own
    positions, vnMatches12 all -1 (Tracking.cc:316-320)"""
    k1 = f1["keys"]
    prev = np.stack([k1["x"], k1["y"]], axis=1).astype(np.float32) if len(k1) else np.zeros((0, 2), np.float32)
    return dict(f1=f1, f2=f2, prev_matched=prev, match12=np.full(len(k1), -1, np.int32))


def next_pair(pair, result, f2):
    """the next frame's pair: mvIniMatches and mvbPrevMatched carried along"""
    return dict(f1=pair["f1"], f2=f2, prev_matched=result[1].copy(), match12=result[0].copy())


SIEGE_ROWS, SIEGE_FEATS = 9, 10


def add_siege(rng, f1, f2, x, y):
    """A row whose every listed candidate is held by a closer row when the walk
    reaches it.  Appended to F2: features c0..c9 around (x, y) at distances 1,
    2, .., 9 and 12 from a descriptor B (c_i = B with its first i + 1 bits
    flipped, c9 with 12).  Appended to F1: rows r0..r7 with exactly c0..c7's
    descriptors, then R with B.  Each r_i takes c_i at distance 0; R's eight
    smallest candidates are c0..c7, all held at 0, so its answer (c8 at 9,
    second best 12) lies beyond any list of eight.  Returns (f1, f2, R)."""
    B = rng.randint(0, 256, 32).astype(np.uint8)

    def first_bits(k):
        d = B.copy()
        for b in range(k):
            d[b >> 3] ^= np.uint8(1 << (b & 7))
        return d

    dc = [first_bits(i + 1) for i in range(9)] + [first_bits(12)]
    kc = make_keys(x + rng.uniform(-10, 10, 10), y + rng.uniform(-10, 10, 10), np.zeros(10, np.int32),
                   np.zeros(10, np.float32))
    kr = make_keys(x + rng.uniform(-3, 3, 9), y + rng.uniform(-3, 3, 9), np.zeros(9, np.int32),
                   np.zeros(9, np.float32))
    dr = dc[:8] + [B]
    g1 = frame_dict(np.concatenate([f1["keys"], kr]), np.concatenate([f1["desc"], np.array(dr, np.uint8)]))
    g2 = frame_dict(np.concatenate([f2["keys"], kc]), np.concatenate([f2["desc"], np.array(dc, np.uint8)]))
    return g1, g2, len(g1["keys"]) - 1


def planted_pair(seed, n1=300, n2=300, siege=False, **kw):
    """(pair, twin rows, cluster rows[, the siege's last row]) of n1 x n2
    features, the siege's rows and features included"""
    rng = np.random.RandomState(seed)
    f1 = make_f1(rng, n1 - (SIEGE_ROWS if siege else 0))
    plants, twins, clusters = plant_rows(rng, f1)
    f2 = make_f2(rng, f1, n2 - (SIEGE_FEATS if siege else 0), plants=plants, **kw)
    if siege:
        f1, f2, last = add_siege(rng, f1, f2, 60.0, 60.0)
        return first_pair(f1, f2), twins, clusters, last
    return first_pair(f1, f2), twins, clusters


def summary(st, n1):
    return dict(steals=int(st["displaced"].sum()), filter_changed=int(st["filter_changed"].sum()),
                ratio_rejected=int(st["ratio_rejected"].sum()), rot_removed=int(st["rot_removed"].sum()),
                stale=int(st["stale"].sum()), accepted=int(st["accepted"].sum()), max_nlow=int(st["nlow"].max())
                if n1 else 0)
