"""Shared by the planted projection-matcher tests (frame grid +
ORBmatcher::SearchByProjection, csrc/kernels_proj.hip): synthetic frames built
directly (no extractor), descriptors at planted Hamming distances, and `model`,
a numpy restatement of the kernels' decomposition -- stable (cell, index) sort,
per-query lists of the PJ_T smallest (distance << 16 | rank) keys plus a count,
a walk over the lists, exact rescans -- with counters of the paths it took.
The oracle restates the reference loop; the model restates the kernels; the
tests require both to agree before the GPU is asked.  No GPU, no orbx import."""
import functools

import numpy as np

from native import KEYPOINT_DTYPE  # noqa: F401

PROJ_QUERY_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("radius", "<f4"), ("min_level", "<i4"),
                             ("max_level", "<i4"), ("xr", "<f4"), ("angle", "<f4")])

# mirrored from csrc/proj_internal.h and k_grid_build (test_constants_mirror_the_kernel)
PJ_T = 8
PJ_MAXN = 8192
COLS, ROWS = 64, 48
GRID_BLOCK = 1024
TH_HIGH = 100
HISTO_LENGTH = 30
INT_MAX = 2 ** 31 - 1
f32 = np.float32

# (mnMinX, mnMinY, mnMaxX, mnMaxY): an undistorted 1241x376 camera, and image
# bounds as undistortion of the corners leaves them (negative minimum)
GEOMETRIES = {"plain": (0.0, 0.0, 1241.0, 376.0), "distorted": (-31.25, -17.5, 783.5, 497.25)}

_POPCOUNT = np.array([bin(i).count("1") for i in range(256)], np.int64)


def geometry(name):
    """the grid constants as Frame computes them (src/Frame.cc:80-81), float32"""
    x0, y0, x1, y1 = (f32(v) for v in GEOMETRIES[name])
    return dict(min_x=float(x0), min_y=float(y0), max_x=float(x1), max_y=float(y1),
                grid_w_inv=float(f32(COLS) / f32(x1 - x0)), grid_h_inv=float(f32(ROWS) / f32(y1 - y0)))


def c_roundf(v):
    """roundf: halves away from zero (exact in double for float32 input)"""
    v = np.asarray(v, np.float32).astype(np.float64)
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5)).astype(np.int64)


def grid_product(g, v, axis):
    """(coordinate - minimum) * inverse cell size, as PosInGrid forms it in float32"""
    lo, inv = (g["min_x"], g["grid_w_inv"]) if axis == 0 else (g["min_y"], g["grid_h_inv"])
    return f32(f32(f32(v) - f32(lo)) * f32(inv))


def step_to_product(g, axis, t):
    """(below, at): `at` is the smallest float32 coordinate whose grid product
    is >= t, `below` the float32 before it (product < t); found by stepping"""
    lo, inv = (g["min_x"], g["grid_w_inv"]) if axis == 0 else (g["min_y"], g["grid_h_inv"])
    v = f32(t / inv + lo)
    while grid_product(g, v, axis) >= f32(t):
        v = np.nextafter(v, f32(-np.inf))
    while grid_product(g, v, axis) < f32(t):
        v = np.nextafter(v, f32(np.inf))
    below = np.nextafter(v, f32(-np.inf))
    assert grid_product(g, below, axis) < f32(t) <= grid_product(g, v, axis)
    return below, v


def cell_centre(g, axis, c):
    lo, inv = (g["min_x"], g["grid_w_inv"]) if axis == 0 else (g["min_y"], g["grid_h_inv"])
    return float(f32(c / inv + lo))


def plant(rng, base, d):
    """base with exactly d chosen bits flipped: Hamming distance d to base"""
    out = base.copy()
    for b in rng.choice(256, size=int(d), replace=False):
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def hamming(descs, d):
    return _POPCOUNT[np.bitwise_xor(descs, d)].sum(axis=-1)


def make_frame(xs, ys, desc, octave=0, angle=0.0, uright=None, occupied=None, geom="plain"):
    """A frame from arrays: float32 keypoints, [n, 32] descriptors, optional
    uright (float32) and occupied (uint8), with the grid constants of `geom`."""
    n = len(xs)
    k = np.zeros(n, KEYPOINT_DTYPE)
    k["x"], k["y"] = np.asarray(xs, np.float32), np.asarray(ys, np.float32)
    k["octave"], k["angle"] = octave, np.asarray(angle, np.float32)
    k["size"], k["class_id"] = 31.0, -1
    g = geometry(geom)
    fr = dict(keys=k, desc=np.ascontiguousarray(desc, np.uint8).reshape(n, 32),
              uright=None if uright is None else np.ascontiguousarray(uright, np.float32),
              occupied=None if occupied is None else np.ascontiguousarray(occupied, np.uint8),
              min_x=g["min_x"], min_y=g["min_y"], grid_w_inv=g["grid_w_inv"], grid_h_inv=g["grid_h_inv"])
    for a in (fr["keys"], fr["desc"], fr["uright"], fr["occupied"]):
        if a is not None:
            a.flags.writeable = False
    return fr


class Scene:
    """Collects planted features and queries; build() -> (frame, q, qd)."""

    def __init__(self, geom="plain", seed=0, uright=False):
        self.geom, self.g = geom, geometry(geom)
        self.rng = np.random.default_rng(seed)
        self.with_uright = uright
        self.f, self.q = [], []
        self._site = 0

    def base(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    def near(self, base, d):
        return plant(self.rng, base, d)

    def site(self):
        """the next point of a 24 px lattice inside the image: windows of up
        to 8 px radius around different sites share no feature"""
        g = self.g
        nx = int((g["max_x"] - g["min_x"] - 48) // 24)
        ny = int((g["max_y"] - g["min_y"] - 48) // 24)
        i = self._site
        assert i < nx * ny, "scene is out of sites"
        self._site += 1
        return g["min_x"] + 24.0 + 24.0 * (i % nx), g["min_y"] + 24.0 + 24.0 * (i // nx)

    def feat(self, x, y, desc, octave=0, angle=0.0, uright=-1.0, occupied=0):
        self.f.append((f32(x), f32(y), int(octave), f32(angle), f32(uright), int(occupied), desc))
        return len(self.f) - 1

    def query(self, x, y, r, desc, levels=(-1, -1), xr=0.0, angle=0.0):
        self.q.append((f32(x), f32(y), f32(r), int(levels[0]), int(levels[1]), f32(xr), f32(angle), desc))
        return len(self.q) - 1

    def build(self):
        f, q = self.f, self.q
        occ = np.array([v[5] for v in f], np.uint8)
        fr = make_frame([v[0] for v in f], [v[1] for v in f],
                        np.array([v[6] for v in f], np.uint8).reshape(len(f), 32),
                        octave=np.array([v[2] for v in f], np.int32), angle=[v[3] for v in f],
                        uright=np.array([v[4] for v in f], np.float32) if self.with_uright else None,
                        occupied=occ if occ.any() else None, geom=self.geom)
        qs = np.zeros(len(q), PROJ_QUERY_DTYPE)
        for i, v in enumerate(q):
            qs[i] = v[:7]
        qd = np.array([v[7] for v in q], np.uint8).reshape(len(q), 32)
        qs.flags.writeable = False
        qd.flags.writeable = False
        return fr, qs, qd


# --------------------------------------------------------------------------- the path model
def grid(frame):
    """k_grid_build: (px, py, ingrid, cell_feat, rank) -- cell_feat is the
    stable sort of the in-grid features by cell (ix-major), rank its inverse"""
    k = frame["keys"]
    px = c_roundf((k["x"] - f32(frame["min_x"])) * f32(frame["grid_w_inv"]))
    py = c_roundf((k["y"] - f32(frame["min_y"])) * f32(frame["grid_h_inv"]))
    ingrid = (px >= 0) & (px < COLS) & (py >= 0) & (py < ROWS)
    idx = np.nonzero(ingrid)[0]
    cell_feat = idx[np.argsort((px * ROWS + py)[idx], kind="stable")]
    rank = np.full(len(k), -1, np.int64)
    rank[cell_feat] = np.arange(len(cell_feat))
    return px, py, ingrid, cell_feat, rank


EARLY = ("right", "left", "below", "above")  # the four early returns, in code order


def window(frame, x, y, r):
    """area_cells: (x0, x1, y0, y1), or the name of the early return taken"""
    mx, my = f32(frame["min_x"]), f32(frame["min_y"])
    wi, hi = f32(frame["grid_w_inv"]), f32(frame["grid_h_inv"])
    x, y, r = f32(x), f32(y), f32(r)
    x0 = max(int(np.floor((x - mx - r) * wi)), 0)
    if x0 >= COLS:
        return "right"
    x1 = min(int(np.ceil((x - mx + r) * wi)), COLS - 1)
    if x1 < 0:
        return "left"
    y0 = max(int(np.floor((y - my - r) * hi)), 0)
    if y0 >= ROWS:
        return "below"
    y1 = min(int(np.ceil((y - my + r) * hi)), ROWS - 1)
    if y1 < 0:
        return "above"
    return x0, x1, y0, y1


def _keyed(frame, G, Q, qd, mode, taken):
    """sorted (distance << 16 | rank) keys of query Q's keyed candidates --
    in the window's cells, past the level and box tests, not in `taken`, past
    the mode-1 stereo gate -- or the name of the early return"""
    px, py, ingrid, _, rank = G
    w = window(frame, Q["x"], Q["y"], Q["radius"])
    if isinstance(w, str):
        return w
    x0, x1, y0, y1 = w
    k = frame["keys"]
    r = f32(Q["radius"])
    m = ingrid & (px >= x0) & (px <= x1) & (py >= y0) & (py <= y1) & ~taken
    mn, mxl = int(Q["min_level"]), int(Q["max_level"])
    if mn > 0 or mxl >= 0:
        m &= k["octave"] >= mn
        if mxl >= 0:
            m &= k["octave"] <= mxl
    m &= (np.abs(k["x"] - f32(Q["x"])) < r) & (np.abs(k["y"] - f32(Q["y"])) < r)
    ur = frame.get("uright")
    if mode == 1 and ur is not None:
        m &= ~((ur > 0) & (np.abs(f32(Q["xr"]) - ur) > r))
    idx = np.nonzero(m)[0]
    return np.sort((hamming(frame["desc"][idx], qd) << 16) | rank[idx])


def rot_bin(qangle, kangle):
    """the rotation histogram bin, in float32 as the kernel forms it"""
    rot = f32(f32(qangle) - f32(kangle))
    if rot < 0:
        rot = f32(rot + f32(360.0))
    return int(c_roundf(f32(rot * f32(f32(1.0) / f32(HISTO_LENGTH))))) % HISTO_LENGTH


def three_maxima(hist):
    """the inlined ladder of k_proj_resolve: (ind1, ind2, ind3), -1 = dropped"""
    ind, mx = [-1, -1, -1], [0, 0, 0]
    for i, s in enumerate(hist):
        s = int(s)
        if s > mx[0]:
            mx, ind = [s, mx[0], mx[1]], [i, ind[0], ind[1]]
        elif s > mx[1]:
            mx, ind = [mx[0], s, mx[1]], [ind[0], i, ind[1]]
        elif s > mx[2]:
            mx[2], ind[2] = s, i
    if f32(mx[1]) < f32(0.1) * f32(mx[0]):
        ind[1] = ind[2] = -1
    elif f32(mx[2]) < f32(0.1) * f32(mx[0]):
        ind[2] = -1
    return tuple(ind)


def model(mode, frame, q, qd, nnratio=0.6, th_dist=100, check_ori=True):
    """(match int32[n], nmatches, stats).  stats: `outside` features, `path`
    per query (an EARLY name, "empty", "list", "rescan_match", "rescan_reject",
    "rescan_none"), `ncand` per query (keyed candidates unoccupied at call
    start), counters of each path, `exact_T` / `exact_T1` queries with PJ_T /
    PJ_T + 1 keyed candidates, `ratio_equal` mode-1 acceptances with
    best == nnratio * second in float32, `hist`, `kept` bins, `bin_of`."""
    n, nq = len(frame["keys"]), len(q)
    G = grid(frame)
    cell_feat = G[3]
    occ = np.zeros(n, bool) if frame.get("occupied") is None else frame["occupied"].astype(bool)
    stats = dict(outside=int((~G[2]).sum()), path=[None] * nq, ncand=np.zeros(nq, np.int64),
                 ratio_equal=0, hist=np.zeros(HISTO_LENGTH, np.int64), kept=(-1, -1, -1),
                 bin_of=np.full(n, -1, np.int64))
    lists = []
    for i in range(nq):  # k_proj_cand
        ks = _keyed(frame, G, q[i], qd[i], mode, occ)
        if isinstance(ks, str):
            stats["path"][i] = ks
            lists.append(None)
            continue
        stats["ncand"][i] = len(ks)
        lists.append(ks[:PJ_T])
    taken = occ.copy()
    match = np.full(n, -1, np.int32)
    nm = 0
    ratio = f32(nnratio)
    for i in range(nq):  # k_proj_resolve
        if lists[i] is None:
            continue
        nc = int(stats["ncand"][i])
        if nc == 0:
            stats["path"][i] = "empty"
            continue
        free = [int(k) for k in lists[i] if not taken[cell_feat[int(k) & 0xFFFF]]]
        rescan = not (len(free) >= 2 or nc <= PJ_T)
        if rescan:
            free = [int(k) for k in _keyed(frame, G, q[i], qd[i], mode, taken)[:2]]
        k1 = free[0] if free else None
        second = free[1] >> 16 if len(free) >= 2 else INT_MAX
        ok = False
        if k1 is not None:
            best = k1 >> 16
            if mode == 1:
                ok = best <= TH_HIGH and f32(best) <= ratio * f32(second)
                if ok and f32(best) == ratio * f32(second):
                    stats["ratio_equal"] += 1
            else:
                ok = best <= th_dist
        stats["path"][i] = "list" if not rescan else \
            "rescan_match" if ok else "rescan_none" if k1 is None else "rescan_reject"
        if not ok:
            continue
        idx = int(cell_feat[k1 & 0xFFFF])
        taken[idx] = True
        match[idx] = i
        nm += 1
        if mode != 1 and check_ori:
            b = rot_bin(q["angle"][i], frame["keys"]["angle"][idx])
            stats["bin_of"][idx] = b
            stats["hist"][b] += 1
    if mode != 1 and check_ori:
        kept = three_maxima(stats["hist"])
        stats["kept"] = kept
        drop = (stats["bin_of"] >= 0) & ~np.isin(stats["bin_of"], kept)
        match[drop] = -1
        nm -= int(drop.sum())
    for name in EARLY + ("empty", "list", "rescan_match", "rescan_reject", "rescan_none"):
        stats[name] = sum(1 for p in stats["path"] if p == name)
    stats["exact_T"] = int((stats["ncand"] == PJ_T).sum())
    stats["exact_T1"] = int((stats["ncand"] == PJ_T + 1).sum())
    return match, nm, stats


# --------------------------------------------------------------------------- planted cases
class Case:
    """One call: inputs, arguments, the literal answer where it can be worked
    out by hand (`expect`: feature -> query or -1) and the non-vacuity check
    on the model's stats (`check(case, stats)`)."""

    def __init__(self, mode, frame, q, qd, nnratio=0.6, th_dist=100, check_ori=False, expect=None,
                 check=None):
        self.mode, self.frame, self.q, self.qd = mode, frame, q, qd
        self.nnratio, self.th_dist, self.check_ori = nnratio, th_dist, check_ori
        self.expect, self.check = expect or {}, check

    @property
    def args(self):
        return (self.mode, self.frame, self.q, self.qd, self.nnratio, self.th_dist, self.check_ori)


_MODEL_CACHE = {}


def model_of(name):
    """model(...) of a registered case, computed once per process"""
    if name not in _MODEL_CACHE:
        _MODEL_CACHE[name] = model(*case(name).args)
    return _MODEL_CACHE[name]


def assert_reaches_its_path(name):
    """the case's non-vacuity assertion and literal answer, on the model alone"""
    c = case(name)
    m, nm, st = model_of(name)
    assert nm == int((m >= 0).sum())
    if c.check is not None:
        c.check(c, m, st)
    for feat, qi in c.expect.items():
        assert m[feat] == qi, (name, feat, int(m[feat]), qi)
    return m, nm, st


# ---- grid
def _case_grid(geom, all_outside=False):
    s = Scene(geom, seed=21)
    g = s.g
    midx, midy = (g["min_x"] + g["max_x"]) / 2, (g["min_y"] + g["max_y"]) / 2
    pos = []
    if all_outside:
        for d in (30.0, 60.0, 500.0, 3000.0):
            pos += [(g["min_x"] - d, midy), (g["max_x"] + d, midy), (midx, g["min_y"] - d),
                    (midx, g["max_y"] + d), (g["min_x"] - d, g["max_y"] + d)]
    else:
        for axis, last in ((0, COLS), (1, ROWS)):
            for t in (-0.5, 0.5, last - 1.5, last - 0.5):
                below, at = step_to_product(g, axis, t)
                for v in (np.nextafter(below, f32(-np.inf)), below, at, np.nextafter(at, f32(np.inf))):
                    pos.append((v, midy) if axis == 0 else (midx, v))
        pos += [(midx + 3.0 * i, midy + 2.0 * i) for i in range(1, 6)]  # plainly inside
    for x, y in pos:
        d = s.base()
        s.feat(x, y, d)
        s.query(x, y, 5000.0, d)

    def check(c, m, st):
        px, py, ingrid = grid(c.frame)[:3]
        assert st["outside"] >= 4 and not (m[~ingrid] >= 0).any()
        if all_outside:
            assert st["outside"] == len(m) and st["empty"] == len(c.q) and (m == -1).all()
        else:
            assert {-1, 0, 1, COLS - 1, COLS} <= set(px.tolist()), sorted(set(px.tolist()))
            assert {-1, 0, 1, ROWS - 1, ROWS} <= set(py.tolist()), sorted(set(py.tolist()))
            # every in-grid feature is its own query's best (distance 0, whole-grid window)
            assert (m[ingrid] == np.nonzero(ingrid)[0]).all()
            assert st["list"] + st["rescan_match"] + st["rescan_reject"] + st["rescan_none"] == len(c.q)
    return Case(2, *s.build(), th_dist=100, check=check)


# ---- windows
def _case_windows(geom):
    s = Scene(geom, seed=22)
    g = s.g
    midx, midy = (g["min_x"] + g["max_x"]) / 2, (g["min_y"] + g["max_y"]) / 2
    expect = {}
    for i in range(40):  # something to find if a bound were wrong
        x, y = s.site()
        s.feat(x, y, s.base())
    far = {"right": (g["max_x"] + 3000.0, midy), "left": (g["min_x"] - 3000.0, midy),
           "below": (midx, g["max_y"] + 3000.0), "above": (midx, g["min_y"] - 3000.0)}
    early = {k: s.query(x, y, 10.0, s.base()) for k, (x, y) in far.items()}
    # windows clamped at each border (and corners): a feature 12 (8) px inside
    # the border -- the last half cell is outside the grid -- and the query
    # 22 px further out with a 30 px radius
    for bx, by in ((0, None), (1, None), (None, 0), (None, 1), (0, 0), (1, 1), (0, 1), (1, 0)):
        fx = midx + 7.0 if bx is None else (g["min_x"] + 12.0 if bx == 0 else g["max_x"] - 12.0)
        fy = midy + 5.0 if by is None else (g["min_y"] + 8.0 if by == 0 else g["max_y"] - 8.0)
        qx = fx if bx is None else (fx - 22.0 if bx == 0 else fx + 22.0)
        qy = fy if by is None else (fy - 22.0 if by == 0 else fy + 22.0)
        d = s.base()
        f = s.feat(fx, fy, d)
        expect[f] = s.query(qx, qy, 30.0, s.near(d, 3))
    clamped = list(expect.values())
    # the strict box |d| < r: at equality (out) and one float32 step inside (in)
    for axis in (0, 1):
        for sign in (-1.0, 1.0):
            for inside in (False, True):
                x, y = s.site()
                x, y = float(np.floor(x)), float(np.floor(y)) + 0.5  # integers / halves: exact
                r = 7.5 if axis else 8.0
                edge = f32((y if axis else x) + sign * r)
                v = np.nextafter(edge, f32(y if axis else x)) if inside else edge
                d = s.base()
                f = s.feat(x if axis else v, v if axis else y, d)
                qi = s.query(x, y, r, d)
                expect[f] = qi if inside else -1
    # one window over the whole grid
    d = s.base()
    f = s.feat(midx + 1.0, midy + 1.0, d)
    expect[f] = s.query(midx, midy, 5000.0, d)

    def check(c, m, st):
        for k, qi in early.items():
            assert st["path"][qi] == k, (k, st["path"][qi])
        for qi in clamped:
            x0, x1, y0, y1 = window(c.frame, c.q["x"][qi], c.q["y"][qi], c.q["radius"][qi])
            assert x0 == 0 or x1 == COLS - 1 or y0 == 0 or y1 == ROWS - 1
        assert window(c.frame, *[c.q[k][-1] for k in ("x", "y", "radius")]) == (0, COLS - 1, 0, ROWS - 1)
    return Case(2, *s.build(), th_dist=100, expect=expect, check=check)


# ---- levels
LEVEL_BOUNDS = ((-1, -1), (0, -1), (0, 0), (1, -1), (3, -1), (-1, 2), (-1, 0), (2, 2), (7, 7), (5, 3))


def _case_levels(mode):
    s = Scene("plain", seed=23)
    expect = {}
    for lo, hi in LEVEL_BOUNDS:
        x, y = s.site()
        d = s.base()
        fs = [s.feat(x + 0.5 * o - 2.0, y + (o % 3) - 1.0, s.near(d, 40 - 4 * o), octave=o) for o in range(8)]
        qi = s.query(x, y, 6.0, d, levels=(lo, hi))
        check_levels = lo > 0 or hi >= 0
        allowed = [o for o in range(8) if not check_levels or (o >= lo and (hi < 0 or o <= hi))]
        for o in range(8):  # the distance falls with the octave: the highest allowed octave wins
            expect[fs[o]] = qi if allowed and o == max(allowed) else -1

    def check(c, m, st):
        assert list(st["ncand"]) == [8, 8, 1, 7, 5, 3, 1, 1, 1, 0], list(st["ncand"])
    return Case(mode, *s.build(), nnratio=1.0, th_dist=100, expect=expect, check=check)


# ---- list edges
LIST_K = (1, 2, PJ_T - 1, PJ_T, PJ_T + 1, 2 * PJ_T, 64, 65, 200)


def _case_lists(mode, variant):
    """windows of exactly k keyed candidates, each hit by k + 2 queries with
    one descriptor from places a quarter pixel apart.  variant "occupied": 5
    more features per window occupied at call start; "gated" (mode 1): 5 more
    behind the stereo gate; both at distance 0, so they would win if counted."""
    s = Scene("distorted" if variant == "occupied" else "plain", seed=24 + mode, uright=(mode == 1))
    spans = {}
    for k in LIST_K:
        x, y = s.site()
        d = s.base()
        for j in range(k):
            s.feat(x + s.rng.uniform(-2, 2), y + s.rng.uniform(-2, 2), s.near(d, s.rng.integers(0, 61)),
                   octave=j % 8, uright=(x - 5.0 if j % 3 == 0 else -1.0))
        for j in range(5 if variant != "plain" else 0):
            if variant == "occupied":
                s.feat(x + 0.25 * j, y, d, occupied=1)
            else:
                s.feat(x + 0.25 * j, y, d, uright=x - 5.0 - 3.0 - 1.0 - j)  # |xr - uright| > r = 3
        q0 = len(s.q)
        for j in range(k + 2):
            s.query(x + 0.25 * (j % 3 - 1), y + 0.25 * (j % 2), 3.0, d, xr=x - 5.0)
        spans[k] = (q0, k + 2)

    def check(c, m, st):
        for k, (q0, cnt) in spans.items():
            assert (st["ncand"][q0:q0 + cnt] == k).all(), (k, st["ncand"][q0:q0 + cnt])
            paths = st["path"][q0:q0 + cnt]
            got = sorted(int(v) for v in m if q0 <= v < q0 + cnt)
            assert got == list(range(q0, q0 + k)), (k, got)  # the first k queries take one each
            if k <= PJ_T:  # complete lists: never a rescan, the last two find them fully claimed
                assert paths == ["list"] * cnt, (k, paths)
            else:
                assert paths[k:] == ["rescan_none"] * 2, (k, paths)
                assert paths[k - 1] == "rescan_match", (k, paths)
        q0 = spans[PJ_T + 1][0]
        assert st["path"][q0:q0 + PJ_T + 3] == ["list"] * (PJ_T - 1) + ["rescan_match"] * 2 + ["rescan_none"] * 2
        assert st["rescan_match"] >= 1 and st["rescan_none"] >= 1
        assert st["exact_T"] >= 1 and st["exact_T1"] >= 1
        if c.frame["occupied"] is not None:
            assert not (m[c.frame["occupied"] > 0] >= 0).any()
    return Case(mode, *s.build(), nnratio=1.0, th_dist=100, check_ori=False, check=check)


# ---- stereo gate
def _case_stereo():
    s = Scene("plain", seed=25, uright=True)
    expect = {}
    r = 4.0

    def spot(feats, xr_off, want):
        """feats: (distance, uright offset from 50 or None=no stereo); query xr = 50 + xr_off"""
        x, y = s.site()
        d = s.base()
        ids = [s.feat(x + 0.5 * j, y, s.near(d, dist), uright=ur) for j, (dist, ur) in enumerate(feats)]
        qi = s.query(x, y, r, d, xr=xr_off)
        for j, f in enumerate(ids):
            expect[f] = qi if j == want else -1

    step_up = float(np.nextafter(f32(54.0), f32(np.inf)))
    spot([(10, -1.0)], 500.0, 0)            # no stereo: no gate however far xr is
    spot([(10, 0.0)], 500.0, 0)             # uright == 0 is "no stereo" too (> 0 test)
    spot([(10, 50.0)], 54.0, 0)             # |xr - uright| == radius: kept
    spot([(10, 50.0)], step_up, None)       # one float32 step more: dropped
    spot([(10, 50.0)], 46.0, 0)             # equality on the other side
    spot([(5, 50.0), (20, -1.0)], 60.0, 1)  # the gated feature would be the best
    spot([(10, -1.0), (12, 50.0), (40, -1.0)], 60.0, 0)  # gated second: 10 <= 0.6 * 40, not 0.6 * 12
    spot([(10, -1.0), (12, 50.0), (40, -1.0)], 52.0, None)  # same, gate open: rejected by the ratio

    def check(c, m, st):
        assert list(st["ncand"]) == [1, 1, 1, 0, 1, 1, 2, 3]
    return Case(1, *s.build(), nnratio=0.6, check=check, expect=expect)


# ---- thresholds
def ratio_pairs():
    """for nnratio = float32(0.6): (second, largest accepted best) with the
    product exactly an integer (equality) and not, computed in float32"""
    ratio = f32(0.6)
    eq = [sd for sd in range(5, 120) if float(ratio * f32(sd)) == int(ratio * f32(sd)) and
          int(ratio * f32(sd)) >= 3]
    ne = [sd for sd in range(5, 120) if sd % 5 == 0 and float(ratio * f32(sd)) != int(ratio * f32(sd))]
    out = []
    for sd in (eq[0], ne[0]):
        acc = max(b for b in range(sd + 1) if f32(b) <= ratio * f32(sd))
        out.append((sd, acc))
    return out


def _case_thr_mode1(nnratio, th_dist):
    s = Scene("plain", seed=26, uright=False)
    expect = {}

    def spot(dists, want):
        x, y = s.site()
        d = s.base()
        ids = [s.feat(x + 0.5 * j, y, s.near(d, dist)) for j, dist in enumerate(dists)]
        qi = s.query(x, y, 4.0, d)
        for j, f in enumerate(ids):
            expect[f] = qi if j == want else -1

    spot([100], 0)       # TH_HIGH inclusive, second = INT_MAX
    spot([101], None)
    spot([0, 0], 0)      # 0 <= ratio * 0
    spot([20, 20], None if nnratio < 1 else 0)
    spot([7], 0)
    n_equal = 1          # the [0, 0] spot
    if nnratio == 0.5:
        spot([30, 60], 0)
        spot([60, 30], 1)
        spot([30, 59], None)
        n_equal += 2
    else:
        assert f32(nnratio) == f32(0.6)
        (s_eq, a_eq), (s_ne, a_ne) = ratio_pairs()
        assert f32(a_eq) == f32(0.6) * f32(s_eq) and f32(a_ne) < f32(0.6) * f32(s_ne)
        spot([a_eq, s_eq], 0)
        spot([a_eq + 1, s_eq], None)
        spot([a_ne, s_ne], 0)
        spot([a_ne + 1, s_ne], None)
        n_equal += 1

    def check(c, m, st):
        assert st["ratio_equal"] == n_equal, st["ratio_equal"]
    return Case(1, *s.build(), nnratio=nnratio, th_dist=th_dist, expect=expect, check=check)


def _case_thr_mode23(mode, th):
    s = Scene("distorted", seed=27)
    expect = {}
    for dist in (th, th + 1, max(th - 1, 0)):
        if dist > 256:
            continue  # 257 differing bits do not exist: th_dist = 256 accepts every descriptor
        x, y = s.site()
        d = s.base()
        f = s.feat(x, y, s.near(d, dist))
        qi = s.query(x, y, 4.0, d)
        expect[f] = qi if dist <= th else -1
    return Case(mode, *s.build(), th_dist=th, expect=expect)


# ---- ties
def _case_ties(mode):
    s = Scene("plain", seed=28)
    g = s.g
    expect = {}
    cells = {}
    # two cells in x: the lower index sits in the later-visited cell ix + 1
    _, at = step_to_product(g, 0, 20.5)
    y = cell_centre(g, 1, 10)
    d = s.base()
    right = s.feat(float(at) + 1.0, y, s.near(d, 10))
    left = s.feat(float(at) - 1.0, y, s.near(d, 10))
    qi = s.query(float(at), y, 3.0, d)
    expect[left], expect[right] = qi, -1
    cells["x"] = (left, right)
    # two cells in y within one ix
    _, at = step_to_product(g, 1, 30.5)
    x = cell_centre(g, 0, 40)
    d = s.base()
    lower = s.feat(x, float(at) + 1.0, s.near(d, 10))
    upper = s.feat(x, float(at) - 1.0, s.near(d, 10))
    qi = s.query(x, float(at), 3.0, d)
    expect[upper], expect[lower] = qi, -1
    cells["y"] = (upper, lower)
    # one cell: the lower index wins
    x, y = cell_centre(g, 0, 50), cell_centre(g, 1, 20)
    d = s.base()
    a = s.feat(x + 0.5, y, s.near(d, 10))
    b = s.feat(x - 0.5, y, s.near(d, 10))
    qi = s.query(x, y, 3.0, d)
    expect[a], expect[b] = qi, -1
    cells["same"] = (a, b)
    # the tied best was claimed by an earlier query: the other one is taken
    x, y = cell_centre(g, 0, 10), cell_centre(g, 1, 40)
    d = s.base()
    a = s.feat(x + 0.5, y, s.near(d, 10))
    b = s.feat(x - 0.5, y, s.near(d, 10))
    c3 = s.feat(x, y + 0.5, s.near(d, 10))
    q1, q2, q3, q4 = (s.query(x, y, 3.0, d) for _ in range(4))
    expect[a], expect[b], expect[c3] = q1, q2, q3

    def check(c, m, st):
        px, py = grid(c.frame)[:2]
        l, r = cells["x"]
        assert px[l] + 1 == px[r] and py[l] == py[r] and l > r
        u, lo = cells["y"]
        assert py[u] + 1 == py[lo] and px[u] == px[lo] and u > lo
        a_, b_ = cells["same"]
        assert (px[a_], py[a_]) == (px[b_], py[b_])
        assert q4 not in m.tolist()
    return Case(mode, *s.build(), nnratio=1.0, th_dist=100, expect=expect, check=check)


# ---- rotation
ROT_CENTRE = [0.0, 30.0, 60.0, 90.0, 120.0, 150.0, 180.0, 210.0, 240.0, 270.0, 300.0, 330.0, 355.0]


def _rot_scene(s, counts, extra=()):
    """counts: bin -> matches planted at the bin's centre; extra: (qangle, kangle)
    pairs, one match each.  Returns the features by pair."""
    feats = []
    pairs = [(ROT_CENTRE[b] + 3.0, 3.0) for b, c in counts.items() for _ in range(c)] + list(extra)
    for qa, ka in pairs:
        x, y = s.site()
        d = s.base()
        f = s.feat(x, y, s.near(d, 5), angle=ka)
        qi = s.query(x, y, 4.0, d, angle=qa)
        feats.append((f, qi))
    return feats


def _case_rot_hist(mode, name, check_ori=True):
    counts, dropped = {"h11": ({0: 11, 4: 1, 9: 1}, {4, 9}), "h10": ({0: 10, 4: 1, 9: 1}, set()),
                       "tie": ({2: 5, 6: 5, 8: 3, 11: 3}, {11}), "one": ({3: 4}, set()),
                       "four": ({1: 6, 5: 4, 7: 3, 10: 2, 12: 1}, {10, 12})}[name]
    s = Scene("plain", seed=29)
    expect = {}
    feats = _rot_scene(s, counts)
    bins = [b for b, c in counts.items() for _ in range(c)]
    for (f, qi), b in zip(feats, bins):
        expect[f] = -1 if (b in dropped and check_ori and mode != 1) else qi

    def check(c, m, st):
        if mode != 1 and check_ori:
            assert {b: int(v) for b, v in enumerate(st["hist"]) if v} == counts
            assert set(counts) - set(st["kept"]) == dropped
    return Case(mode, *s.build(), nnratio=0.9, th_dist=100, check_ori=check_ori, expect=expect, check=check)


def _case_rot_none(mode):
    s = Scene("plain", seed=30)
    for _ in range(6):
        x, y = s.site()
        d = s.base()
        s.feat(x, y, s.near(d, 120), angle=10.0)
        s.query(x, y, 4.0, d, angle=200.0)

    def check(c, m, st):
        assert st["hist"].sum() == 0 and st["kept"] == (-1, -1, -1) and (m == -1).all()
    return Case(mode, *s.build(), th_dist=100, check_ori=True, check=check)


# (query angle, feature angle): rot = 0, 15, 45, 14.999999, 345, 359.99997,
# then negative differences: -15 -> 345, -315 -> 45, and one so small that
# + 360 rounds to 360.0f
ROT_EDGES = ((77.0, 77.0), (100.0, 85.0), (50.0, 5.0), (float(f32(14.999999)), 0.0), (350.0, 5.0),
             (float(f32(359.99997)), 0.0), (10.0, 25.0), (20.0, 335.0), (0.0, 1e-6))


def _case_rot_edge(mode, k):
    """ten matches at the centre of the edge pair's expected bin, the edge
    pair, and one match in each of two other bins: with the pair binned as
    expected the top count is 11 and the two others are dropped; binned
    anywhere else it is 10 and they stay."""
    qa, ka = ROT_EDGES[k]
    b = rot_bin(qa, ka)
    others = [(b + 3) % 13, (b + 6) % 13]
    s = Scene("distorted", seed=31)
    expect = {}
    feats = _rot_scene(s, {b: 10, others[0]: 1, others[1]: 1}, extra=[(qa, ka)])
    for f, qi in feats:
        expect[f] = qi
    for f, qi in feats[10:12]:
        expect[f] = -1

    def check(c, m, st):
        assert st["hist"][b] == 11 and st["kept"] == (b, -1, -1)
        assert st["bin_of"][feats[-1][0]] == b
    return Case(mode, *s.build(), th_dist=100, check_ori=True, expect=expect, check=check)


def expected_rot_bins():
    """the bins of ROT_EDGES worked out in float32, step by step"""
    factor = f32(1.0) / f32(30.0)
    out = []
    for qa, ka in ROT_EDGES:
        rot = f32(qa) - f32(ka)
        if rot < 0:
            rot = rot + f32(360.0)
        v = float(f32(rot * factor))
        out.append(int(np.floor(v + 0.5)) % 30)
    return out


# ---- sizes
SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 4096, 4097, 8191, 8192)
MODE_ARGS = {1: dict(nnratio=1.0, th_dist=100, check_ori=False), 2: dict(nnratio=0.6, th_dist=100, check_ori=True),
             3: dict(nnratio=0.6, th_dist=14, check_ori=True)}


def random_scene(n, nq, mode, seed, geom="plain", one_cell=False):
    """n random features (about one in eight outside the grid; all of them in
    one cell if one_cell), descriptors a few bits off one of two bases so that
    distances tie and half of a window is within the thresholds; nq queries around features, a share repeated so that claims
    and rescans occur, then one whole-grid query"""
    rng = np.random.default_rng(seed)
    g = geometry(geom)
    w, h = g["max_x"] - g["min_x"], g["max_y"] - g["min_y"]
    if one_cell:
        cx, cy = cell_centre(g, 0, 31), cell_centre(g, 1, 17)
        xs = cx + rng.uniform(-0.4, 0.4, n) / g["grid_w_inv"]
        ys = cy + rng.uniform(-0.4, 0.4, n) / g["grid_h_inv"]
    else:
        xs = g["min_x"] + rng.uniform(-0.07, 1.07, n) * w
        ys = g["min_y"] + rng.uniform(-0.07, 1.07, n) * h
        xs[0], ys[0] = g["min_x"] + 0.37 * w, g["min_y"] + 0.61 * h  # n = 1: a feature inside
    pool = rng.integers(0, 256, (2, 32)).astype(np.uint8)
    desc = np.array([plant(rng, pool[rng.integers(2)], rng.integers(0, 12)) for _ in range(n)], np.uint8)
    ur = np.where(rng.uniform(size=n) < 0.5, xs - rng.uniform(1, 30, n), -1.0) if mode == 1 else None
    occ = (rng.uniform(size=n) < 0.1).astype(np.uint8) if seed % 2 else None
    if occ is not None:
        occ[0] = 0
    fr = make_frame(xs, ys, desc.reshape(n, 32), octave=rng.integers(0, 8, n), angle=rng.uniform(0, 360, n),
                    uright=ur, occupied=occ, geom=geom)
    src = rng.integers(0, n, nq)
    q = np.zeros(nq + 1, PROJ_QUERY_DTYPE)
    k = fr["keys"]
    q["x"][:nq] = k["x"][src] + rng.uniform(-2, 2, nq)
    q["y"][:nq] = k["y"][src] + rng.uniform(-2, 2, nq)
    q["radius"][:nq] = np.where(rng.uniform(size=nq) < 0.5, 8.0, 25.0)
    lv = k["octave"][src]
    ch = rng.integers(0, 3, nq)
    q["min_level"][:nq] = np.where(ch == 0, -1, np.where(ch == 1, lv - 1, 0))
    q["max_level"][:nq] = np.where(ch == 0, -1, np.where(ch == 1, lv + 1, -1))
    q["xr"][:nq] = q["x"][:nq] - rng.uniform(1, 30, nq)
    q["angle"][:nq] = np.mod(k["angle"][src] + rng.normal(0, 20, nq), 360)
    qd = np.array([plant(rng, desc[i], rng.integers(0, 8)) for i in src] + [pool[0]], np.uint8).reshape(nq + 1, 32)
    # half of the queries repeat one of the first few exactly (place, radius,
    # descriptor): the same list is walked until it runs out of unclaimed entries
    rep = np.nonzero(rng.uniform(size=nq) < 0.5)[0]
    rep = rep[rep > nq // 32]
    first = rng.integers(0, nq // 32 + 1, len(rep))
    for name in ("x", "y", "radius", "xr"):
        q[name][rep] = q[name][first]
    q["min_level"][rep], q["max_level"][rep] = -1, -1
    qd[rep] = qd[first]
    q[nq] = ((g["min_x"] + g["max_x"]) / 2, (g["min_y"] + g["max_y"]) / 2, 5000.0, -1, -1, 0.0, 0.0)
    q.flags.writeable = False
    qd.flags.writeable = False
    return fr, q, qd


def _case_size(mode, n, one_cell=False, nq=300):
    geom = "distorted" if n % 2 else "plain"
    fr, q, qd = random_scene(n, nq, mode, seed=1000 + n + (7 if one_cell else 0), geom=geom, one_cell=one_cell)

    def check(c, m, st):
        assert window(c.frame, *[c.q[k][-1] for k in ("x", "y", "radius")]) == (0, COLS - 1, 0, ROWS - 1)
        assert st["ncand"][-1] <= n - st["outside"] and (m >= 0).any()
        if one_cell:
            assert st["outside"] == 0 and len(set(grid(c.frame)[4].tolist())) == n
            assert st["ncand"].max() > 7000 and st["rescan_match"] + st["rescan_reject"] >= 1
        elif n >= 63:
            assert st["outside"] >= 4 and st["list"] >= 1
            # windows of more than PJ_T candidates, hit until the list runs out
            # (under mode 3's th_dist = 14 the runs of claims are shorter: the
            # densest frames only)
            if n >= (8191 if mode == 3 else 4096):
                assert st["rescan_match"] + st["rescan_reject"] + st["rescan_none"] >= 1
    return Case(mode, fr, q, qd, check=check, **MODE_ARGS[mode])


def _case_nq(nq):
    fr, q, qd = random_scene(65, 300, 2, seed=1065, geom="distorted")
    return Case(2, fr, q[:nq], qd[:nq], **MODE_ARGS[2])


# ---- registry
def _registry():
    r = {}
    for geom in ("plain", "distorted"):
        r["grid-%s" % geom] = functools.partial(_case_grid, geom)
        r["windows-%s" % geom] = functools.partial(_case_windows, geom)
    r["grid-all-outside"] = functools.partial(_case_grid, "distorted", True)
    r["stereo-gate"] = _case_stereo
    for th in (50, 200):
        r["thr-m1-ratio0.5-th%d" % th] = functools.partial(_case_thr_mode1, 0.5, th)
    r["thr-m1-ratio0.6"] = functools.partial(_case_thr_mode1, float(f32(0.6)), 100)
    for mode in (1, 2, 3):
        r["levels-m%d" % mode] = functools.partial(_case_levels, mode)
        r["lists-m%d" % mode] = functools.partial(_case_lists, mode, "plain")
        r["lists-occupied-m%d" % mode] = functools.partial(_case_lists, mode, "occupied")
        r["ties-m%d" % mode] = functools.partial(_case_ties, mode)
    r["lists-gated-m1"] = functools.partial(_case_lists, 1, "gated")
    r["rot-h11-m1-ori"] = functools.partial(_case_rot_hist, 1, "h11", True)
    r["rot-h11-m1-noori"] = functools.partial(_case_rot_hist, 1, "h11", False)
    for mode in (2, 3):
        for th in (0, 64, 100, 256):
            r["thr-m%d-th%d" % (mode, th)] = functools.partial(_case_thr_mode23, mode, th)
        for h in ("h11", "h10", "tie", "one", "four"):
            r["rot-%s-m%d" % (h, mode)] = functools.partial(_case_rot_hist, mode, h)
        r["rot-none-m%d" % mode] = functools.partial(_case_rot_none, mode)
        for k in range(len(ROT_EDGES)):
            r["rot-edge%d-m%d" % (k, mode)] = functools.partial(_case_rot_edge, mode, k)
    for n in SIZES:
        for mode in (1, 2, 3):
            r["size-%d-m%d" % (n, mode)] = functools.partial(_case_size, mode, n)
    for mode in (1, 2, 3):
        r["size-8192-onecell-m%d" % mode] = functools.partial(_case_size, mode, 8192, True, 120)
    for nq in (1, 3, 4, 5):
        r["nq-%d" % nq] = functools.partial(_case_nq, nq)
    return r


_REGISTRY = _registry()
CASE_NAMES = tuple(_REGISTRY)


@functools.lru_cache(maxsize=None)
def case(name):
    """the named planted case, built once per process and never mutated"""
    return _REGISTRY[name]()
