"""Shared by the stereo matcher tests (Frame::ComputeStereoMatches,
Frame.cc:446-620): a plain numpy/Python restatement with a branch census,
the mirror of the launch width of k_stereo_match, and planted frames that
reach the branches natural synthetic pairs never take.  No GPU, no orbx
import.

restate() follows the reference statement by statement: np.float32 where the
reference has `float`, Python floats (doubles) only for `uL-0.01`, exact
integers for the Hamming distances and the SADs (cv::norm(NORM_L1) of two
centred float patches of integers is an exact integer below 2^24).

Two branches of the reference are unreachable and are neither planted nor
tested:

* `deltaR < -1 || deltaR > 1`, and a NaN deltaR.  The best incR is the first
  minimum in incR order under a strict `<`, so for an interior minimum
  dist1 > dist2 <= dist3: the denominator 2 * (dist1 + dist3 - 2 * dist2) is
  positive and |dist1 - dist3| is at most half of it, |deltaR| <= 0.5.
* Portrait frames extract no keypoints (nIni == 0 in the quadtree, as in the
  reference), so a portrait pair only reaches the matcher with planted
  keypoints; planted_tall() is the only portrait frame here.
"""
import functools
import math

import numpy as np

from native import KEYPOINT_DTYPE  # noqa: F401

F = np.float32
TH_HIGH, TH_LOW = 100, 50
W, H, NF, NLEVELS = 640, 480, 1000, 8  # every planted frame but the tall one
FX, BF = 435.2, 386.1448
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)

CENSUS_KEYS = ("empty_row", "maxu_neg", "cand_over_64", "cand_over_128", "ham_tie_at_best",
               "best_75_99", "at_minu", "at_maxu", "sad_entered", "iniu_endu_skip", "incr_minus_l",
               "incr_plus_l", "disp_neg", "disp_ge_maxd", "disp_zero_clamp", "kept_level0",
               "kept_level_up", "nd")


class StereoRangeError(IndexError):
    """the reference would index vRowIndices / its tables out of range, or
    cv::Mat::rowRange / colRange would assert"""


# --------------------------------------------------------------------------- launch width
def stereo_waves(kcap, nfeatures, nframes):
    """sw of splan_launch (csrc/api_stereo.hip): the wavefronts k_stereo_match
    spreads over one frame's left keypoints.  test_stereo_planted.py pins the
    constants and both expressions to the source."""
    waves = max(4, min(kcap, nfeatures + 256))
    return min(waves, max((waves + 3) // 4, (16384 + nframes - 1) // nframes))


def stereo_iterations(nl, kcap, nfeatures, nframes):
    """loop iterations of the wave that owns left keypoint 0: the stride is
    gridDim.x * 4 with gridDim.x = (sw + 3) / 4 blocks of four waves"""
    stride = (stereo_waves(kcap, nfeatures, nframes) + 3) // 4 * 4
    return (nl + stride - 1) // stride


def scan_chunk(nrows):
    """rows per thread of stereo_block_scan (k_stereo_rows, 1024 threads)"""
    return (nrows + 1023) // 1024


# --------------------------------------------------------------------------- restatement
def _roundf(x):
    """C round() on a float: halves away from zero (exact in double)"""
    x = float(x)
    return F(math.copysign(math.floor(abs(x) + 0.5), x))


def sad_profile(IL, strip):
    """vDists of :558-572 as exact integers: the centred 11 x 11 left window
    against the 11 windows of the centred 11 x 21 right strip"""
    a = IL.astype(np.int64) - int(IL[5, 5])
    out = []
    for k in range(11):
        b = strip[:, k:k + 11].astype(np.int64)
        out.append(int(np.abs(a - (b - b[5, 5])).sum()))
    return out


def restate(kl, dl, kr, dr, scale, inv_scale, lpyr, rpyr, mb, mbf):
    """Frame.cc:446-620 on one rectified pair.  Returns (mvuRight f32[N],
    mvDepth f32[N], kept, census): census counts the branches taken
    (CENSUS_KEYS), and holds `median` / `median_bin` (None without a match),
    `max_sad` (largest SAD entering the median), `max_kept_sad` (largest
    surviving it, -1 if none) and `per_kp`, one word per left keypoint."""
    kl = np.ascontiguousarray(kl, KEYPOINT_DTYPE)
    kr = np.ascontiguousarray(kr, KEYPOINT_DTYPE)
    dl = np.ascontiguousarray(dl, np.uint8).reshape(-1, 32)
    dr = np.ascontiguousarray(dr, np.uint8).reshape(-1, 32)
    scale = np.asarray(scale, F)
    inv_scale = np.asarray(inv_scale, F)
    nlevels = len(scale)
    N = len(kl)
    uright = np.full(N, -1.0, F)
    depth = np.full(N, -1.0, F)
    cs = dict.fromkeys(CENSUS_KEYS, 0)
    per_kp = [""] * N
    th_orb = (TH_HIGH + TH_LOW) // 2
    nrows = lpyr[0].shape[0]

    rows = [[] for _ in range(nrows)]
    for iR in range(len(kr)):
        o = int(kr["octave"][iR])
        if o < 0 or o >= nlevels:
            raise StereoRangeError("right octave %d" % o)
        y = F(kr["y"][iR])
        r = F(2.0) * scale[o]
        maxr, minr = math.ceil(float(y + r)), math.floor(float(y - r))
        if minr < 0 or maxr >= nrows:
            raise StereoRangeError("right keypoint %d spans rows %d..%d" % (iR, minr, maxr))
        for yi in range(minr, maxr + 1):
            rows[yi].append(iR)
    rx, ro = kr["x"].astype(F), kr["octave"].astype(np.int64)

    min_d = F(0)
    max_d = F(mbf) / F(mb)
    dist_idx = []  # (SAD, iL)
    for iL in range(N):
        level = int(kl["octave"][iL])
        vL, uL = F(kl["y"][iL]), F(kl["x"][iL])
        if not vL >= 0 or int(vL) >= nrows:
            raise StereoRangeError("left keypoint %d on row %r" % (iL, vL))
        cand = rows[int(vL)]
        if not cand:
            cs["empty_row"] += 1
            per_kp[iL] = "empty_row"
            continue
        min_u, max_u = uL - max_d, uL - min_d
        if max_u < 0:
            cs["maxu_neg"] += 1
            per_kp[iL] = "maxu_neg"
            continue
        cs["cand_over_64"] += len(cand) > 64
        cs["cand_over_128"] += len(cand) > 128
        c = np.array(cand, np.int64)
        gate = (ro[c] >= level - 1) & (ro[c] <= level + 1) & (rx[c] >= min_u) & (rx[c] <= max_u)
        g = c[gate]  # ascending iR
        cs["at_minu"] += int((rx[g] == min_u).sum())
        cs["at_maxu"] += int((rx[g] == max_u).sum())
        best_dist, best_r = TH_HIGH, 0
        if len(g):
            d = _POP[dl[iL][None, :] ^ dr[g]].sum(axis=1)
            j = int(np.argmin(d))  # the first of equal distances: strict '<'
            if d[j] < best_dist:
                best_dist, best_r = int(d[j]), int(g[j])
                cs["ham_tie_at_best"] += int((d == d[j]).sum()) > 1
        if best_dist >= th_orb:
            cs["best_75_99"] += best_dist < TH_HIGH
            per_kp[iL] = "hamming_%d" % best_dist
            continue
        if level < 0 or level >= nlevels:
            raise StereoRangeError("left octave %d" % level)
        cs["sad_entered"] += 1
        sf = inv_scale[level]
        su, sv, sr = _roundf(uL * sf), _roundf(vL * sf), _roundf(rx[best_r] * sf)
        w = L = 5
        li, ri = lpyr[level], rpyr[level]
        rows_l, cols_l = li.shape
        y0, xl0 = int(sv) - w, int(su) - w
        if y0 < 0 or y0 + 2 * w + 1 > rows_l or xl0 < 0 or xl0 + 2 * w + 1 > cols_l:
            raise StereoRangeError("left window of keypoint %d" % iL)
        IL = li[y0:y0 + 2 * w + 1, xl0:xl0 + 2 * w + 1]
        iniu = sr + F(L) - F(w)
        endu = sr + F(L) + F(w) + F(1)
        if iniu < 0 or endu >= ri.shape[1]:
            cs["iniu_endu_skip"] += 1
            per_kp[iL] = "iniu_endu_skip"
            continue
        xr0 = int(sr) - L - w
        if xr0 < 0 or xr0 + 2 * (L + w) + 1 > ri.shape[1]:
            raise StereoRangeError("right window of keypoint %d" % iL)
        v = sad_profile(IL, ri[y0:y0 + 2 * w + 1, xr0:xr0 + 2 * (L + w) + 1])
        k = int(np.argmin(v))  # first minimum in incR order
        best_sad, inc = v[k], k - L
        if inc == -L or inc == L:
            cs["incr_minus_l" if inc < 0 else "incr_plus_l"] += 1
            per_kp[iL] = "incr_edge"
            continue
        d1, d2, d3 = F(v[k - 1]), F(v[k]), F(v[k + 1])
        delta = (d1 - d3) / (F(2.0) * (d1 + d3 - F(2.0) * d2))
        if delta < -1 or delta > 1:  # unreachable, see the module docstring
            per_kp[iL] = "delta"
            continue
        best_u = scale[level] * (sr + F(inc) + delta)
        disparity = uL - best_u
        if not (disparity >= min_d and disparity < max_d):
            cs["disp_neg" if disparity < min_d else "disp_ge_maxd"] += 1
            per_kp[iL] = "disparity_gate"
            continue
        if disparity <= 0:
            cs["disp_zero_clamp"] += 1
            disparity = F(0.01)
            best_u = F(float(uL) - 0.01)  # the double literal of :597
        depth[iL] = F(mbf) / disparity
        uright[iL] = best_u
        dist_idx.append((best_sad, iL))
        per_kp[iL] = "match"

    nd = len(dist_idx)
    cs["nd"] = nd
    cs["median"] = cs["median_bin"] = None
    cs["max_sad"] = cs["max_kept_sad"] = -1
    kept = nd
    if nd:
        dist_idx.sort()
        median = F(dist_idx[nd // 2][0])
        th = F(1.5) * F(1.4) * median
        cs["median"] = dist_idx[nd // 2][0]
        cs["median_bin"] = dist_idx[nd // 2][0] >> 8
        cs["max_sad"] = dist_idx[-1][0]
        for s, iL in dist_idx:
            if F(s) < th:
                cs["max_kept_sad"] = max(cs["max_kept_sad"], s)
                cs["kept_level0" if kl["octave"][iL] == 0 else "kept_level_up"] += 1
            else:
                uright[iL] = depth[iL] = -1
                per_kp[iL] = "median_dropped"
                kept -= 1
    cs["per_kp"] = per_kp
    return uright, depth, kept, cs


# --------------------------------------------------------------------------- planted frames
class _Planter:
    """a constant-128 image pair, patches stamped at level 0, keypoints and
    32-byte descriptors of our choosing"""

    def __init__(self, seed, w=W, h=H):
        self.rng = np.random.default_rng(seed)
        self.L = np.full((h, w), 128, np.uint8)
        self.R = np.full((h, w), 128, np.uint8)
        self.k = ([], [])
        self.d = ([], [])

    def desc(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def flipped(self, d, nbits):
        bits = np.unpackbits(d)
        bits[self.rng.choice(256, nbits, replace=False)] ^= 1
        return np.packbits(bits)

    def key(self, side, x, y, d, octave=0):
        self.k[side].append((x, y, 31.0, 0.0, 50.0, octave, -1))
        self.d[side].append(np.asarray(d, np.uint8))
        return len(self.k[side]) - 1

    def stamp(self, img, x, y, patch):
        ph, pw = patch.shape
        y0, x0 = y - ph // 2, x - pw // 2
        assert 0 <= y0 and y0 + ph <= img.shape[0] and 0 <= x0 and x0 + pw <= img.shape[1]
        img[y0:y0 + ph, x0:x0 + pw] = patch

    def texture(self, h, w):
        return self.rng.integers(64, 192, (h, w)).astype(np.uint8)

    def strip_for(self, T, sad):
        """a 21-wide right strip whose centre window is T with single pixels
        raised until the SAD at incR = 0 is exactly `sad`; the other windows
        are unrelated texture (SADs in the thousands)"""
        strip = self.texture(11, 21)
        strip[:, 5:16] = T
        left, p = sad, 0
        while left > 0:
            r, c = divmod(p, 11)
            p += 1
            if (r, c) == (5, 5):
                continue
            step = min(left, 50)
            strip[r, 5 + c] += step
            left -= step
        v = sad_profile(T, strip)
        assert v[5] == sad and min(v[:5] + v[6:]) > max(4 * sad, 2000), v
        return strip

    def pair(self, xl, y, disp, sad=0, dr=None, keys=True):
        """a textured match: left window T at (xl, y), right strip at
        (xl - disp, y), one descriptor for both unless dr is given"""
        T = self.texture(11, 11)
        self.stamp(self.L, xl, y, T)
        self.stamp(self.R, xl - disp, y, self.strip_for(T, sad))
        if not keys:
            return T
        d = self.desc()
        iL = self.key(0, float(xl), float(y), d)
        self.key(1, float(xl - disp), float(y), d if dr is None else dr(d))
        return iL

    def mirror(self, x, y):
        """case (a): one 33-wide patch, mirror-symmetric about column x, in
        both images at the same place: SAD 0 at incR 0, equal SADs at +-k, so
        deltaR == 0 and the disparity is exactly 0"""
        half = self.texture(11, 17)
        P = np.concatenate([half[:, :0:-1], half], axis=1)
        assert P.shape == (11, 33) and np.array_equal(P, P[:, ::-1])
        self.stamp(self.L, x, y, P)
        self.stamp(self.R, x, y, P)
        d = self.desc()
        self.key(1, float(x), float(y), d)
        return self.key(0, float(x), float(y), d)

    def extreme_patch(self, kind, p=0.9):
        """case (b): an independent left window and right strip of pixels
        from {0, 255}, and their best SAD.  kind 0: left 255 with
        probability p around a centre 0, right 0 with probability p around
        centres 255; kind 1: the reverse.  Every packed byte pair sits at 0,
        255 or 510; the SAD grows with p (near 50000 at 0.9).  kind 2: fair
        coins everywhere (near 14000).  Redrawn until the first minimum is
        interior."""
        while True:
            if kind == 2:
                T = self.rng.choice(np.array([0, 255], np.uint8), (11, 11))
                S = self.rng.choice(np.array([0, 255], np.uint8), (11, 21))
            else:
                hi = (self.rng.random((11, 11)) < p, self.rng.random((11, 21)) < 1 - p)
                T = np.where(hi[0] ^ (kind == 1), 255, 0).astype(np.uint8)
                S = np.where(hi[1] ^ (kind == 1), 255, 0).astype(np.uint8)
                T[5, 5] = 0 if kind == 0 else 255
                S[5, 5:16] = 255 if kind == 0 else 0
            v = sad_profile(T, S)
            if 0 < int(np.argmin(v)) < 10:
                return T, S, min(v)

    def extreme(self, xl, y, disp, T, S):
        self.stamp(self.L, xl, y, T)
        self.stamp(self.R, xl - disp, y, S)
        d = self.desc()
        self.key(1, float(xl - disp), float(y), d)
        return self.key(0, float(xl), float(y), d)

    def region(self, x0, x1, y0, y1, disp, block=4):
        """a large blocky texture, the right one `disp` px to the left: it
        survives the pyramid's resampling, for keypoints above level 0"""
        bh, bw = (y1 - y0 + block - 1) // block, (x1 - x0 + block - 1) // block
        t = np.kron(self.rng.integers(40, 216, (bh, bw)), np.ones((block, block), np.int64))
        t = t[:y1 - y0, :x1 - x0].astype(np.uint8)
        self.L[y0:y1, x0:x1] = t
        self.R[y0:y1, x0 - disp:x1 - disp] = t

    def finish(self, name, mb=BF / FX, mbf=BF, **extra):
        def arr(side):
            k = np.array(self.k[side], KEYPOINT_DTYPE).reshape(-1)
            d = np.array(self.d[side], np.uint8).reshape(-1, 32)
            return k, d
        kl, dl = arr(0)
        kr, dr = arr(1)
        out = dict(name=name, L=self.L, R=self.R, kl=kl, dl=dl, kr=kr, dr=dr, mb=mb, mbf=mbf,
                   nf=NF, guard="strict")
        out.update(extra)
        return out


def _median_frame(name, seed, sads):
    """case (e): one textured match per entry of `sads`, planted in a shuffled
    order so the SAD order is not the keypoint order"""
    p = _Planter(seed)
    order = p.rng.permutation(len(sads))
    idx = {}
    for slot, j in enumerate(order):
        idx[int(j)] = p.pair(120 + 60 * (slot % 8), 24 + 24 * slot, 20, sads[j])
    return p.finish(name, sads=list(sads), left_of=[idx[j] for j in range(len(sads))])


def case_a_only():
    # four disparity-0 matches and nothing else: median 0, thDist 0, all dropped
    p = _Planter(101)
    for j in range(4):
        p.mirror(100 + 120 * j, 40 + 90 * j)
    return p.finish("a_only")


def case_a_kept():
    # three disparity-0 matches among six of SAD 40 (median 40: all nine
    # kept, so the clamp's values reach the output), with (c) and (d)
    p = _Planter(102)
    for j in range(3):
        p.mirror(100 + 150 * j, 30 + 40 * j)
    for j in range(4):
        p.pair(200 + 90 * j, 160 + 30 * j, 20, 40)
    d = p.desc()  # (c): endu = (W - 8) + 11 >= cols; the left window still fits
    p.key(1, float(W - 8), 300.0, d)
    c_end = p.key(0, float(W - 6), 300.0, d)
    d = p.desc()  # (c) again from the other side: iniu = -1 < 0
    p.key(1, -1.0, 330.0, d)
    c_ini = p.key(0, 10.0, 330.0, d)
    # (d): maxU = -1 < 0 on a row whose candidate (uR = -1.5 <= maxU, same
    # descriptor) would pass every gate and put the left window outside
    d = p.desc()
    p.key(1, -1.5, 360.0, d)
    d_neg = p.key(0, -1.0, 360.0, d)
    # the first skipped column: endu = (W - 11) + 11 == cols, over a texture
    # that would match were it not skipped
    c_eq = p.pair(W - 6, 390, 5, 40)
    # the last column not skipped (endu == cols - 1), in the frame's last rows
    # and columns, and the first (iniu == 10: the strip starts at column 0)
    # in its first: both windows end on the frame's edge
    last = p.pair(W - 6, H - 6, 6, 40)
    first = p.pair(30, 5, 20, 40)
    return p.finish("a_kept", c_end=c_end, c_ini=c_ini, d_neg=d_neg, c_eq=c_eq,
                    corners=(first, last))


def case_b():
    # ten {0, 255} matches: 4 + 3 of the two high kinds, 3 fair ones
    p = _Planter(103)
    for j, kind in enumerate((0, 2, 1, 0, 1, 2, 0, 1, 2, 0)):
        p.extreme(100 + 50 * j, 30 + 44 * j, 20, *p.extreme_patch(kind)[:2])
    return p.finish("b")


def case_b_mid():
    """A median at or above 0x8000 can drop nothing (2.1 * 0x8000 is past the
    largest SAD, 121 * 510), so case (b) pins the select's upper range only
    loosely.  Here the median m sits in a histogram bin >= 94 and SADs from a
    pool of {0, 255} patches straddle thDist = 2.1f * m (bins near 200): four
    fair patches below m, m, the pool's last SAD below thDist, its first at
    or above, and two more above.  One rank off either way changes the kept
    set: from m's lower neighbour the threshold falls below all the upper
    four, from its upper neighbour nothing is dropped."""
    p = _Planter(107)
    pool = sorted((p.extreme_patch(j % 2, 0.40 + 0.55 * (j // 2) / 119)[::-1] + (j,)
                   for j in range(240)), key=lambda e: (e[0], e[3]))
    sads = [e[0] for e in pool]
    mi = next(i for i, s in enumerate(sads) if s >= 95 * 256)
    th = F(1.5) * F(1.4) * F(sads[mi])
    hi = next(i for i, s in enumerate(sads) if not F(s) < th)
    assert sads[mi] < 121 * 510 / 2.2 and mi < hi - 1 and hi + 1 < len(pool) - 1
    low = [p.extreme_patch(2)[::-1] for _ in range(4)]
    assert max(e[0] for e in low) < sads[mi] / 1.5
    chosen = low + [pool[i] for i in (mi, hi - 1, hi, hi + 1, len(pool) - 1)]
    order = p.rng.permutation(len(chosen))
    left_of = [0] * len(chosen)
    for slot, j in enumerate(order):
        left_of[j] = p.extreme(100 + 50 * slot, 30 + 44 * slot, 20, chosen[j][2], chosen[j][1])
    return p.finish("b_mid", sads=[e[0] for e in chosen], left_of=left_of, th=float(th))


# 2.1f * 10 == 21.0f and 2.1f * 20 == 42.0f exactly (ties to even), so the
# SADs 21 and 42 below equal thDist and are dropped by `first < thDist`
CASES_E = {
    "e_one": (50,),
    "e_two": (10, 30),
    "e_equal": (40, 40, 40, 40, 40),
    "e_odd": (6, 8, 10, 10, 20, 21, 30),   # median 10, thDist 21.0: 20 stays, 21 goes
    "e_even": (5, 10, 15, 20, 41, 42),     # median 20, thDist 42.0: 41 stays, 42 goes
}


def case_e(name):
    return _median_frame(name, 200 + sorted(CASES_E).index(name), CASES_E[name])


def case_f():
    """Hamming-gate rows, maxD = mbf / mb = 40.5 exactly"""
    p = _Planter(104)
    tag = {}
    tag["ham74"] = p.pair(300, 16, 20, 12, dr=lambda d: p.flipped(d, 74))
    tag["ham75"] = p.pair(300, 40, 20, 12, dr=lambda d: p.flipped(d, 75))
    # two candidates 10 bits off, 71 indices apart in one row of 72: iR order decides
    T = p.pair(400, 70, 10, 14, keys=False)
    strip = p.strip_for(T, 9)
    p.stamp(p.R, 365, 70, strip)
    d = p.desc()
    tag["tie_lo"] = p.key(1, 390.0, 70.0, p.flipped(d, 10))
    for j in range(70):
        p.key(1, 10.0 + 9 * j, 70.0, p.desc())
    tag["tie_hi"] = p.key(1, 365.0, 70.0, p.flipped(d, 10))
    tag["tie"] = p.key(0, 400.0, 70.0, d)
    # uR == minU (459.5, which rounds to 460) and one ulp below it
    for name, y, ur in (("at_minu", 100, F(500) - F(40.5)),
                        ("below_minu", 124, np.nextafter(F(500) - F(40.5), F(-1)))):
        p.pair(500, y, 40, 16, keys=False)
        d = p.desc()
        p.key(1, float(ur), float(y), d)
        tag[name] = p.key(0, 500.0, float(y), d)
    # uR == maxU is the disparity-0 patch of (a); one ulp above is out
    tag["at_maxu"] = p.mirror(200, 150)
    p.pair(200, 180, 0, 16, keys=False)
    d = p.desc()
    p.key(1, float(np.nextafter(F(200), F(1000))), 180.0, d)
    tag["above_maxu"] = p.key(0, 200.0, 180.0, d)
    # left octave 2 in a textured region, one candidate each at octaves 0..4
    p.region(30, 330, 250, 474, 12)
    for j, o in enumerate((2, 0, 1, 3, 4)):
        d = p.desc()
        y = 282.0 + 40 * j
        p.key(1, 168.0, y, d, octave=o)
        tag["oct%d" % o] = p.key(0, 180.0, y, d, octave=2)
    return p.finish("f", mb=1.0, mbf=40.5, tag=tag)


def case_g():
    # octave-2 keypoints in a large textured region: the SAD windows come
    # from the pyramid (A.off / A.pitch), not from the frame
    p = _Planter(105)
    p.region(40, 600, 60, 420, 13)  # 13 / 1.2 px at level 2: the two sides resample differently
    for j in range(3):
        d = p.desc()
        p.key(1, 187.0 + 90 * j, 120.0 + 100 * j, d, octave=2)
        p.key(0, 200.0 + 90 * j, 120.0 + 100 * j, d, octave=2)
    return p.finish("g")


ERROR_KINDS = ("left_window", "right_window", "left_octave")


def with_error(case, kind):
    """a copy of an (e) frame (left keypoint i matches right keypoint i) whose
    first pair is moved to where the reference would assert: the left window
    leaves the level (uL = 3, candidate at 2), the right strip does (uR = 5
    matched from uL = 20), or the left octave is nlevels.  The oracle must not
    see the last one: it indexes its tables before it checks."""
    kl, kr = case["kl"].copy(), case["kr"].copy()
    assert np.array_equal(case["dl"][0], case["dr"][0])
    if kind == "left_window":
        kl["x"][0], kr["x"][0] = 3.0, 2.0
    elif kind == "right_window":
        kl["x"][0], kr["x"][0] = 20.0, 5.0
    else:
        assert kind == "left_octave"
        kl["octave"][0] = NLEVELS
    return dict(case, kl=kl, kr=kr)


PLANTED = ("a_only", "a_kept", "b", "b_mid", "e_one", "e_two", "e_equal", "e_odd", "e_even", "f",
           "g")


@functools.lru_cache(maxsize=None)
def planted(name):
    """the planted frame `name` of PLANTED (built once, do not modify)"""
    if name in CASES_E:
        return case_e(name)
    return {"a_only": case_a_only, "a_kept": case_a_kept, "b": case_b, "b_mid": case_b_mid,
            "f": case_f, "g": case_g}[name]()


TALL_W, TALL_H = 704, 2112
# 24 rows with 1..24 matches each (300 in all); the rows on both sides of the
# scan's chunk boundaries (1024 = 1024 threads x chunk 1, 2048 = x chunk 2)
# share image rows with their neighbour, so they take columns from opposite ends
TALL_ROWS = ((1023, 3, 0), (1024, 5, 1), (2047, 4, 0), (2048, 6, 1))


@functools.lru_cache(maxsize=None)
def planted_tall():
    p = _Planter(106, TALL_W, TALL_H)
    counts = [c for c in range(1, 25) if c not in (3, 4, 5, 6)]
    special = [s[0] for s in TALL_ROWS]
    free = [int(y) + (40 if min(abs(int(y) - s) for s in special) <= 16 else 0)
            for y in np.linspace(8, 2104, len(counts)).round()]
    assert all(abs(a - b) > 16 for i, a in enumerate(free + special) for b in (free + special)[:i]
               if (a, b) not in ((1024, 1023), (2048, 2047)))
    plan = [(int(y), c, 0) for y, c in zip(free, counts)] + list(TALL_ROWS)
    for j, (y, c, from_right) in enumerate(sorted(plan)):
        for k in range(c):
            col = 23 - k if from_right else k
            p.pair(40 + 28 * col, y, 20, 10 + (7 * j + k) % 11)
    return p.finish("tall", nf=2000, guard="empty", rows=sorted(r[0] for r in plan))


# --------------------------------------------------------------------------- oracle side
@functools.lru_cache(maxsize=None)
def _oracle_levels(O, key, nf, guard):
    L, R = _IMAGES[key]
    el = O.Extractor(nf, 1.2, NLEVELS, 20, 7, guard)
    er = O.Extractor(nf, 1.2, NLEVELS, 20, 7, guard)
    kl, dl = el.extract(L)
    kr, dr = er.extract(R)
    t = el.tables()
    return (kl, dl, kr, dr, t, [el.level(l) for l in range(NLEVELS)],
            [er.level(l) for l in range(NLEVELS)])


_IMAGES = {}


def oracle_pair(O, key, L, R, nf, guard="strict"):
    """(kl, dl, kr, dr, tables, left levels, right levels) of the oracle's
    extractors on the pair; cached under `key`, do not modify"""
    _IMAGES.setdefault(key, (L, R))
    return _oracle_levels(O, key, nf, guard)


def oracle_planted(O, case):
    """the oracle's (uRight, depth, kept) on a planted frame"""
    _, _, _, _, t, lp, rp = oracle_pair(O, "planted:" + case["name"], case["L"], case["R"],
                                        case["nf"], case["guard"])
    return O.compute_stereo_matches(case["kl"], case["dl"], case["kr"], case["dr"], t["scale"],
                                    t["inv_scale"], lp, rp, case["mb"], case["mbf"])


def bits_equal(a, b, what):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    if not np.array_equal(a.view(np.uint32), b.view(np.uint32)):
        bad = np.nonzero(a.view(np.uint32) != b.view(np.uint32))[0]
        raise AssertionError("%s differs at %d of %d, first %d: %r vs %r" %
                             (what, len(bad), len(a), bad[0], a[bad[0]], b[bad[0]]))
