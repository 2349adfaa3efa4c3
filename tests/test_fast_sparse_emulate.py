"""k_fast_strips' sparse post-pass (strips with 1..64 corners, one corner per
lane of one wave), restated in numpy and checked against the literal per-cell
procedure of ComputeKeyPointsOctTree: cv::FAST with NMS inside the cell at
iniThFAST, again at minThFAST if that left the cell empty, keypoints in raster
order.  No GPU: this pins down the selection rule the kernel implements (kept
flags at both thresholds from the 8 neighbours inside the cell, the per-cell
choice of threshold, the rank within a cell by the list entry r << 9 | c).

A strip here is its band: bh rows, the cells' bands side by side (wcell
columns each, the last cell `wlast`), strengths A in 0..255 with A = 0 where
there is no corner at t_lo = min(ini, min) (as the kernel's strength map)."""
import numpy as np
import pytest

THRESHOLDS = [(20, 7), (7, 7), (30, 12), (9, 15)]


def literal(A, wcell, ncells, ini, mn):
    """per cell: [(r, c, response)] in raster order"""
    bh, bw = A.shape
    out = []
    for k in range(ncells):
        x0, x1 = k * wcell, bw if k == ncells - 1 else (k + 1) * wcell
        cell = A[:, x0:x1].astype(np.int32)
        kept = []
        for th in (ini, mn):
            score = np.where(cell > th, cell - 1, 0)  # cornerScore of the corners at th, 0 elsewhere
            pad = np.pad(score, 1)
            nb = np.max([pad[1 + dy:1 + dy + bh, 1 + dx:1 + dx + (x1 - x0)]
                         for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy], axis=0)
            keep = (cell > th) & (score > nb)
            if keep.any():
                kept = [(int(r), int(x0 + c), int(cell[r, c] - 1)) for r, c in np.argwhere(keep)]
                break
        out.append(kept)
    return out


def sparse_path(A, wcell, ncells, ini, mn, order):
    """the kernel's sparse path: lane i holds corner `order[i]` of the list"""
    bh, bw = A.shape
    rs, cs = np.nonzero(A)
    rs, cs = rs[order], cs[order]
    n = len(rs)
    assert n <= 64
    a = A[rs, cs].astype(np.int32)
    rw = np.float32(1.0) / np.float32(wcell)
    k = np.minimum(((cs.astype(np.float32) + np.float32(0.5)) * rw).astype(np.int32), ncells - 1)
    cb0 = k * wcell
    cb1 = np.where(k == ncells - 1, bw, cb0 + wcell)
    vu, vd, vl, vr = rs > 0, rs + 1 < bh, cs > cb0, cs + 1 < cb1
    ou, od, ol, orr = vu.astype(int), vd.astype(int), vl.astype(int), vr.astype(int)
    Ai = A.astype(np.int32)
    g = lambda dr, dc: Ai[rs + dr, cs + dc]  # clamped offsets: an outside neighbour reads the centre row / column
    mx = np.maximum.reduce([np.where(vu, g(-ou, 0), 0), np.where(vd, g(od, 0), 0), np.where(vl, g(0, -ol), 0),
                            np.where(vr, g(0, orr), 0), np.where(vu & vl, g(-ou, -ol), 0),
                            np.where(vu & vr, g(-ou, orr), 0), np.where(vd & vl, g(od, -ol), 0),
                            np.where(vd & vr, g(od, orr), 0)]) if n else np.zeros(0, np.int32)
    nbm = np.where(mx > mn, mx - 1, 0)
    nbi = np.where(mx > ini, mx - 1, 0)
    ki = (a > ini) & (a - 1 > nbi)
    km = (a > mn) & (a - 1 > nbm)
    e = (rs << 9) | cs
    out = [[] for _ in range(ncells)]
    counts = np.zeros(ncells, np.int64)
    for kc in np.unique(k[ki | km]):
        same = k == kc
        sel = same & (ki if (same & ki).any() else km)
        counts[kc] = sel.sum()
        slots = [None] * int(sel.sum())
        for i in np.nonzero(sel)[0]:
            rank = int((sel & (e < e[i])).sum())
            assert slots[rank] is None
            slots[rank] = (int(rs[i]), int(cs[i]), int(a[i] - 1))
        out[kc] = slots
    return out, counts


def check(A, wcell, ncells, ini, mn, rng):
    t_lo = min(ini, mn)
    A = np.where(A > t_lo, A, 0).astype(np.uint8)
    n = int(np.count_nonzero(A))
    got, counts = sparse_path(A, wcell, ncells, ini, mn, rng.permutation(n))
    ref = literal(A, wcell, ncells, ini, mn)
    assert got == ref
    assert [len(x) for x in ref] == list(counts)
    return ref


@pytest.mark.parametrize("ini,mn", THRESHOLDS)
def test_random_strips(ini, mn):
    rng = np.random.default_rng(1000 * ini + mn)
    for trial in range(300):
        bh = int(rng.integers(1, 40))
        wcell = int(rng.integers(8, 40))
        ncells = int(rng.integers(1, 9))
        wlast = int(rng.integers(1, wcell + 7))  # narrower or wider than wcell (the planner's last cell)
        bw = (ncells - 1) * wcell + wlast
        A = np.zeros((bh, bw), np.uint8)
        n = int(rng.integers(0, 65))
        n = min(n, bh * bw)
        # clustered placement, so that neighbours (and equal neighbours) occur
        idx = set()
        while len(idx) < n:
            r, c = int(rng.integers(0, bh)), int(rng.integers(0, bw))
            for _ in range(int(rng.integers(1, 5))):
                if len(idx) < n:
                    idx.add((min(bh - 1, max(0, r + int(rng.integers(-1, 2)))),
                             min(bw - 1, max(0, c + int(rng.integers(-1, 2))))))
        for r, c in idx:
            A[r, c] = rng.choice([8, 13, 20, 21, 31, 40, int(rng.integers(1, 256))])
        check(A, wcell, ncells, ini, mn, rng)


@pytest.mark.parametrize("ini,mn", THRESHOLDS)
def test_edges_of_cell_and_band(ini, mn):
    """corners on the first / last row and column of the band and of every
    cell: a neighbour across a cell border does not suppress (the literal
    procedure runs FAST on the cell alone)"""
    rng = np.random.default_rng(5)
    bh, wcell, ncells, wlast = 12, 10, 3, 7
    bw = 2 * wcell + wlast
    A = np.zeros((bh, bw), np.uint8)
    for r in (0, bh - 1, 5):
        for c in (0, wcell - 1, wcell, 2 * wcell - 1, 2 * wcell, bw - 1):
            A[r, c] = 40 + (r + c) % 7
    A[5, wcell - 1], A[5, wcell] = 50, 90  # neighbours in different cells: both kept
    ref = check(A, wcell, ncells, ini, mn, rng)
    assert (5, wcell - 1, 49) in ref[0] and (5, wcell, 89) in ref[1]


@pytest.mark.parametrize("ini,mn", THRESHOLDS)
def test_equal_neighbours_suppress_each_other(ini, mn):
    rng = np.random.default_rng(6)
    A = np.zeros((8, 30), np.uint8)
    A[3, 4] = A[3, 5] = 60    # cell 0: adjacent, equal: neither kept -> cell empty at both thresholds
    A[2, 14] = A[3, 15] = 60  # cell 1: diagonal, equal, plus a lone corner
    A[6, 12] = 35
    ref = check(A, 10, 3, ini, mn, rng)
    assert ref[0] == [] and ref[1] == [(6, 12, 34)] and ref[2] == []


def test_cell_retried_at_min_threshold():
    """a cell whose corners all fail at 20 but pass at 7 takes the minThFAST
    flags; its neighbour cell with one corner above 20 keeps only the
    iniThFAST ones (a corner of 15 there is dropped)"""
    rng = np.random.default_rng(7)
    A = np.zeros((10, 20), np.uint8)
    A[1, 2], A[4, 6], A[8, 9] = 12, 15, 9
    A[2, 13], A[7, 17] = 33, 15
    ref = check(A, 10, 2, 20, 7, rng)
    assert ref[0] == [(1, 2, 11), (4, 6, 14), (8, 9, 8)]
    assert ref[1] == [(2, 13, 32)]
    # at the minimum threshold a neighbour between the thresholds suppresses
    A[2, 14] = 18  # fails at 20, but stronger than nothing at 20: cell 1 unchanged
    assert check(A, 10, 2, 20, 7, rng)[1] == [(2, 13, 32)]
    A[2, 13] = 16  # now cell 1 retries at 7: 18 beats its neighbour 16
    assert check(A, 10, 2, 20, 7, rng)[1] == [(2, 14, 17), (7, 17, 14)]


@pytest.mark.parametrize("wlast", [3, 10, 16])
def test_last_cell_width(wlast):
    """the strip's last cell narrower / equal / wider than wcell (the column to
    cell map clamps to the last cell)"""
    rng = np.random.default_rng(wlast)
    wcell, ncells = 10, 3
    bw = 2 * wcell + wlast
    A = np.zeros((6, bw), np.uint8)
    for c in range(0, bw, 2):
        A[(c // 2) % 6, c] = 25 + c
    ref = check(A, wcell, ncells, 20, 7, rng)
    assert sum(len(x) for x in ref) > 0 and all(c >= 2 * wcell for _, c, _ in ref[2])
