"""Corners per FAST strip of one frame (CPU: the oracle's pyramid levels + numpy).

k_fast_strips chooses a strip's post-pass by the number of corners the strip
holds at t_lo = min(iniThFAST, minThFAST) before NMS (0 / 1..64 / more; DESIGN.md
§4 round 7).  This tool restates the planner's strips (plan_geometry in
csrc/geometry.cpp: bands of one cell row, cells grouped up to ORBX_STRIP_MAXW)
and counts those corners per strip with a numpy FAST strength, so the mix can
be read off without a GPU:

    python tools/fast_strip_stats.py --workload c4 --kind pan --frame 10

Also imported by tests/test_fast_sparse_strips.py (strip_corner_counts).
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "orb-slam-system_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

EDGE, MINB, STRIP_MAXW = 19, 16, 256  # orbx_internal.h: ORBX_EDGE, ORBX_MINB, ORBX_STRIP_MAXW

# cv::FAST's 16-point circle, (dx, dy) from (0, 3) clockwise
CIRCLE = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3),
          (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]

WORKLOADS = {  # bench.py's extraction shapes
    "c1": dict(W=640, H=480, nfeatures=1000, nlevels=8, guard="strict"),
    "c2": dict(W=640, H=480, nfeatures=1000, nlevels=1, guard="strict"),
    "c4": dict(W=1920, H=1080, nfeatures=2000, nlevels=8, guard="empty"),
    "c5": dict(W=1241, H=376, nfeatures=2000, nlevels=8, guard="strict"),
}


def fast_strength(img):
    """A[y, x] = the largest t + 1 for which (x, y) is a FAST-9 corner at
    threshold t (cv's cornerScore + 1; 0 = no corner at any t >= 0, and in the
    3-px border): a pixel is a corner at threshold t iff A > t."""
    img = np.asarray(img, np.int16)
    h, w = img.shape
    out = np.zeros((h, w), np.int16)
    if h < 7 or w < 7:
        return out.astype(np.uint8)
    v = img[3:h - 3, 3:w - 3]
    d = np.stack([img[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] - v for dx, dy in CIRCLE])

    def arc9(x):  # max over the 16 arcs of the minimum of 9 contiguous points
        m2 = np.minimum(x, np.roll(x, -1, 0))
        m4 = np.minimum(m2, np.roll(m2, -2, 0))
        m8 = np.minimum(m4, np.roll(m4, -4, 0))
        return np.minimum(m8, np.roll(x, -8, 0)).max(0)

    out[3:h - 3, 3:w - 3] = np.maximum(np.maximum(arc9(d), arc9(-d)), 0)
    return out.astype(np.uint8)


def level_strips(w, h):
    """The planner's strips of a w x h level: dicts with the band rows [y0, y1)
    and columns [x0, x1) (level coordinates), wcell and the cells' column
    ranges; cells are the reference's grid (ORBextractor.cc:298-340)."""
    maxbx, maxby = w - EDGE + 3, h - EDGE + 3
    wf, hf = np.float32(maxbx - MINB), np.float32(maxby - MINB)
    ncols, nrows = int(wf / np.float32(30)), int(hf / np.float32(30))
    if ncols <= 0 or nrows <= 0:
        return []
    wcell = int(np.ceil(wf / np.float32(ncols)))
    hcell = int(np.ceil(hf / np.float32(nrows)))
    strips = []
    for i in range(nrows):
        ry = MINB + i * hcell
        rh = min(ry + hcell + 6, maxby) - ry
        cells = []
        for j in range(ncols):
            rx = MINB + j * wcell
            rw = min(rx + wcell + 6, maxbx) - rx
            if rw < 7 or rh < 7:
                continue
            cells.append((rx + 3, rx + rw - 3))
        per = max(1, STRIP_MAXW // max(wcell, 1))
        for j0 in range(0, len(cells), per):
            cs = cells[j0:j0 + per]
            strips.append(dict(y0=ry + 3, y1=ry + rh - 3, x0=cs[0][0], x1=cs[-1][1], wcell=wcell, cells=cs))
    return strips


def unique_levels(levels):
    """drops a level that repeats the previous one's size (the extractor aliases it)"""
    out = []
    for lv in levels:
        if not out or out[-1].shape != lv.shape:
            out.append(lv)
    return out


def strip_corner_counts(levels, t_lo):
    """corners (A > t_lo, before NMS) per strip, over the given level images"""
    counts = []
    for lv in levels:
        a = fast_strength(lv) > t_lo
        for s in level_strips(lv.shape[1], lv.shape[0]):
            counts.append(int(a[s["y0"]:s["y1"], s["x0"]:s["x1"]].sum()))
    return np.array(counts, np.int64)


def report(counts):
    n = len(counts)
    pct = lambda q: int(np.percentile(counts, q)) if n else 0
    share = lambda m: 100.0 * float(m.sum()) / max(n, 1)
    dense = counts > 64
    return dict(strips=n, waves=4 * n, corners=int(counts.sum()), mean=round(float(counts.mean()), 1) if n else 0.0,
                median=pct(50), p90=pct(90), p99=pct(99), max=int(counts.max()) if n else 0,
                pct_empty=round(share(counts == 0), 1), pct_1_64=round(share((counts > 0) & ~dense), 1),
                pct_over_64=round(share(dense), 1),
                pct_corners_in_over_64=round(100.0 * float(counts[dense].sum()) / max(int(counts.sum()), 1), 1))


def main():
    from oracle import oracle as O
    from orbx import synth
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--workload", choices=sorted(WORKLOADS), default="c4")
    ap.add_argument("--kind", choices=["pan", "noise", "rects", "flat"], default="pan")
    ap.add_argument("--frame", type=int, default=10)
    ap.add_argument("--ini", type=int, default=20)
    ap.add_argument("--min", type=int, default=7)
    a = ap.parse_args()
    wl = WORKLOADS[a.workload]
    O.build()
    ex = O.Extractor(wl["nfeatures"], 1.2, wl["nlevels"], a.ini, a.min, cell_guard=wl["guard"])
    ex.extract(synth.frame(wl["W"], wl["H"], a.frame, a.kind))
    levels = unique_levels([ex.level(l) for l in range(wl["nlevels"])])
    r = report(strip_corner_counts(levels, min(a.ini, a.min)))
    print("%s %s frame %d, t_lo %d, %d unique levels: %s" % (a.workload, a.kind, a.frame, min(a.ini, a.min),
                                                              len(levels), r))


if __name__ == "__main__":
    main()
