"""k_fast_strips' post-pass by strip content: empty
strips only clear their cells' counts, strips with 1..64 corners are finished
by one wave in registers, the others take the four-wave row-mask form.  Frames
built here hold all three kinds of strip; the dense-strip counter proves which
path ran, and every keypoint field, descriptor byte and count equals the
oracle's under both settings of Plan.set_options(fast_post=...)."""
import functools
import os
import sys

import numpy as np
import pytest

from orbx import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import fast_strip_stats as fss  # noqa: E402  (the CPU strip model, tools/fast_strip_stats.py)

pytestmark = pytest.mark.gpu


def mixed_frame(w, h, seed):
    """flat background; the top third of the rows stays empty, the middle
    third holds isolated pixels and small squares in its right third (a few
    corners per strip), the bottom third is iid noise (hundreds of corners
    per strip) -- by rows, since a narrow level is one strip wide"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 128, np.uint8)
    a, b = h // 3, 2 * h // 3
    for _ in range(max(6, (b - a) * w // 1800)):
        x, y, s = int(rng.integers(2 * w // 3, w - 3)), int(rng.integers(a, b - 3)), int(rng.integers(1, 4))
        img[y:y + s, x:x + s] = int(rng.choice([40, 90, 160, 230]))
    img[b:] = rng.integers(0, 256, (h - b, w), dtype=np.uint8)
    return img


def blob_frame(w, h, seed):
    """flat background with isolated pixels and small squares everywhere"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), 128, np.uint8)
    for _ in range(max(8, w * h // 1500)):
        x, y, s = int(rng.integers(0, w - 3)), int(rng.integers(0, h - 3)), int(rng.integers(1, 4))
        img[y:y + s, x:x + s] = int(rng.choice([40, 90, 160, 230]))
    return img


@functools.lru_cache(maxsize=None)
def _frame(kind, w, h, seed):
    if kind == "mixed":
        return mixed_frame(w, h, seed)
    if kind == "blob":
        return blob_frame(w, h, seed)
    return synth.frame(w, h, seed, kind)  # "noise" / "flat"


_REF = {}


def _reference(oracle, kind, w, h, seed, nf, L, ini, mn, guard):
    """the oracle's keypoints, descriptors and per-strip corner counts of a
    frame, computed once per configuration"""
    key = (kind, w, h, seed, nf, L, ini, mn, guard)
    if key not in _REF:
        ex = oracle.Extractor(nf, 1.2, L, ini, mn, cell_guard=guard)
        k, d = ex.extract(_frame(kind, w, h, seed))
        levels = fss.unique_levels([ex.level(l) for l in range(L)])
        _REF[key] = (k, d, fss.strip_corner_counts(levels, min(ini, mn)))
    return _REF[key]


def _cmp(res, ref, what):
    (k, d), (rk, rd) = res, ref[:2]
    assert len(k) == len(rk), "%s: count %d vs %d" % (what, len(k), len(rk))
    for f in k.dtype.names:
        assert np.array_equal(k[f], rk[f]), "%s: field %s differs" % (what, f)
    assert np.array_equal(d, rd), "%s: descriptors differ" % what


def _extract(plan, frames, fast_post):
    import torch
    plan.set_options(fast_post=fast_post)
    plan.debug_counters()
    plan.extract(torch.from_numpy(np.ascontiguousarray(frames)).cuda())
    plan.check()
    return plan.results(len(frames)), plan.debug_counters()


# (w, h, nlevels, guard): which kernel form FAST takes there
#  800x200x3  level 0 (800 >= 400 px wide, 34-row bands, 16-B-aligned rows) on
#             the column walk, level 2 (667 wide) too (level 1 repeats level 0's
#             size and shares its strips); strips of 8
#             cells x 31 px = 254 px -> tile pitch 288, k_fast_strips_p288
#  320x240x4  every level under 400 px: block staging; 8 cells x 32 px = 262 px
#             -> pitch 288 as well (k_fast_strips_p288)
#  240x200x3  6 cells x 35 px = 216 px -> pitch 240: k_fast_strips with the
#             run-time pitch, block staging
#  500x121x3  level 0 has two cell rows of 45 band rows (> 32): block staging
#             (the column walk takes <= 32 rows) and, for the dense strips, the
#             general output form; level 2 (417x101) has 35-row bands (level 1
#             repeats level 0's size and shares its strips)
SHAPES = [(800, 200, 3, "empty"), (320, 240, 4, "strict"), (240, 200, 3, "strict"), (500, 121, 3, "empty")]


@pytest.mark.parametrize("w,h,L,guard", SHAPES)
def test_mixed_frame_both_settings(gpu, oracle, w, h, L, guard):
    ref = _reference(oracle, "mixed", w, h, 1, 1000, L, 20, 7, guard)
    cnt = ref[2]
    assert (cnt == 0).any() and ((cnt > 0) & (cnt <= 64)).any() and (cnt > 64).any(), "frame lacks a strip kind"
    plan = gpu.Plan(gpu.params(1000, 1.2, L, 20, 7, guard), w, h, 1)
    frames = _frame("mixed", w, h, 1)[None]
    res_a, c_a = _extract(plan, frames, "auto")
    res_d, c_d = _extract(plan, frames, "dense")
    _cmp(res_a[0], ref, "auto")
    _cmp(res_d[0], ref, "dense")
    assert c_d["fast_dense_strips"] == len(cnt), "dense: every strip counts"
    assert c_a["fast_dense_strips"] == int((cnt > 64).sum()), "auto: the strips with more than 64 corners"
    assert 0 < c_a["fast_dense_strips"] < c_d["fast_dense_strips"]
    # (the noise strips hold more corners than the list: they overflow it under either setting)
    assert c_a["fast_overflow_strips"] == c_d["fast_overflow_strips"] <= c_a["fast_dense_strips"]


@pytest.mark.parametrize("ini,mn", [(20, 7), (7, 7), (30, 12)])
def test_thresholds(gpu, oracle, ini, mn):
    w, h, L = 800, 200, 3
    ref = _reference(oracle, "mixed", w, h, 2, 1000, L, ini, mn, "empty")
    plan = gpu.Plan(gpu.params(1000, 1.2, L, ini, mn, "empty"), w, h, 1)
    res, c = _extract(plan, _frame("mixed", w, h, 2)[None], "auto")
    _cmp(res[0], ref, "thresholds %d / %d" % (ini, mn))
    assert c["fast_dense_strips"] == int((ref[2] > 64).sum())
    assert 0 < c["fast_dense_strips"] < len(ref[2])


def test_flat_frame(gpu, oracle):
    """no corner anywhere: every strip is empty, no keypoint, count 0"""
    w, h, L = 800, 200, 3
    plan = gpu.Plan(gpu.params(1000, 1.2, L, 20, 7, "empty"), w, h, 1)
    res, c = _extract(plan, _frame("flat", w, h, 0)[None], "auto")
    assert len(res[0][0]) == 0 and len(res[0][1]) == 0
    assert int(plan.counts[0].item()) == 0
    assert c["fast_dense_strips"] == 0


def test_no_stale_state_across_calls(gpu, oracle):
    """one plan: a noise frame (every strip dense), then a flat one (every
    strip empty), then blobs (sparse); then the three as one batch.  No count
    or key of an earlier call or of a neighbouring frame survives."""
    w, h, L = 320, 240, 4
    kinds = [("noise", 3), ("flat", 0), ("blob", 4)]
    refs = [_reference(oracle, k, w, h, s, 1000, L, 20, 7, "strict") for k, s in kinds]
    plan = gpu.Plan(gpu.params(1000, 1.2, L, 20, 7, "strict"), w, h, 3)
    for (k, s), ref in zip(kinds, refs):
        res, _ = _extract(plan, _frame(k, w, h, s)[None], "auto")
        _cmp(res[0], ref, "single %s" % k)
    assert len(refs[1][0]) == 0 and len(refs[0][0]) > 0 and len(refs[2][0]) > 0
    batch = np.stack([_frame(k, w, h, s) for k, s in kinds])
    res, c = _extract(plan, batch, "auto")
    for i, ref in enumerate(refs):
        _cmp(res[i], ref, "batch frame %d (%s)" % (i, kinds[i][0]))
    assert c["fast_dense_strips"] == sum(int((r[2] > 64).sum()) for r in refs)


def boundary_frame(w, h):
    """level-0 strips with exactly 63, 64 and 65 corners: isolated bright
    pixels 8 px apart (one FAST corner each, no two on a common circle)"""
    img = np.full((h, w), 128, np.uint8)
    strips = [s for s in fss.level_strips(w, h) if s["x1"] - s["x0"] >= 8 * 17 and s["y1"] - s["y0"] >= 8 * 3 + 1]
    for s, n in zip(strips, (63, 64, 65)):
        for i in range(n):
            img[s["y0"] + 8 * (i // 17), s["x0"] + 8 * (i % 17)] = 228
    assert len(strips) >= 3
    return img


def test_boundary_63_64_65(gpu, oracle):
    w, h, L = 800, 200, 3
    img = boundary_frame(w, h)
    ex = oracle.Extractor(1000, 1.2, L, 20, 7, cell_guard="empty")
    rk, rd = ex.extract(img)
    cnt = fss.strip_corner_counts(fss.unique_levels([ex.level(l) for l in range(L)]), 7)
    assert {63, 64, 65} <= set(cnt.tolist()), sorted(set(cnt.tolist()))
    plan = gpu.Plan(gpu.params(1000, 1.2, L, 20, 7, "empty"), w, h, 1)
    for fast_post in ("auto", "dense"):
        res, c = _extract(plan, img[None], fast_post)
        _cmp(res[0], (rk, rd), "boundary, " + fast_post)
        assert c["fast_dense_strips"] == (int((cnt > 64).sum()) if fast_post == "auto" else len(cnt))
    assert (cnt > 64).sum() >= 1


def test_corner_list_shorter_than_64(gpu, oracle):
    """with the corner list cut to 24 entries (orbx_debug_set_fast_ccap, as
    test_fast_corner_list_overflow_path) strips with 24 < nc <= 64 take the
    dense path's strength-map scan, not the sparse path"""
    w, h, L, ccap = 800, 200, 3, 24
    ref = _reference(oracle, "mixed", w, h, 1, 1000, L, 20, 7, "empty")
    cnt = ref[2]
    assert ((cnt > ccap) & (cnt <= 64)).any(), "no strip between the list length and 64"
    assert gpu.lib().orbx_debug_set_fast_ccap(ccap) == gpu.OK
    try:
        plan = gpu.Plan(gpu.params(1000, 1.2, L, 20, 7, "empty"), w, h, 1)
    finally:
        gpu.lib().orbx_debug_set_fast_ccap(-1)
    res, c = _extract(plan, _frame("mixed", w, h, 1)[None], "auto")
    _cmp(res[0], ref, "ccap %d" % ccap)
    assert c["fast_overflow_strips"] == int((cnt > ccap).sum())
    assert c["fast_dense_strips"] == int((cnt > ccap).sum())
