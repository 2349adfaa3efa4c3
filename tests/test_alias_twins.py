"""Twin rows: a keypoint that wins the quadtree both in a level and in a level
aliasing it (level 1 of the reference's scale table [1, 1, s, ...] is level
0's image) is computed once by k_orient_brief and written to both rows.

Every case holds the GPU result against the oracle on every keypoint field
and descriptor byte, and the plan option that turns the sharing off
(twins="off", ORBX_PLAN_NO_TWINS) against the default byte for byte over the
whole output buffers (rows past a frame's count included), for both BRIEF
forms.  Each case asserts from the oracle's output that the classes it is
meant to exercise are not empty.

A bounded CPU search with the oracle (640x480 and 320x240; 11 feature counts
100..3000; pan / rects / noise; frames 0, 3, 7, 11, 40; 8 and 2 levels: 660
frames) found no level-1 winner without a level-0 twin, so that class has no
case here; such a keypoint takes the unchanged compute path (it stays in the
alias level's processing order)."""
import numpy as np
import pytest

from orbx import synth

pytestmark = pytest.mark.gpu

IDX = 7
# (w, h, nfeatures, nlevels, kind, level-0 rows without a twin expected)
CASES = [
    (640, 480, 1000, 8, "pan", False),    # all twins: 282 / 314 / 256
    (640, 480, 1000, 8, "rects", False),
    (640, 480, 1000, 8, "noise", False),
    (640, 480, 300, 8, "pan", True),      # proper subset: 58 twins + 98 level-0-only / 60 + 103 / 64 + 192
    (640, 480, 300, 8, "rects", True),
    (640, 480, 300, 8, "noise", True),
    (320, 240, 200, 8, "pan", True),      # smallest shape, still mixed: 40 + 38
    (640, 480, 500, 2, "noise", True),    # the alias level is the last level: 256 + 768
]

_REF = {}


def _ref(oracle, w, h, nf, L, kind, idx=IDX, sf=1.2):
    """frame and oracle output, computed once per case and shared"""
    key = (w, h, nf, L, kind, idx, sf)
    if key not in _REF:
        img = synth.frame(w, h, idx, kind)
        k, d = oracle.Extractor(nf, sf, L, 20, 7, cell_guard="strict").extract(img)
        for a in (img, k, d):
            a.setflags(write=False)
        _REF[key] = (img, k, d)
    return _REF[key]


def _classes(k, d, u, la):
    """(twins, rows of level u without a twin, rows of level la without one):
    rows of the two levels that agree in angle, response and descriptor"""
    def rows(l):
        m = k["octave"] == l
        return set(zip(k["angle"][m].tolist(), k["response"][m].tolist(), map(bytes, d[m])))
    a, b = rows(u), rows(la)
    return len(a & b), len(a - b), len(b - a)


def _cmp_kps(a, b, what):
    assert len(a) == len(b), "%s: count %d vs %d" % (what, len(a), len(b))
    for f in a.dtype.names:
        if not np.array_equal(a[f], b[f]):
            bad = np.nonzero(a[f] != b[f])[0]
            raise AssertionError("%s: field %s differs at %d rows, first %d: %r vs %r" %
                                 (what, f, len(bad), bad[0], a[bad[0]], b[bad[0]]))


def _run(gpu, plan, frames, **opts):
    """one extraction into sentinel-filled outputs: (per-frame results, raw buffers)"""
    import torch
    B = frames.shape[0]
    plan.set_options(**opts)
    plan.kps.fill_(0xA5)
    plan.desc.fill_(0xA5)
    plan.counts.fill_(-1)
    plan.extract(torch.from_numpy(np.array(frames)).cuda())
    plan.check()
    raw = (plan.kps[:B].cpu().numpy().copy(), plan.desc[:B].cpu().numpy().copy(), plan.counts[:B].cpu().numpy().copy())
    return plan.results(B), raw


def _check_plan(gpu, plan, frames, refs, brief, what):
    res, raw = _run(gpu, plan, frames, brief=brief)
    for f, (rk, rd) in enumerate(refs):
        _cmp_kps(res[f][0], rk, "%s frame %d (%s blur)" % (what, f, brief))
        assert np.array_equal(res[f][1], rd), "%s frame %d: descriptors differ (%s blur)" % (what, f, brief)
    res_off, raw_off = _run(gpu, plan, frames, brief=brief, twins="off")
    for name, a, b in zip(("keypoints", "descriptors", "counts"), raw, raw_off):
        assert np.array_equal(a, b), "%s: %s differ between twins on and off (%s blur)" % (what, name, brief)
    # back on: the pairs' arrival counters survive the runs without them
    res_on, raw_on = _run(gpu, plan, frames, brief=brief)
    for name, a, b in zip(("keypoints", "descriptors", "counts"), raw, raw_on):
        assert np.array_equal(a, b), "%s: %s differ on a second run (%s blur)" % (what, name, brief)


@pytest.mark.parametrize("brief", ["patch", "level"])
@pytest.mark.parametrize("w,h,nf,L,kind,l0only", CASES)
def test_twin_rows_match_oracle_and_option_off(gpu, oracle, brief, w, h, nf, L, kind, l0only):
    img, rk, rd = _ref(oracle, w, h, nf, L, kind)
    tw, u_only, a_only = _classes(rk, rd, 0, 1)
    assert tw > 0, "case has no twin rows"
    assert (u_only > 0) == l0only, "level-0 rows without a twin: %d" % u_only
    plan = gpu.Plan(gpu.params(nf, 1.2, L, 20, 7, "strict"), w, h, 1)
    assert list(plan.geo.alias[:L])[:2] == [0, 0]
    _check_plan(gpu, plan, img[None], [(rk, rd)], brief, "%dx%d %d %s" % (w, h, nf, kind))


@pytest.mark.parametrize("brief", ["patch", "level"])
def test_twin_rows_batch_of_different_counts(gpu, oracle, brief):
    """four frames of one batch with different counts (one of them empty),
    extracted twice at different frame slots of the plan"""
    w, h, nf, L = 640, 480, 300, 8
    kinds = ("pan", "flat", "noise", "rects")
    refs = [_ref(oracle, w, h, nf, L, kind) for kind in kinds]
    counts = [len(r[1]) for r in refs]
    assert len(set(counts)) == len(counts) and 0 in counts, counts
    assert all(_classes(r[1], r[2], 0, 1)[0] > 0 for r in refs if len(r[1]))
    plan = gpu.Plan(gpu.params(nf, 1.2, L, 20, 7, "strict"), w, h, 4)
    frames = np.stack([r[0] for r in refs])
    _check_plan(gpu, plan, frames, [(r[1], r[2]) for r in refs], brief, "batch")
    order = [2, 0, 3]
    _check_plan(gpu, plan, frames[order], [(refs[i][1], refs[i][2]) for i in order], brief, "batch of 3")


@pytest.mark.parametrize("w,h,nf,L,kind", [c[:5] for c in CASES if c[2] in (300, 200, 500)] + [CASES[0][:5]])
def test_twin_rows_single_frame_drop_in(gpu, oracle, w, h, nf, L, kind):
    """the ORBextractor drop-in call (one frame: the wide quadtree kernel)"""
    img, rk, rd = _ref(oracle, w, h, nf, L, kind)
    assert _classes(rk, rd, 0, 1)[0] > 0
    ex = gpu.Extractor(nf, 1.2, L, 20, 7, cell_guard="strict")
    for call in range(2):
        k, d = ex.extract(img)
        _cmp_kps(k, rk, "drop-in call %d" % call)
        assert np.array_equal(d, rd), "drop-in call %d: descriptors differ" % call


@pytest.mark.parametrize("brief", ["patch", "level"])
def test_alias_pairs_above_level_0(gpu, oracle, brief):
    """scale factor 1.001 on 320x240: levels alias as [0, 0, 0, 3, 4, 4, 6, 6] --
    pairs (4, 5) and (6, 7) whose two levels differ in scale (the twin row
    takes octave, scale and size from its own level's tables), and level 2, a
    second alias of level 0, which is computed on its own"""
    w, h, nf, L, sf = 320, 240, 600, 8, 1.001
    refs = [_ref(oracle, w, h, nf, L, kind, sf=sf) for kind in ("rects", "noise", "pan")]
    plan = gpu.Plan(gpu.params(nf, sf, L, 20, 7, "strict"), w, h, 3)
    assert list(plan.geo.alias[:L]) == [0, 0, 0, 3, 4, 4, 6, 6]
    for img, rk, rd in refs:
        for u, la in ((0, 1), (4, 5), (6, 7)):
            assert _classes(rk, rd, u, la)[0] > 0, (u, la)
        m4, m5 = rk["octave"] == 4, rk["octave"] == 5
        assert m4.any() and m5.any() and not np.array_equal(rk["x"][m4][:1], rk["x"][m5][:1])
    frames = np.stack([r[0] for r in refs])
    _check_plan(gpu, plan, frames, [(r[1], r[2]) for r in refs], brief, "scale 1.001")


def test_no_alias_level_is_the_plain_path(gpu, oracle):
    """one level: no alias level, the option changes nothing, and the quadtree
    and BRIEF stages are one launch each -- as they are with an alias level"""
    import torch
    for L in (1, 8):
        w, h, nf = 640, 480, 1000
        img, rk, rd = _ref(oracle, w, h, nf, L, "rects")
        plan = gpu.Plan(gpu.params(nf, 1.2, L, 20, 7, "strict"), w, h, 2)
        if L == 1:
            assert list(plan.geo.alias[:L]) == [0]
        frames = np.stack([img, img])
        _check_plan(gpu, plan, frames, [(rk, rd), (rk, rd)], "patch", "%d level(s)" % L)
        plan.set_options()
        plan.set_timing(True)
        plan.extract(torch.from_numpy(frames).cuda())
        plan.check()
        st = plan.stage_times()
        plan.set_timing(False)
        assert st["quadtree"][1] == 1 and st["orient_brief"][1] == 1, st


@pytest.mark.parametrize("brief", ["patch", "level"])
def test_identity_order_fallback_has_no_twins(gpu, oracle, brief):
    """20 features over a noise frame: level 0 holds more keys than the
    quadtree's winner bitmap has room for (3 smax words), so the processing
    order is the identity and the pair is computed without twin rows"""
    w, h, nf, L = 640, 480, 20, 8
    img, rk, rd = _ref(oracle, w, h, nf, L, "noise")
    g = gpu.geometry(gpu.params(nf, 1.2, L, 20, 7, "strict"), w, h)
    smax = max(max(g.features[l] - 1, g.nini[l]) for l in range(L))
    r2 = _ref(oracle, w, h, nf, L, "rects")
    # the frames' level-0 key counts are at least the level-0 rows that larger
    # feature budgets keep of them (every winner is a distinct key): 1024 and
    # 314, both above the 96 smax keys the bitmap covers
    for big, kind in ((500, "noise"), (1000, "rects")):
        bk = _ref(oracle, w, h, big, 2 if big == 500 else 8, kind)[1]
        assert int((bk["octave"] == 0).sum()) > 96 * smax
    assert _classes(rk, rd, 0, 1)[0] > 0 and _classes(r2[1], r2[2], 0, 1)[0] > 0
    plan = gpu.Plan(gpu.params(nf, 1.2, L, 20, 7, "strict"), w, h, 2)
    frames = np.stack([img, r2[0]])
    _check_plan(gpu, plan, frames, [(rk, rd), (r2[1], r2[2])], brief, "identity order")


def test_twins_option_flag(gpu):
    lib = gpu.lib()
    plan = gpu.Plan(gpu.params(300, 1.2, 8, 20, 7), 320, 240, 1)
    for flags in (gpu.ORBX_PLAN_NO_TWINS, gpu.ORBX_PLAN_NO_TWINS | 8, gpu.ORBX_PLAN_NO_TWINS | 16 | 1 | 64, 0):
        assert lib.orbx_plan_set_options(plan._h, flags) == gpu.OK, flags
    for flags in (256, gpu.ORBX_PLAN_NO_TWINS | 32, gpu.ORBX_PLAN_NO_TWINS | 24):
        assert lib.orbx_plan_set_options(plan._h, flags) == gpu.ERR_ARG, flags
