"""k_stereo_rows / k_stereo_match / k_stereo_filter where tests/test_stereo.py
does not reach: several left keypoints per wavefront (the loop, its prefetch
and the reuse of the LDS partials), the planted frames of tests/stereo_util.py
(disparity clamp, window skips, maxU < 0, median 0, the upper histogram bins,
Hamming-gate rows, 1 / 2 / all-equal kept matches, a keypoint above level 0),
frames taller than 1024 and 2048 rows (scan chunks 2 and 3), and every source
of the error word followed by a clean call.  All against the oracle, bit for
bit on mvuRight, mvDepth and the kept count; each test first proves, from the
restatement's census or the mirror of the launch width, that it is not vacuous.
"""
import ctypes

import numpy as np
import pytest

import stereo_util as su
from orbx import synth

pytestmark = pytest.mark.gpu
MB, MBF = su.BF / su.FX, su.BF


def _extractors(gpu, L, R, nf, guard="strict"):
    el = gpu.Extractor(nf, 1.2, su.NLEVELS, 20, 7, guard)
    er = gpu.Extractor(nf, 1.2, su.NLEVELS, 20, 7, guard)
    return el, er, el.extract(L), er.extract(R)


def _capacity(gpu, ex, w, h):
    cap = ctypes.c_int(0)
    gpu._check(gpu.lib().orbx_extractor_capacity(ex._h, w, h, ctypes.byref(cap)), "capacity")
    return cap.value


def _synth(oracle, w, h, idx, nf, mb=MB, mbf=MBF, guard="strict"):
    """(L, R, oracle extraction, oracle stereo result) of a synthetic pair, cached"""
    key = ("synth", w, h, idx, nf, mb, mbf, guard)
    if key not in _synth.cache:
        L, R = synth.stereo_pair(w, h, idx)
        o = su.oracle_pair(oracle, key[:4] + (guard,), L, R, nf, guard)
        kl, dl, kr, dr, t, lp, rp = o
        res = oracle.compute_stereo_matches(kl, dl, kr, dr, t["scale"], t["inv_scale"], lp, rp, mb,
                                            mbf)
        _synth.cache[key] = (L, R, o, res)
    return _synth.cache[key]


_synth.cache = {}


def _same_keys(a, b):
    return np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _census(oracle, case):
    _, _, _, _, t, lp, rp = su.oracle_pair(oracle, "planted:" + case["name"], case["L"], case["R"],
                                           case["nf"], case["guard"])
    return su.restate(case["kl"], case["dl"], case["kr"], case["dr"], t["scale"], t["inv_scale"],
                      lp, rp, case["mb"], case["mbf"])[3]


def _assert_reaches(name, cs):
    """the branch each planted frame exists for, from the restatement's census"""
    if name == "a_only":
        assert cs["nd"] >= 3 and cs["median"] == 0 and cs["disp_zero_clamp"] >= 3
    elif name == "a_kept":
        assert cs["disp_zero_clamp"] >= 3 and cs["kept_level0"] == 9
        assert cs["iniu_endu_skip"] >= 3 and cs["maxu_neg"] >= 1
    elif name == "b":
        assert cs["max_kept_sad"] >= 0x8000 and cs["median_bin"] >= 128
    elif name == "b_mid":
        assert cs["median_bin"] >= 94 and cs["max_kept_sad"] >= 0x8000
        assert cs["nd"] == 9 and cs["kept_level0"] == 6 and cs["max_sad"] > cs["max_kept_sad"]
    elif name in su.CASES_E:
        sads = su.CASES_E[name]
        assert cs["nd"] == len(sads) and cs["median"] == sorted(sads)[len(sads) // 2]
        kept = cs["kept_level0"]
        assert kept == {"e_one": 1, "e_two": 2, "e_equal": 5, "e_odd": 5, "e_even": 5}[name]
    elif name == "f":
        assert cs["best_75_99"] and cs["cand_over_64"] and cs["ham_tie_at_best"]
        assert cs["at_minu"] and cs["at_maxu"] and cs["kept_level_up"] >= 3
    elif name == "g":
        assert cs["kept_level_up"] == 3
    else:
        raise AssertionError(name)


# --------------------------------------------------------------------------- the strided loop
def test_strided_loop_dropin(gpu, oracle):
    w, h, nf = 640, 480, 1000
    L, R, (kl, dl, kr, dr, t, lp, rp), _ = _synth(oracle, w, h, 2, nf, su.BF / 435.2)
    el, er, (gkl, gdl), (gkr, gdr) = _extractors(gpu, L, R, nf)
    assert _same_keys(gkl, kl) and _same_keys(gkr, kr)
    cap = _capacity(gpu, el, w, h)
    n = len(kl)
    nl = min(cap, 3 * n)
    # the second copy reversed: a wave's successive keypoints are different ones
    idx = np.concatenate([np.arange(n), np.arange(n)[::-1], np.arange(n)])[:nl]
    assert su.stereo_iterations(nl, cap, nf, 1) >= 3
    assert -(-nl // su.stereo_waves(cap, nf, 1)) >= 3
    kl3, dl3 = kl[idx], dl[idx]
    ur0, dep0, n0 = oracle.compute_stereo_matches(kl3, dl3, kr, dr, t["scale"], t["inv_scale"], lp,
                                                  rp, su.BF / 435.2, su.BF)
    assert n0 > 300
    ur, dep, nm = gpu.compute_stereo_matches(el, er, kl3, dl3, gkr, gdr, su.BF / 435.2, su.BF)
    assert nm == n0
    su.bits_equal(ur, ur0, "mvuRight")
    su.bits_equal(dep, dep0, "mvDepth")


def test_strided_loop_batched(gpu, oracle):
    import torch
    W, H, B, nf = 1241, 376, 32, 2000
    fx = 718.856
    ref = [_synth(oracle, W, H, 40 + j, nf, su.BF / fx) for j in range(8)]
    prm = gpu.params(nf, 1.2, su.NLEVELS, 20, 7)
    pl, pr = gpu.Plan(prm, W, H, B), gpu.Plan(prm, W, H, B)
    sp = gpu.StereoPlan(pl)
    # neighbouring frames differ: a frame-offset mix-up shows
    fl = torch.from_numpy(np.stack([ref[f % 8][0] for f in range(B)])).cuda()
    fr = torch.from_numpy(np.stack([ref[f % 8][1] for f in range(B)])).cuda()
    pl.extract(fl)
    pr.extract(fr)
    sp.match(pl, pr, fl, fr, su.BF / fx, su.BF)
    pl.check()
    pr.check()
    sp.check()
    cl = pl.counts.cpu().numpy()
    iters = [su.stereo_iterations(int(c), pl.kcap, nf, B) for c in cl]
    assert max(iters) >= 4 and min(iters) >= 2
    assert max(-(-int(c) // su.stereo_waves(pl.kcap, nf, B)) for c in cl) >= 4
    nm = sp.nmatches.cpu().numpy()
    urs, deps = sp.uright.cpu().numpy(), sp.depth.cpu().numpy()
    for f in range(B):
        (kl, _, _, _, _, _, _), (ur0, dep0, n0) = ref[f % 8][2], ref[f % 8][3]
        assert cl[f] == len(kl) and nm[f] == n0, f
        su.bits_equal(urs[f, :len(kl)], ur0, "frame %d mvuRight" % f)
        su.bits_equal(deps[f, :len(kl)], dep0, "frame %d mvDepth" % f)


# --------------------------------------------------------------------------- planted frames
@pytest.mark.parametrize("name", su.PLANTED)
def test_planted_dropin(gpu, oracle, name):
    case = su.planted(name)
    _assert_reaches(name, _census(oracle, case))
    ur0, dep0, n0 = su.oracle_planted(oracle, case)
    el, er, _, _ = _extractors(gpu, case["L"], case["R"], case["nf"])
    ur, dep, nm = gpu.compute_stereo_matches(el, er, case["kl"], case["dl"], case["kr"], case["dr"],
                                             case["mb"], case["mbf"])
    assert nm == n0
    su.bits_equal(ur, ur0, name + " mvuRight")
    su.bits_equal(dep, dep0, name + " mvDepth")


@pytest.fixture(scope="module")
def batch3(gpu):
    """left / right Plan and StereoPlan of three 640 x 480 frames"""
    prm = gpu.params(su.NF, 1.2, su.NLEVELS, 20, 7)
    pl, pr = gpu.Plan(prm, su.W, su.H, 3), gpu.Plan(prm, su.W, su.H, 3)
    return pl, pr, gpu.StereoPlan(pl)


def _match_middle(gpu, oracle, batch3, case):
    """the planted frame between synthetic pairs 2 and 3, its keypoints put in
    place of the extracted ones of slot 1: (StereoPlan, the outer frames'
    oracle records)"""
    import torch
    pl, pr, sp = batch3
    outer = [_synth(oracle, su.W, su.H, i, su.NF, case["mb"], case["mbf"]) for i in (2, 3)]
    fl = torch.from_numpy(np.stack([outer[0][0], case["L"], outer[1][0]])).cuda()
    fr = torch.from_numpy(np.stack([outer[0][1], case["R"], outer[1][1]])).cuda()
    pl.extract(fl)
    pr.extract(fr)
    pl.check()
    pr.check()
    outs = []
    for plan, k, d in ((pl, case["kl"], case["dl"]), (pr, case["kr"], case["dr"])):
        kps, desc, cnt = plan.kps.clone(), plan.desc.clone(), plan.counts.clone()
        assert len(k) <= plan.kcap
        kps[1, :len(k)] = torch.from_numpy(k.view(np.uint8).reshape(-1, 28).copy()).cuda()
        desc[1, :len(k)] = torch.from_numpy(np.ascontiguousarray(d)).cuda()
        cnt[1] = len(k)
        outs.append((kps, desc, cnt))
    sp.match(pl, pr, fl, fr, case["mb"], case["mbf"], left_out=outs[0], right_out=outs[1])
    return sp, outer, pl.counts.cpu().numpy()


def _compare_batch3(sp, outer, counts, case, planted_result):
    nm = sp.nmatches.cpu().numpy()
    urs, deps = sp.uright.cpu().numpy(), sp.depth.cpu().numpy()
    for f, rec in ((0, outer[0]), (2, outer[1])):
        kl, (ur0, dep0, n0) = rec[2][0], rec[3]
        assert counts[f] == len(kl) and nm[f] == n0, f
        su.bits_equal(urs[f, :len(kl)], ur0, "frame %d mvuRight" % f)
        su.bits_equal(deps[f, :len(kl)], dep0, "frame %d mvDepth" % f)
    ur0, dep0, n0 = planted_result
    assert nm[1] == n0
    su.bits_equal(urs[1, :len(ur0)], ur0, case["name"] + " mvuRight")
    su.bits_equal(deps[1, :len(ur0)], dep0, case["name"] + " mvDepth")


@pytest.mark.parametrize("name", su.PLANTED)
def test_planted_in_the_middle_of_a_batch(gpu, oracle, batch3, name):
    case = su.planted(name)
    _assert_reaches(name, _census(oracle, case))
    sp, outer, counts = _match_middle(gpu, oracle, batch3, case)
    sp.check()
    assert outer[0][3][2] > 0 and outer[1][3][2] > 0  # the neighbours have matches to lose
    _compare_batch3(sp, outer, counts, case, su.oracle_planted(oracle, case))


# --------------------------------------------------------------------------- tall frames
def test_tall_natural_1080p_scan_chunk_2(gpu, oracle):
    w, h, nf = 1920, 1080, 2000
    assert su.scan_chunk(h) == 2
    L, R, (kl, dl, kr, dr, t, lp, rp), (ur0, dep0, n0) = _synth(oracle, w, h, 5, nf, guard="empty")
    assert ((ur0 >= 0) & (kl["y"] >= 1024)).sum() >= 1  # matches past the first 1024 rows
    el, er, (gkl, gdl), (gkr, gdr) = _extractors(gpu, L, R, nf, "empty")
    assert _same_keys(gkl, kl) and _same_keys(gkr, kr)
    ur, dep, nm = gpu.compute_stereo_matches(el, er, gkl, gdl, gkr, gdr, MB, MBF)
    assert nm == n0
    su.bits_equal(ur, ur0, "mvuRight")
    su.bits_equal(dep, dep0, "mvDepth")


def test_tall_planted_704x2112_scan_chunk_3(gpu, oracle):
    case = su.planted_tall()
    assert case["L"].shape == (2112, 704) and su.scan_chunk(2112) == 3
    cs = _census(oracle, case)
    rows = case["kl"]["y"][[w == "match" for w in cs["per_kp"]]]
    assert {1023, 1024, 2047, 2048} <= set(rows.astype(int)) and cs["kept_level0"] == 300
    ur0, dep0, n0 = su.oracle_planted(oracle, case)
    el, er, _, _ = _extractors(gpu, case["L"], case["R"], case["nf"], case["guard"])
    ur, dep, nm = gpu.compute_stereo_matches(el, er, case["kl"], case["dl"], case["kr"], case["dr"],
                                             case["mb"], case["mbf"])
    assert nm == n0 == 300
    su.bits_equal(ur, ur0, "mvuRight")
    su.bits_equal(dep, dep0, "mvDepth")


# --------------------------------------------------------------------------- the error word
def _with_bad_pair(kl, dl, kr, dr, kind):
    """a synthetic pair's keypoints with one planted pair (or left keypoint)
    appended on row 240 that the kernels must refuse before any access"""
    d = np.arange(7, 39, dtype=np.uint8)[None, :] * 5
    left = np.zeros(1, su.KEYPOINT_DTYPE)
    right = np.zeros(1, su.KEYPOINT_DTYPE)
    left["y"] = right["y"] = 240.0
    if kind == "left_window":       # best candidate at distance 0, left window starts at x = -2
        left["x"], right["x"] = 3.0, 2.0
    elif kind == "right_window":    # iniu = 5, endu = 16: no skip; the strip starts at x = -5
        left["x"], right["x"] = 20.0, 5.0
    else:
        assert kind == "left_octave"
        left["x"], left["octave"] = 100.0, su.NLEVELS
        return np.concatenate([kl, left]), np.concatenate([dl, d]), kr, dr
    return (np.concatenate([kl, left]), np.concatenate([dl, d]), np.concatenate([kr, right]),
            np.concatenate([dr, d]))


@pytest.mark.parametrize("kind", su.ERROR_KINDS)
def test_error_then_clean_call_dropin(gpu, oracle, kind):
    w, h, nf = 640, 480, 1000
    L, R, (kl, dl, kr, dr, t, lp, rp), (ur0, dep0, n0) = _synth(oracle, w, h, 2, nf)
    el, er, (gkl, gdl), (gkr, gdr) = _extractors(gpu, L, R, nf)
    assert _same_keys(gkl, kl) and _same_keys(gkr, kr)
    bad = _with_bad_pair(kl, dl, kr, dr, kind)
    if kind != "left_octave":  # the oracle indexes its tables by the octave before it checks
        with pytest.raises(oracle.OracleError):
            oracle.compute_stereo_matches(*bad, t["scale"], t["inv_scale"], lp, rp, MB, MBF)
    with pytest.raises(gpu.OrbxError) as e:
        gpu.compute_stereo_matches(el, er, *bad, MB, MBF)
    assert e.value.code == gpu.ERR_ARG
    # the error word does not stick
    ur, dep, nm = gpu.compute_stereo_matches(el, er, gkl, gdl, gkr, gdr, MB, MBF)
    assert nm == n0 > 0
    su.bits_equal(ur, ur0, "mvuRight")
    su.bits_equal(dep, dep0, "mvDepth")


def test_error_then_clean_call_plan_check(gpu, oracle, batch3):
    case = su.planted("e_odd")
    bad = su.with_error(case, "right_window")
    with pytest.raises(oracle.OracleError):
        su.oracle_planted(oracle, bad)
    sp, _, _ = _match_middle(gpu, oracle, batch3, bad)
    with pytest.raises(gpu.OrbxError) as e:
        sp.check()
    assert e.value.code == gpu.ERR_ARG
    sp, outer, counts = _match_middle(gpu, oracle, batch3, case)
    sp.check()  # orbs_plan_check cleared the word
    _compare_batch3(sp, outer, counts, case, su.oracle_planted(oracle, case))
