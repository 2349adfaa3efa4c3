"""Initializer's homography / fundamental RANSAC on the GPU
(csrc/kernels_initransac.hip) against the CPU restatement
(tests/cpp/initransac_ref.c): every output word bit for bit, NaNs compared as
equal, no tolerance."""
import ctypes

import numpy as np
import pytest

import initransac_util as U

pytestmark = pytest.mark.gpu

# (matches, nit): the wavefront edges of both, thinned from the full product so
# that every value of either occurs with a small and a large value of the other
GRID = ((8, 1), (8, 64), (8, 200), (9, 63), (9, 65), (63, 1), (63, 64), (64, 65), (64, 200), (65, 63), (65, 200),
        (257, 1), (257, 64), (257, 65), (257, 200),
        # the score kernel's tile of 32 matches: one short, exact, one over
        (31, 65), (32, 64), (33, 63))


def _same(got, ref, what):
    bad = U.same_result(got, ref)
    assert not bad, (what, bad, {k: (got[k], ref[k]) for k in bad if not k.startswith("inliers")})
    assert len(got["inliers_H"]) == len(got["inliers_F"]) == ref["nmatch"]


def _grid_scene(nm, nit):
    return ("planar" if (nm + nit) % 2 else "general"), nm, 3, nit


@pytest.mark.parametrize("nm,nit", GRID)
def test_size_grid(gpu, nm, nit):
    pair, _ = U.scene(*_grid_scene(nm, nit))
    ref = U.scene_ref(*_grid_scene(nm, nit))
    (got,) = gpu.initializer_ransac([pair], nit)
    assert got["nmatch"] == nm
    _same(got, ref, (nm, nit))


def _no_winner_pair(nit):
    p, _, _ = U.planted_cases()["no_winner"]
    return dict(p, sets=np.resize(p["sets"], (nit, 8)))  # its two sets in turn: neither scores for H


def test_batch_of_seven_interleaved(gpu):
    """the sizes interleaved, both scene kinds and a pair without an H winner:
    neighbouring workgroups belong to different pairs with unequal match counts,
    and each pair equals its single-pair result"""
    nit = 65
    pairs = [U.scene(k, nm, 4, nit)[0] for k, nm in (("planar", 257), ("general", 8), ("general", 65), ("planar", 9),
                                                    ("general", 64), ("planar", 63))]
    pairs.insert(3, _no_winner_pair(nit))
    refs = [U.ref_initialize(p, nit) for p in pairs]
    assert refs[3]["it_H"] == -1 and refs[3]["SH"] == 0 and not refs[3]["inliers_H"].any()
    assert sum(r["it_H"] >= 0 and r["it_F"] >= 0 for r in refs) >= 5
    got = gpu.initializer_ransac(pairs, nit)
    assert len(got) == 7
    for i, (g, r) in enumerate(zip(got, refs)):
        _same(g, r, i)
    _same(gpu.initializer_ransac([pairs[3]], nit)[0], refs[3], "no winner alone")


@pytest.mark.parametrize("name", sorted(U.planted_cases()))
def test_planted_case(gpu, name):
    pair, nit, sigma = U.planted_cases()[name]
    (got,) = gpu.initializer_ransac([pair], nit, sigma)
    _same(got, U.ref_initialize(pair, nit, sigma), name)


def test_planted_cases_in_one_batch(gpu):
    """the sigma = 1 cases that share an iteration count go into one call"""
    by_nit = {}
    for name, (pair, nit, sigma) in sorted(U.planted_cases().items()):
        if sigma == U.SIGMA and nit > 0:
            by_nit.setdefault(nit, []).append((name, pair))
    assert max(len(v) for v in by_nit.values()) >= 2
    for nit, group in by_nit.items():
        got = gpu.initializer_ransac([p for _, p in group], nit)
        for (name, p), g in zip(group, got):
            _same(g, U.ref_initialize(p, nit), name)


def test_chi_exactly_at_threshold(gpu):
    pair, nit, s_at, s_above, i = U.chi_exact_case()
    for sigma, flag in ((s_at, 1), (s_above, 0)):
        ref = U.ref_initialize(pair, nit, sigma)
        assert ref["inliers_H"][i] == flag
        (got,) = gpu.initializer_ransac([pair], nit, sigma)
        _same(got, ref, sigma)


def test_unequal_frames_and_unreferenced_keys(gpu):
    """n1 != n2 in both directions; the unmatched keys move Normalize's means"""
    for e1, e2 in ((90, 0), (0, 75)):
        pair, _ = U.scene("general", 50, 6, nit=33, extra1=e1, extra2=e2)
        assert len(pair["keys1"]) != len(pair["keys2"])
        ref = U.ref_initialize(pair, 33)
        (got,) = gpu.initializer_ransac([pair], 33)
        _same(got, ref, (e1, e2))
        # without the unreferenced keys the normalisation, and so the result, differs
        first, second = U.match_list(pair["match12"])
        bare = dict(keys1=pair["keys1"][first], keys2=pair["keys2"][second],
                    match12=np.arange(50, dtype=np.int32), sets=pair["sets"])
        assert not U.same_bits(U.ref_initialize(bare, 33)["hyp"], ref["hyp"])


# --------------------------------------------------------------------------- the raw ABI
def _raw(gpu, pairs, nit, sigma=1.0, null=(), inl_off=None, npair=None):
    """orbm_initializer_ransac with poison-filled outputs: (rc, res, inlH, inlF)"""
    arr = (gpu.RansacPair * max(len(pairs), 1))()
    keep = []
    total = [0]
    for p, pr in enumerate(pairs):
        a = [np.ascontiguousarray(pr["keys1"], U.KEYPOINT_DTYPE), np.ascontiguousarray(pr["keys2"], U.KEYPOINT_DTYPE),
             np.ascontiguousarray(pr["match12"], np.int32), np.ascontiguousarray(pr["sets"], np.int32).reshape(-1)]
        keep.append(a)
        ptr = [None if ("pair.%s" % k) in null else x.ctypes.data_as(ctypes.c_void_p)
               for k, x in zip(("keys1", "keys2", "match12", "sets"), a)]
        arr[p] = gpu.RansacPair(pr.get("n1", len(a[0])), pr.get("n2", len(a[1])), *ptr)
        total.append(total[-1] + int((a[2] >= 0).sum()))
    off = np.array(total if inl_off is None else inl_off, np.int32)
    res = np.full(max(len(pairs), 1) * 24, 0x7B7B7B7B, np.uint32)
    inl = [np.full(max(total[-1], 1) + 16, 0x7B, np.uint8) for _ in range(2)]
    P = lambda name, a: None if name in null else a.ctypes.data_as(ctypes.c_void_p)
    rc = gpu.lib().orbm_initializer_ransac(len(pairs) if npair is None else npair,
                                           None if "pairs" in null else ctypes.cast(arr, ctypes.c_void_p), nit,
                                           ctypes.c_float(sigma), 0, P("res", res), P("inl_H", inl[0]),
                                           P("inl_F", inl[1]), P("inl_off", off))
    return rc, res, inl[0], inl[1]


def _untouched(out):
    _, res, a, b = out
    return (res == 0x7B7B7B7B).all() and (a == 0x7B).all() and (b == 0x7B).all()


def test_argument_errors_leave_the_outputs_untouched(gpu):
    pair, _ = U.scene("general", 20, 2, nit=4)
    ok = _raw(gpu, [pair], 4)
    assert ok[0] == gpu.OK and not _untouched(ok)
    assert (ok[2][20:] == 0x7B).all() and (ok[3][20:] == 0x7B).all()  # nothing past nmatch
    E, UNS = gpu.ERR_ARG, gpu.ERR_UNSUPPORTED

    def mod(**kw):
        d = {k: np.array(v) for k, v in pair.items()}
        for k, f in kw.items():
            if k in ("n1", "n2"):
                d[k] = f
            else:
                f(d[k])
        return d

    def setv(i, v, field=None):
        def f(a):
            if field:
                a[field][i] = v
            else:
                a.reshape(-1)[i] = v
        return f

    cases = [
        ("npair < 0", dict(pairs=[pair], nit=4, npair=-1), E),
        ("nit < 0", dict(pairs=[pair], nit=-1), E),
        ("pairs NULL", dict(pairs=[pair], nit=4, null=("pairs",)), E),
        ("res NULL", dict(pairs=[pair], nit=4, null=("res",)), E),
        ("inliers_H NULL", dict(pairs=[pair], nit=4, null=("inl_H",)), E),
        ("inliers_F NULL", dict(pairs=[pair], nit=4, null=("inl_F",)), E),
        ("inl_off NULL", dict(pairs=[pair], nit=4, null=("inl_off",)), E),
        ("keys1 NULL", dict(pairs=[pair], nit=4, null=("pair.keys1",)), E),
        ("keys2 NULL", dict(pairs=[pair], nit=4, null=("pair.keys2",)), E),
        ("match12 NULL", dict(pairs=[pair], nit=4, null=("pair.match12",)), E),
        ("sets NULL", dict(pairs=[pair], nit=4, null=("pair.sets",)), E),
        ("sigma NaN", dict(pairs=[pair], nit=4, sigma=float("nan")), E),
        ("sigma inf", dict(pairs=[pair], nit=4, sigma=float("inf")), E),
        ("key NaN", dict(pairs=[mod(keys1=setv(0, np.nan, "x"))], nit=4), E),
        ("key inf (unmatched key of frame 2)", dict(pairs=[mod(keys2=setv(-1, np.inf, "y"))], nit=4), E),
        ("match12 >= n2", dict(pairs=[mod(match12=setv(0, len(pair["keys2"])))], nit=4), E),
        ("set index == nmatch", dict(pairs=[mod(sets=setv(5, 20))], nit=4), E),
        ("set index < 0", dict(pairs=[mod(sets=setv(31, -1))], nit=4), E),
        ("inl_off too narrow", dict(pairs=[pair], nit=4, inl_off=[0, 19]), E),
        ("n1 < 0", dict(pairs=[mod(n1=-1)], nit=4), E),
        ("second pair bad", dict(pairs=[pair, mod(sets=setv(0, 99))], nit=4), E),
        ("nit > 4096", dict(pairs=[pair], nit=4097), UNS),
        ("n1 > 8192", dict(pairs=[mod(n1=8193)], nit=4), UNS),
        ("n2 > 8192", dict(pairs=[mod(n2=8193)], nit=4), UNS),
    ]
    for what, kw, want in cases:
        if kw["nit"] > 4:  # the table is never read: nit is refused first
            kw["pairs"] = [dict(kw["pairs"][0], sets=np.zeros(8, np.int32))]
        out = _raw(gpu, **kw)
        assert out[0] == want, (what, out[0])
        assert _untouched(out), what
    # fewer than 8 matches: seven rows matched
    m = np.full(len(pair["keys1"]), -1, np.int32)
    m[np.nonzero(pair["match12"] >= 0)[0][:7]] = np.arange(7)
    out = _raw(gpu, [dict(pair, match12=m, sets=np.zeros((4, 8), np.int32))], 4)
    assert out[0] == E and _untouched(out)


def test_no_pairs(gpu):
    assert gpu.initializer_ransac([], 200) == []
    assert gpu.lib().orbm_initializer_ransac(0, None, 200, ctypes.c_float(1.0), 0, None, None, None, None) == gpu.OK


def test_nit_zero_reports_both_winners_absent(gpu):
    pair, nit, sigma = U.planted_cases()["nit0"]
    (got,) = gpu.initializer_ransac([pair], 0)
    assert got["it_H"] == got["it_F"] == -1 and np.isnan(got["RH"]) and got["SH"] == 0 and got["SF"] == 0
    assert not got["H21"].any() and not got["F21"].any() and not got["inliers_H"].any() and not got["inliers_F"].any()
    assert got["nmatch"] == 40
    out = _raw(gpu, [pair], 0, null=("pair.sets",))  # sets is not read
    assert out[0] == gpu.OK
