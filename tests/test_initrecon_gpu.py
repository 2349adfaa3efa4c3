"""Initializer's ReconstructH / ReconstructF on the GPU
(csrc/kernels_initrecon.hip) against the CPU restatement
(tests/cpp/initrecon_ref.c): every output word bit for bit, NaNs compared as
equal, no tolerance."""
import ctypes

import numpy as np
import pytest

import initransac_util as RU
import initrecon_util as U
from kfwindow_util import frame_dict

pytestmark = pytest.mark.gpu

TILE = 128  # RC_TILE of csrc/initrecon_internal.h: inlier matches per workgroup of the CheckRT kernel
# inlier counts: the smallest, the min(50, n - 1) index, the wavefront, the tile
COUNTS = (8, 50, 51, 52, 63, 64, 65, TILE - 1, TILE, TILE + 1)


def _same(got, ref, what):
    bad = U.same_recon(got, ref)
    assert not bad, (what, bad, {k: (got[k], ref[k]) for k in bad if k not in ("P3D", "triangulated")})


@pytest.mark.parametrize("kind", ["planar", "general"])
@pytest.mark.parametrize("n", COUNTS)
def test_inlier_counts(gpu, kind, n):
    pair, _ = U.scene(kind, n, 2, noise=0.3)
    ref = U.scene_ref(kind, n, 2, noise=0.3)
    assert ref["n_inliers"] == n and ref["ncand"] in (4, 8)
    (got,) = gpu.initializer_reconstruct([pair])
    _same(got, ref, (kind, n))


@pytest.mark.parametrize("kind", ["planar", "general"])
def test_frame_of_8192_keys(gpu, kind):
    """n1 = 8192: 6000 inliers, 1500 flagged-out matches, 692 unmatched keys"""
    args = dict(nout=1500, extra1=692, extra2=100, noise=0.3)
    pair, _ = U.scene(kind, 6000, 4, **args)
    assert len(pair["keys1"]) == 8192
    ref = U.scene_ref(kind, 6000, 4, **args)
    assert ref["ok"] == 1 and ref["triangulated"].sum() > 5900
    (got,) = gpu.initializer_reconstruct([pair])
    _same(got, ref, kind)


def _low_rh(pair):
    rs = pair["ransac"].copy()
    rs["RH"] = 0.3
    return rs


def _batch_of_seven():
    P = U.planted_cases()
    p64, _ = U.scene("planar", 64, 8)
    return [U.scene("planar", 257, 5, noise=0.3)[0], U.scene("general", 65, 5, noise=0.3)[0],
            dict(U.scene("planar", 131, 6)[0], model=U.AUTO), P["fall_through_f"][0], P["absent_model_h"][0],
            U.scene("general", 9, 7)[0], dict(p64, model=U.AUTO, ransac=_low_rh(p64))]


def test_batch_of_seven_interleaved(gpu):
    """H, F, AUTO to either side, a failing pair and an absent model, unequal
    sizes: neighbouring workgroups belong to different pairs, and each pair
    equals its single-pair result"""
    pairs = _batch_of_seven()
    refs = [U.ref_reconstruct(p) for p in pairs]
    assert [r["model_used"] for r in refs] == [U.H, U.F, U.H, U.F, U.H, U.F, U.F]
    assert [r["ok"] for r in refs] == [1, 1, 1, 0, 0, 0, 1]
    assert refs[4]["ncand"] == 0 and refs[3]["counters"]["f_fallthrough"] == 1
    got = gpu.initializer_reconstruct(pairs)
    assert len(got) == 7
    for i, (g, r) in enumerate(zip(got, refs)):
        _same(g, r, i)
    for i in (0, 3, 4, 6):
        _same(gpu.initializer_reconstruct([pairs[i]])[0], refs[i], ("alone", i))


@pytest.mark.parametrize("name", sorted(U.planted_cases()))
def test_planted_case(gpu, name):
    pair, kw = U.planted_cases()[name]
    (got,) = gpu.initializer_reconstruct([pair], **kw)
    _same(got, U.ref_reconstruct(pair, **kw), name)


def test_planted_cases_in_one_batch(gpu):
    group = [(n, p) for n, (p, kw) in sorted(U.planted_cases().items()) if not kw]
    assert len(group) >= 20
    got = gpu.initializer_reconstruct([p for _, p in group])
    for (name, p), g in zip(group, got):
        _same(g, U.ref_reconstruct(p), name)


def test_thresholds_are_arguments(gpu):
    pair, _ = U.scene("general", 60, 11)
    for kw in (dict(min_parallax=3.0), dict(min_triangulated=60), dict(min_triangulated=59), dict(sigma=0.05)):
        ref = U.ref_reconstruct(pair, **kw)
        (got,) = gpu.initializer_reconstruct([pair], **kw)
        _same(got, ref, kw)
    assert U.ref_reconstruct(pair, min_parallax=3.0)["ok"] == 0 and U.ref_reconstruct(pair, min_triangulated=59)["ok"] == 1


def test_chain_from_descriptors_to_the_initial_map(gpu):
    """search_for_initialization -> initializer_ransac -> initializer_reconstruct
    on one synthetic pair: the matcher finds the planted correspondences, the
    RANSAC its models, and the reconstruction equals the restatement run on what
    the RANSAC left"""
    scene_pair, truth = U.scene("general", 300, 9, nout=0, extra1=20, extra2=20, noise=0.2)
    k1, k2 = scene_pair["keys1"].copy(), scene_pair["keys2"].copy()
    rng = np.random.default_rng(5)
    d1 = rng.integers(0, 256, (len(k1), 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, (len(k2), 32), dtype=np.uint8)
    first, second = RU.match_list(scene_pair["match12"])
    d2[second] = d1[first]
    for k in (k1, k2):
        k["octave"], k["angle"] = 0, 0.0
    prev = np.stack([k1["x"], k1["y"]], 1).astype(np.float32)
    ((match12, _, nm),) = gpu.search_for_initialization([dict(f1=frame_dict(k1, d1, 640, 480),
                                                              f2=frame_dict(k2, d2, 640, 480), prev_matched=prev,
                                                              match12=np.full(len(k1), -1, np.int32))])
    assert nm >= 250 and (match12[first] == second).sum() >= 250
    nit = 200
    sets = RU.rng_sets(nm, nit, 3)
    (rs,) = gpu.initializer_ransac([dict(keys1=k1, keys2=k2, match12=match12, sets=sets)], nit)
    assert rs["nmatch"] == nm and rs["it_F"] >= 0
    pair = dict(keys1=k1, keys2=k2, match12=match12, K=scene_pair["K"], model=U.AUTO, ransac=gpu.ransac_record(rs),
                inliers_H=rs["inliers_H"], inliers_F=rs["inliers_F"])
    (got,) = gpu.initializer_reconstruct([dict(keys1=k1, keys2=k2, match12=match12, K=scene_pair["K"], ransac=rs)])
    ref = U.ref_reconstruct(pair)
    _same(got, ref, "chain")
    assert got["ok"] == 1 and got["model_used"] == U.F and got["triangulated"].sum() >= 200
    tn = np.linalg.norm(truth["t"])
    assert np.abs(got["R21"] - truth["R"]).max() < 5e-3 and np.abs(got["t21"] - truth["t"] / tn).max() < 5e-2


# --------------------------------------------------------------------------- the raw ABI
SENT = 0x7B


def _raw(gpu, pairs, sigma=1.0, min_parallax=1.0, null=(), key_off=None, npair=None, model=None):
    """orbm_initializer_reconstruct with poison-filled outputs: (rc, res, P3D, tri)"""
    arr = (gpu.ReconPair * max(len(pairs), 1))()
    keep, total = [], [0]
    for p, pr in enumerate(pairs):
        a = dict(keys1=np.ascontiguousarray(pr["keys1"], RU.KEYPOINT_DTYPE),
                 keys2=np.ascontiguousarray(pr["keys2"], RU.KEYPOINT_DTYPE),
                 match12=np.ascontiguousarray(pr["match12"], np.int32),
                 ransac=np.ascontiguousarray(pr["ransac"], U.RANSAC_RESULT_DTYPE).reshape(()),
                 inliers_H=np.ascontiguousarray(pr["inliers_H"], np.uint8),
                 inliers_F=np.ascontiguousarray(pr["inliers_F"], np.uint8))
        keep.append(a)
        ptr = {k: None if ("pair.%s" % k) in null else x.ctypes.data_as(ctypes.c_void_p) for k, x in a.items()}
        K = np.asarray(pr["K"], np.float32).reshape(9)
        arr[p] = gpu.ReconPair(pr.get("n1", len(a["keys1"])), pr.get("n2", len(a["keys2"])), ptr["keys1"], ptr["keys2"],
                               ptr["match12"], (ctypes.c_float * 9)(*K.tolist()),
                               int(pr["model"] if model is None else model), ptr["ransac"], ptr["inliers_H"],
                               ptr["inliers_F"])
        total.append(total[-1] + len(a["keys1"]))
    off = np.array(total if key_off is None else key_off, np.int32)
    res = np.full(max(len(pairs), 1) * 33, 0x7B7B7B7B, np.uint32)
    p3d = np.full((max(total[-1], 1) + 16) * 3, 0x7B7B7B7B, np.uint32)
    tri = np.full(max(total[-1], 1) + 16, SENT, np.uint8)
    P = lambda name, a: None if name in null else a.ctypes.data_as(ctypes.c_void_p)
    rc = gpu.lib().orbm_initializer_reconstruct(len(pairs) if npair is None else npair,
                                                None if "pairs" in null else ctypes.cast(arr, ctypes.c_void_p),
                                                ctypes.c_float(sigma), ctypes.c_float(min_parallax), 50, 0, P("res", res),
                                                P("P3D", p3d), P("tri", tri), P("key_off", off))
    return rc, res, p3d, tri


def _untouched(out):
    _, res, p3d, tri = out
    return (res == 0x7B7B7B7B).all() and (p3d == 0x7B7B7B7B).all() and (tri == SENT).all()


def test_argument_errors_leave_the_outputs_untouched(gpu):
    pair, _ = U.scene("general", 20, 2)
    n1, n2 = len(pair["keys1"]), len(pair["keys2"])
    ok = _raw(gpu, [pair])
    assert ok[0] == gpu.OK and not _untouched(ok)
    assert (ok[3][n1:] == SENT).all() and (ok[2][3 * n1:] == 0x7B7B7B7B).all()  # nothing past n1
    E, UNS = gpu.ERR_ARG, gpu.ERR_UNSUPPORTED

    def mod(**kw):
        d = {k: (np.array(v) if isinstance(v, np.ndarray) else v) for k, v in pair.items()}
        for k, f in kw.items():
            if callable(f):
                f(d[k])
            else:
                d[k] = f
        return d

    def setv(i, v, field=None):
        def f(a):
            if field:
                a[field][i] = v
            else:
                a.reshape(-1)[i] = v
        return f

    def rs(**kw):
        r = pair["ransac"].copy()
        for k, v in kw.items():
            r[k] = v
        return r

    cases = [
        ("npair < 0", dict(pairs=[pair], npair=-1), E),
        ("pairs NULL", dict(pairs=[pair], null=("pairs",)), E),
        ("res NULL", dict(pairs=[pair], null=("res",)), E),
        ("P3D NULL", dict(pairs=[pair], null=("P3D",)), E),
        ("triangulated NULL", dict(pairs=[pair], null=("tri",)), E),
        ("key_off NULL", dict(pairs=[pair], null=("key_off",)), E),
        ("keys1 NULL", dict(pairs=[pair], null=("pair.keys1",)), E),
        ("keys2 NULL", dict(pairs=[pair], null=("pair.keys2",)), E),
        ("match12 NULL", dict(pairs=[pair], null=("pair.match12",)), E),
        ("ransac NULL", dict(pairs=[pair], null=("pair.ransac",)), E),
        ("inliers_F NULL under F", dict(pairs=[pair], null=("pair.inliers_F",)), E),
        ("inliers_H NULL under H", dict(pairs=[pair], null=("pair.inliers_H",), model=U.H), E),
        ("inliers_H NULL under AUTO", dict(pairs=[pair], null=("pair.inliers_H",), model=U.AUTO), E),
        ("inliers_F NULL under AUTO", dict(pairs=[pair], null=("pair.inliers_F",), model=U.AUTO), E),
        ("model 3", dict(pairs=[pair], model=3), E),
        ("model -1", dict(pairs=[pair], model=-1), E),
        ("sigma NaN", dict(pairs=[pair], sigma=float("nan")), E),
        ("sigma inf", dict(pairs=[pair], sigma=float("inf")), E),
        ("min_parallax NaN", dict(pairs=[pair], min_parallax=float("nan")), E),
        ("K NaN", dict(pairs=[mod(K=setv(4, np.nan))]), E),
        ("K inf", dict(pairs=[mod(K=setv(2, np.inf))]), E),
        ("key NaN", dict(pairs=[mod(keys1=setv(0, np.nan, "x"))]), E),
        ("key inf (frame 2)", dict(pairs=[mod(keys2=setv(-1, np.inf, "y"))]), E),
        ("match12 >= n2", dict(pairs=[mod(match12=setv(int(np.nonzero(pair["match12"] >= 0)[0][0]), n2))]), E),
        ("nmatch one over", dict(pairs=[mod(ransac=rs(nmatch=int(pair["ransac"]["nmatch"]) + 1))]), E),
        ("nmatch one under", dict(pairs=[mod(ransac=rs(nmatch=int(pair["ransac"]["nmatch"]) - 1))]), E),
        ("key_off too narrow", dict(pairs=[pair], key_off=[0, n1 - 1]), E),
        ("key_off negative", dict(pairs=[pair], key_off=[-1, n1]), E),
        ("n1 < 0", dict(pairs=[mod(n1=-1)]), E),
        ("second pair bad", dict(pairs=[pair, mod(K=setv(0, np.nan))]), E),
        ("n1 > 8192", dict(pairs=[mod(n1=8193)]), UNS),
        ("n2 > 8192", dict(pairs=[mod(n2=8193)]), UNS),
    ]
    for what, kw, want in cases:
        out = _raw(gpu, **kw)
        assert out[0] == want, (what, out[0])
        assert _untouched(out), what
    # under a forced model the other flag array is not needed
    assert _raw(gpu, [pair], null=("pair.inliers_H",))[0] == gpu.OK


def test_no_pairs(gpu):
    assert gpu.initializer_reconstruct([]) == []
    assert gpu.lib().orbm_initializer_reconstruct(0, None, ctypes.c_float(1.0), ctypes.c_float(1.0), 50, 0, None, None,
                                                  None, None) == gpu.OK


def test_failure_zeroes_the_pairs_rows_and_keeps_the_diagnostics(gpu):
    pair, _ = U.planted_cases()["low_parallax_h"]
    out = _raw(gpu, [pair])
    n1 = len(pair["keys1"])
    assert out[0] == gpu.OK and not out[2][:3 * n1].any() and not out[3][:n1].any()
    res = out[1].view(U.RECON_RESULT_DTYPE)[0]
    assert res["ok"] == 0 and not res["R21"].any() and not res["t21"].any()
    assert res["ncand"] == 8 and res["best"] >= 0 and res["nGood"][res["best"]] == 60 and res["n_inliers"] == 60
