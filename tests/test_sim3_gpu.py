"""Sim3Solver's RANSAC on the GPU (csrc/kernels_sim3.hip)
against the CPU restatement (tests/cpp/sim3_ref.c): every output word bit for
bit, NaNs compared as equal, no tolerance."""
import ctypes

import numpy as np
import pytest

import kfbuild_util as KU
import sim3_util as U

pytestmark = pytest.mark.gpu

# (ncorr, nit): the wavefront and workgroup edges of both, thinned from the full
# product so that every value of either occurs with a small and a large value of
# the other; fix_scale and min_inliers in {3, 20} alternate over the rows
GRID = ((3, 1), (3, 65), (3, 300), (4, 5), (4, 64), (63, 1), (63, 63), (63, 300), (64, 5), (64, 64), (64, 65),
        (65, 1), (65, 63), (65, 300), (257, 5), (257, 64), (257, 65), (257, 300))


def _same(got, ref, what):
    bad = U.same_result(got, ref)
    assert not bad, (what, bad, {k: (got[k], ref[k]) for k in bad if k != "inliers"})
    assert len(got["inliers"]) == ref["ncorr"]


def _grid_problem(ncorr, nit, k):
    fix = bool(k & 1)
    pr, _ = U.scene(ncorr, 3, s=1.0 if fix else (0.7, 1.4)[(k >> 1) & 1], nit=nit, fix_scale=fix,
                    min_inliers=3 if ncorr < 63 or k % 3 == 0 else 20, outliers=0.25 if ncorr > 4 else 0.0)
    return pr


@pytest.mark.parametrize("k,ncorr,nit", [(k,) + g for k, g in enumerate(GRID)])
def test_size_grid(gpu, k, ncorr, nit):
    pr = _grid_problem(ncorr, nit, k)
    ref = U.ref_solve(pr)
    (got,) = gpu.sim3_solve([pr])
    assert got["ncorr"] == ncorr
    _same(got, ref, (ncorr, nit))


def test_both_parameters_take_both_values_on_the_grid():
    prs = [_grid_problem(n, i, k) for k, (n, i) in enumerate(GRID)]
    assert {p["fix_scale"] for p in prs} == {False, True} and {p["min_inliers"] for p in prs} == {3, 20}
    refs = [U.ref_solve(p) for p in prs]
    assert sum(r["it_hit"] >= 0 for r in refs) >= 6 and sum(r["it_hit"] < 0 for r in refs) >= 2


def test_batch_of_seven_interleaved(gpu):
    """the sizes interleaved with an inert problem, one without iterations and
    one that continues an earlier call: neighbouring workgroups belong to
    problems of unequal sizes, and each equals its single-problem result"""
    prs = [_grid_problem(n, i, k) for k, (n, i) in ((7, (63, 300)), (3, (4, 5)), (15, (257, 64)), (10, (64, 65)))]
    base, _ = U.scene(40, 5, nit=12)
    prs.insert(1, dict(base, min_inliers=41))                                        # inert
    prs.insert(3, dict(base, triples=np.zeros((0, 3), np.int32)))                    # nit = 0
    prs.append(dict(U.scene(65, 4, s=0.7, nit=63, fix_scale=True)[0], best_in=7))    # best_in > 0, no hit
    refs = [U.ref_solve(p) for p in prs]
    assert refs[1]["counters"]["inert"] == 1 and refs[6]["it_hit"] == -1 and refs[6]["n_best"] >= 7
    got = gpu.sim3_solve(prs)
    assert len(got) == 7
    for i, (g, r, p) in enumerate(zip(got, refs, prs)):
        _same(g, r, i)
        _same(gpu.sim3_solve([p])[0], r, ("alone", i))


@pytest.mark.parametrize("name", sorted(U.planted_cases()))
def test_planted_case(gpu, name):
    pr = U.planted_cases()[name]
    (got,) = gpu.sim3_solve([pr])
    _same(got, U.ref_solve(pr), name)


def test_planted_cases_in_one_batch(gpu):
    names = sorted(U.planted_cases())
    prs = [U.planted_cases()[n] for n in names]
    for name, g, p in zip(names, gpu.sim3_solve(prs), prs):
        _same(g, U.ref_solve(p), name)


def test_two_calls_with_best_in_carried_equal_one_run(gpu):
    """iterate(n) twice: the second call starts from the first's mnBestInliers"""
    for sc, n in ((dict(ncorr=80, seed=0, s=0.7, fix_scale=True), 30), (dict(ncorr=65, seed=2, s=1.4, fix_scale=False), 4)):
        pr, _ = U.scene(sc["ncorr"], sc["seed"], s=sc["s"], nit=2 * n, fix_scale=sc["fix_scale"], min_inliers=60)
        whole = U.ref_solve(pr)
        assert whole["it_hit"] == -1  # min_inliers is out of reach: both calls run to their end
        (a,) = gpu.sim3_solve([dict(pr, triples=pr["triples"][:n])])
        (b,) = gpu.sim3_solve([dict(pr, triples=pr["triples"][n:], best_in=a["n_best"])])
        assert b["n_best"] == whole["n_best"]
        if b["it_best"] >= 0:  # the best state moved in the second call
            assert b["it_best"] + n == whole["it_best"]
            last = b
        else:
            assert a["it_best"] == whole["it_best"]
            last = a
        for k in U.FLOAT_FIELDS:
            assert U.same_bits(last[k], whole[k]), k
        assert np.array_equal(last["inliers"], whole["inliers"])


# --------------------------------------------------------------------------- the raw ABI
def _raw(gpu, prs, null=(), inl_off=None, nprob=None, **over):
    """orbm_sim3_solve with poison-filled outputs: (rc, res, inl); over: fields
    of the first problem's struct set after it is built"""
    arr = (gpu.Sim3Problem * max(len(prs), 1))()
    keep, total = [], [0]
    for p, pr in enumerate(prs):
        arr[p] = gpu.sim3_problem(pr, keep)
        total.append(total[-1] + arr[p].ncorr)
    for k, v in over.items():
        setattr(arr[0], k, v)
    for name in null:
        if name.startswith("problem."):
            setattr(arr[0], name[8:], None)
    off = np.array(total if inl_off is None else inl_off, np.int32)
    res = np.full(max(len(prs), 1) * 29, 0x7B7B7B7B, np.uint32)
    inl = np.full(max(total[-1], 1) + 16, 0x7B, np.uint8)
    P = lambda name, a: None if name in null else a.ctypes.data_as(ctypes.c_void_p)
    rc = gpu.lib().orbm_sim3_solve(len(prs) if nprob is None else nprob,
                                   None if "problems" in null else ctypes.cast(arr, ctypes.c_void_p), 0, P("res", res),
                                   P("inliers", inl), P("inl_off", off))
    return rc, res, inl


def _untouched(out):
    return (out[1] == 0x7B7B7B7B).all() and (out[2] == 0x7B).all()


def test_argument_errors_leave_the_outputs_untouched(gpu):
    pr, _ = U.scene(20, 2, nit=4, min_inliers=5)
    ok = _raw(gpu, [pr])
    assert ok[0] == gpu.OK and not _untouched(ok)
    assert (ok[2][20:] == 0x7B).all()  # nothing past ncorr
    E, UNS = gpu.ERR_ARG, gpu.ERR_UNSUPPORTED

    def mod(key, idx, v):
        a = np.array(pr[key], copy=True)
        a.reshape(-1)[idx] = v
        return dict(pr, **{key: a})

    cases = [
        ("nprob < 0", dict(prs=[pr], nprob=-1), E),
        ("problems NULL", dict(prs=[pr], null=("problems",)), E),
        ("res NULL", dict(prs=[pr], null=("res",)), E),
        ("inliers NULL", dict(prs=[pr], null=("inliers",)), E),
        ("inl_off NULL", dict(prs=[pr], null=("inl_off",)), E),
        ("ncorr < 0", dict(prs=[pr], ncorr=-1), E),
        ("nit < 0", dict(prs=[pr], nit=-1), E),
        ("min_inliers < 0", dict(prs=[pr], min_inliers=-1), E),
        ("best_in < 0", dict(prs=[pr], best_in=-1), E),
        ("pos1 NULL", dict(prs=[pr], null=("problem.pos1",)), E),
        ("pos2 NULL", dict(prs=[pr], null=("problem.pos2",)), E),
        ("sigma2_1 NULL", dict(prs=[pr], null=("problem.sigma2_1",)), E),
        ("sigma2_2 NULL", dict(prs=[pr], null=("problem.sigma2_2",)), E),
        ("triples NULL", dict(prs=[pr], null=("problem.triples",)), E),
        ("ncorr < 3, not inert", dict(prs=[dict(pr, min_inliers=2)], ncorr=2), E),
        ("triple index == ncorr", dict(prs=[mod("triples", 5, 20)]), E),
        ("triple index < 0", dict(prs=[mod("triples", 11, -1)]), E),
        ("pos1 NaN", dict(prs=[mod("pos1", 4, np.nan)]), E),
        ("pos2 inf", dict(prs=[mod("pos2", -1, np.inf)]), E),
        ("Rcw1 NaN", dict(prs=[mod("Rcw1", 8, np.nan)]), E),
        ("tcw1 inf", dict(prs=[mod("tcw1", 0, -np.inf)]), E),
        ("Rcw2 inf", dict(prs=[mod("Rcw2", 0, np.inf)]), E),
        ("tcw2 NaN", dict(prs=[mod("tcw2", 2, np.nan)]), E),
        ("K1 NaN", dict(prs=[mod("K1", 0, np.nan)]), E),
        ("K2 inf", dict(prs=[mod("K2", 3, np.inf)]), E),
        ("sigma2 NaN", dict(prs=[mod("sigma2_1", 0, np.nan)]), E),
        ("sigma2 inf", dict(prs=[mod("sigma2_2", 19, np.inf)]), E),
        ("sigma2 < 0", dict(prs=[mod("sigma2_1", 7, -0.5)]), E),
        ("9.210 sigma2 >= 2^31", dict(prs=[mod("sigma2_2", 3, 2.4e8)]), E),
        ("inl_off too narrow", dict(prs=[pr], inl_off=[0, 19]), E),
        ("inl_off negative", dict(prs=[pr], inl_off=[-1, 20]), E),
        ("second problem bad", dict(prs=[pr, mod("triples", 0, 99)]), E),
        ("ncorr > 8192", dict(prs=[pr], ncorr=8193, inl_off=[0, 8193]), UNS),
        ("nit > 4096", dict(prs=[pr], nit=4097), UNS),
        ("nprob > 65535", dict(prs=[pr], nprob=65536), UNS),
    ]
    for what, kw, want in cases:
        out = _raw(gpu, **kw)
        assert out[0] == want, (what, out[0])
        assert _untouched(out), what
    # an inert problem reads none of its arrays
    out = _raw(gpu, [dict(pr, min_inliers=21)], null=("problem.pos1", "problem.pos2", "problem.sigma2_1",
                                                    "problem.sigma2_2", "problem.triples"))
    assert out[0] == gpu.OK and (out[2][:20] == 0).all() and (out[2][20:] == 0x7B).all()
    res = out[1].view(np.int32)
    assert list(res[:4]) == [-1, -1, 0, 20] and not out[1][4:].any()
    # the largest sigma2 the conversion admits
    assert _raw(gpu, [mod("sigma2_1", 0, 2.3e8)])[0] == gpu.OK


def test_no_problems(gpu):
    assert gpu.sim3_solve([]) == []
    assert gpu.lib().orbm_sim3_solve(0, None, 0, None, None, None) == gpu.OK


def test_nit_zero_reads_no_triples(gpu):
    pr = U.planted_cases()["nit0"]
    out = _raw(gpu, [pr], null=("problem.triples",))
    assert out[0] == gpu.OK and list(out[1].view(np.int32)[:4]) == [-1, -1, 0, 40]
    assert not out[2][:40].any() and (out[2][40:] == 0x7B).all()


def test_result_chains_into_keyframe_project(gpu):
    """res.sR21 / res.t21 go into the ORBX_KF_FORM_SIM3 camera as they stand:
    the query rows equal those of the restatement's values"""
    pr, truth = U.scene(80, 1, s=0.7, nit=60, fix_scale=False)
    ref = U.ref_solve(pr)
    (got,) = gpu.sim3_solve([pr])
    assert got["it_hit"] >= 0
    n = 80
    pts = KU.make_points(n, pos=pr["pos1"], min_dist_inv=0.5, max_dist_inv=60.0, max_dist=50.0)

    def rows(r):
        cam = KU.make_camera(pr["Rcw1"], pr["tcw1"], np.zeros(3), r["sR21"], r["t21"], *U.K, (0.0, 640.0, 0.0, 480.0))
        return gpu.keyframe_project(gpu.KF_FORM_SIM3, [(cam, pts)], th=7.5)[0]

    (qg, lg, ng), (qr, lr, nr) = rows(got), rows(ref)
    assert ng == nr and ng >= int(truth["planted"].sum()) and np.array_equal(lg, lr)
    assert qg.tobytes() == qr.tobytes()
    # and they are SearchBySim3's: a planted inlier's row lies at its observation in keyframe 2
    live = (lg >= 0) & (truth["planted"] == 1)
    p2 = ref["corr"][:, 8:10]
    assert live.sum() >= 50
    assert np.abs(qg["x"][live] - p2[live, 0]).max() < 3 and np.abs(qg["y"][live] - p2[live, 1]).max() < 3
