"""Keyframe projection and the plan form of the keyframe window search on the
GPU (csrc/kernels_kfbuild.hip, csrc/api_kfbuild.hip) against the
CPU restatements: query rows word for word, levels and counts with no entry
excluded and no tolerance; the plan's search against orbm_keyframe_search and
tests/cpp/kfwindow_ref.c; project_search against kfwindow_ref on the
restatement's rows."""
import functools

import numpy as np
import pytest

import kfbuild_util as U
import kfwindow_util as KW
from kfbuild_util import B

pytestmark = pytest.mark.gpu

SEEDS = {U.FUSE: 200, U.SIM3: 201}


def _same(got, ref, what):
    """got = (q, level, n_live) against a ref_project dict"""
    q, level, nlive = got
    a, b = U.words(q), U.words(ref["q"])
    assert a.shape == b.shape and np.array_equal(a, b), (what, "q", np.nonzero((a != b).any(axis=1))[0][:8])
    assert np.array_equal(level, ref["level"]), (what, "level")
    assert nlive == ref["n_live"], (what, nlive, ref["n_live"])


def _cuda(torch, a):
    return None if a is None else torch.from_numpy(np.array(a, copy=True)).cuda()


def _device_points(torch, P):
    return {k: _cuda(torch, v) for k, v in P.items()}


def _device_problem(torch, cam, pts, n, rows=True):
    full = lambda v, dt, *shape: torch.full(shape, v, dtype=dt, device="cuda")
    pb = dict(camera=cam, points=pts, npts=n, n_live=full(-3, torch.int32, 1), n_nonfinite=full(-3, torch.int32, 1))
    if rows:
        pb.update(q=full(0xAB, torch.uint8, max(n, 1), 20), level=full(77, torch.int32, max(n, 1)))
    return pb


def _read(pb):
    n = pb["npts"]
    q = pb["q"].cpu().numpy()[:n].reshape(-1).view(KW.KF_QUERY_DTYPE)
    return q, pb["level"].cpu().numpy()[:n], int(pb["n_live"].cpu()[0])


# --------------------------------------------------------------------------- rows
@pytest.mark.parametrize("form", U.FORMS)
@pytest.mark.parametrize("n", U.SIZES)
def test_host_form_matches_restatement(gpu, form, n):
    seed = SEEDS[form]
    if n == 3000:
        U.assert_not_vacuous(form, n, seed)
    cam, P = U.random_scene(form, n, seed)
    (got,) = gpu.keyframe_project(form, [(cam, P)], th=U.TH[form])
    assert len(got[0]) == n
    _same(got, U.scene_ref(form, n, seed), n)


def _three(form):
    """three problems: 257 points; none; the first one's point set again under
    another camera with another skip"""
    cam0, P0 = U.random_scene(form, 257, 300 + form)
    cam2 = U.random_camera(form, 310 + form)
    skip2 = np.roll(P0["skip"], 5) ^ (np.arange(257) % 7 == 0).astype(np.uint8)
    assert not np.array_equal(skip2, P0["skip"])
    P2 = dict(P0, skip=skip2)
    return [(cam0, P0), (cam0, U.make_points(0)), (cam2, P2)]


@pytest.mark.parametrize("form", U.FORMS)
def test_host_form_three_problems(gpu, form):
    probs = _three(form)
    for base in (None, (0, 0, 0), (0, 257, 257)):
        refs = [U.ref_project(form, cam, P, U.TH[form], desc_base=0 if base is None else base[i])
                for i, (cam, P) in enumerate(probs)]
        assert refs[0]["n_live"] > 20 and refs[2]["n_live"] > 20 and len(refs[1]["q"]) == 0
        assert not np.array_equal(U.words(refs[0]["q"]), U.words(refs[2]["q"]))
        got = gpu.keyframe_project(form, probs, th=U.TH[form], desc_base=base)
        for i, (g, r) in enumerate(zip(got, refs)):
            _same(g, r, (base, i))


@pytest.mark.parametrize("form", U.FORMS)
def test_plan_form_matches_restatement(gpu, form):
    import torch
    seed = SEEDS[form]
    plan = gpu.KeyframePlan(3, 64, 3000)
    for n in U.SIZES:
        cam, P = U.random_scene(form, n, seed)
        pb = _device_problem(torch, cam, _device_points(torch, P), n)
        plan.project(form, [pb], th=U.TH[form])
        torch.cuda.synchronize()
        _same(_read(pb), U.scene_ref(form, n, seed), n)
        assert int(pb["n_nonfinite"].cpu()[0]) == 0
    probs = _three(form)
    shared = _device_points(torch, probs[0][1])  # problems 0 and 2 alias one point set; the skips differ
    pts = [shared, _device_points(torch, probs[1][1]), dict(shared, skip=_cuda(torch, probs[2][1]["skip"]))]
    pbs = [_device_problem(torch, cam, p, len(P["pos"])) for (cam, P), p in zip(probs, pts)]
    refs = [U.ref_project(form, cam, P, U.TH[form]) for cam, P in probs]
    for order in (pbs, pbs[::-1]):
        plan.project(form, order, th=U.TH[form])
        torch.cuda.synchronize()
        for i, (pb, r) in enumerate(zip(pbs, refs)):
            _same(_read(pb), r, ("batch", i))
    with pytest.raises(gpu.OrbxError) as e:  # project alone needs q and level
        plan.project(form, [dict(pbs[0], q=None)], th=U.TH[form])
    assert e.value.code == gpu.ERR_ARG
    with pytest.raises(gpu.OrbxError) as e:
        plan.project(form, pbs + pbs[:1], th=U.TH[form])  # nprob > max_problems
    assert e.value.code == gpu.ERR_ARG
    with pytest.raises(gpu.OrbxError) as e:
        plan.project(3, pbs, th=U.TH[form])
    assert e.value.code == gpu.ERR_ARG


@pytest.mark.parametrize("form", U.FORMS)
def test_planted_edges(gpu, form):
    """the edge cases test_kfbuild.py asserts on the restatement, at the first
    and last lane of a wavefront (63 | 64) and across a block boundary (255 | 256)"""
    import torch
    cam = U.planted_camera()
    th = U.TH[form]
    thr = gpu.predict_scale_thresholds(cam["log_scale_factor"], 8)
    edges = U.planted_edges(thr)
    P, slots = U.planted_points(edges)
    ref = U.ref_project(form, cam, P, th)
    U.check_planted(edges, slots, ref, th, cam)
    assert {0, 63, 64, 255, 256} <= set(slots) and ref["n_nonfinite"] == 0
    (got,) = gpu.keyframe_project(form, [(cam, P)], th=th)
    _same(got, ref, "host")
    n = len(P["pos"])
    pb = _device_problem(torch, cam, _device_points(torch, P), n)
    gpu.KeyframePlan(1, 64, n).project(form, [pb], th=th)
    torch.cuda.synchronize()
    _same(_read(pb), ref, "plan")


# --------------------------------------------------------------------------- the plan's search
def _device_frame(torch, kf):
    n = len(kf["keys"])
    return dict(keys=_cuda(torch, kf["keys"].view(np.uint8).reshape(n, 28)), desc=_cuda(torch, kf["desc"].reshape(n, 32)),
                min_x=kf["min_x"], min_y=kf["min_y"], grid_w_inv=kf["grid_w_inv"], grid_h_inv=kf["grid_h_inv"])


def _search_problem(torch, kf, q, qd):
    nq = len(q)
    return dict(frame=_device_frame(torch, kf), npts=nq, q=_cuda(torch, q.view(np.uint8).reshape(nq, 20)),
                qdesc=_cuda(torch, qd.reshape(nq, 32)),
                best_idx=torch.full((max(nq, 1),), -9, dtype=torch.int32, device="cuda"),
                best_dist=torch.full((max(nq, 1),), -9, dtype=torch.int32, device="cuda"))


def test_plan_search_equals_keyframe_search(gpu):
    import torch
    rng = np.random.RandomState(77)
    kfs, qs, qds = [], [], []
    for n, nq in ((0, 40), (1, 33), (500, 700), (2000, 0), (2000, 1500)):  # one problem without queries
        kf = KW.make_frame(rng, n)
        q, qd = KW.make_queries(rng, kf, nq)
        kfs.append(kf), qs.append(q), qds.append(qd)
    refs = [KW.ref_search(kf, q, qd) for kf, q, qd in zip(kfs, qs, qds)]
    KW.assert_not_vacuous(kfs[4], *refs[4])
    plan = gpu.KeyframePlan(5, 2000, 1500)
    pbs = [_search_problem(torch, kf, q, qd) for kf, q, qd in zip(kfs, qs, qds)]
    plan.search(pbs)
    torch.cuda.synchronize()
    for p, (pb, (bi, bd, _)) in enumerate(zip(pbs, refs)):
        nq = len(qs[p])
        (hi, hd), = gpu.keyframe_search([kfs[p]], [qs[p]], qds[p] if nq else np.zeros((1, 32), np.uint8))
        gi, gd = pb["best_idx"].cpu().numpy()[:nq], pb["best_dist"].cpu().numpy()[:nq]
        assert np.array_equal(gi, bi) and np.array_equal(gd, bd), (p, np.nonzero(gi != bi)[0][:8])
        assert np.array_equal(gi, hi) and np.array_equal(gd, hd), p
    assert (pbs[3]["best_idx"].cpu().numpy() == -9).all()  # no queries: nothing written
    # a desc outside the problem's pool is answered like an empty window
    bad = qs[2].copy()
    bad["desc"][5], bad["desc"][6] = len(bad), -1
    pb = _search_problem(torch, kfs[2], bad, qds[2])
    plan.search([pb])
    torch.cuda.synchronize()
    gi, gd = pb["best_idx"].cpu().numpy(), pb["best_dist"].cpu().numpy()
    keep = np.ones(len(bad), bool)
    keep[5:7] = False
    assert (gi[5:7] == -1).all() and (gd[5:7] == KW.INT_MAX).all()
    assert np.array_equal(gi[keep], refs[2][0][keep]) and np.array_equal(gd[keep], refs[2][1][keep])
    for small in (gpu.KeyframePlan(1, 1999, 1500), gpu.KeyframePlan(1, 2000, 1499)):
        with pytest.raises(gpu.OrbxError) as e:
            small.search(pbs[4:])
        assert e.value.code == gpu.ERR_ARG


# --------------------------------------------------------------------------- project_search
NPS, NFEAT = 3000, 2000


@functools.lru_cache(maxsize=None)
def _ps_scene(form, seed):
    """(camera, points, map-point descriptors, keyframe): NFEAT features around
    the projections of the restatement's live rows, at the predicted level or
    the one below, descriptors a few bits off the map points'"""
    cam, P = U.random_scene(form, NPS, seed)
    r = U.scene_ref(form, NPS, seed)
    rng = np.random.RandomState(seed + 1)
    live = np.nonzero(r["branch"] == B["live"])[0]
    qdesc = rng.randint(0, 256, (NPS, 32)).astype(np.uint8)
    src = rng.choice(live, NFEAT)
    q = r["q"][src]
    xs = (q["x"] + rng.uniform(-4, 4, NFEAT)).astype(np.float32)
    ys = (q["y"] + rng.uniform(-4, 4, NFEAT)).astype(np.float32)
    desc = np.array([KW.flip(rng, qdesc[s], int(rng.randint(0, 40))) for s in src], np.uint8)
    octv = np.clip(q["level"] - rng.randint(0, 3, NFEAT) + 1, 0, 7).astype(np.int32)
    kf = KW.frame_dict(KW.make_keys(xs, ys, octv), desc)
    qdesc.flags.writeable = False
    return cam, P, qdesc, kf


def _ps_problem(torch, form, seed, rows):
    cam, P, qdesc, kf = _ps_scene(form, seed)
    pb = _device_problem(torch, cam, _device_points(torch, P), NPS, rows=rows)
    pb.update(frame=_device_frame(torch, kf), qdesc=_cuda(torch, qdesc),
              best_idx=torch.full((NPS,), -9, dtype=torch.int32, device="cuda"),
              best_dist=torch.full((NPS,), -9, dtype=torch.int32, device="cuda"))
    return pb


@functools.lru_cache(maxsize=None)
def _ps_expected(form, seed):
    cam, P, qdesc, kf = _ps_scene(form, seed)
    r = U.scene_ref(form, NPS, seed)
    bi, bd, _ = KW.ref_search(kf, r["q"], qdesc)
    return bi, bd


@pytest.mark.parametrize("form", U.FORMS)
def test_project_search_equals_search_on_the_restatement_rows(gpu, form):
    import torch
    seed = 400 + form
    cam, P, qdesc, kf = _ps_scene(form, seed)
    r = U.scene_ref(form, NPS, seed)
    bi, bd = _ps_expected(form, seed)
    live = r["branch"] == B["live"]
    assert (bi[~live] == -1).all() and (bd[~live] == KW.INT_MAX).all()  # inert rows find nothing
    assert (bd[live] <= 50).sum() >= 200
    keep = np.nonzero(live)[0]
    li, ld, _ = KW.ref_search(kf, r["q"][keep], qdesc)  # the live rows alone (desc still names the pool row)
    assert np.array_equal(li, bi[keep]) and np.array_equal(ld, bd[keep])
    plan = gpu.KeyframePlan(2, NFEAT, NPS)
    for rows in (True, False):
        pb = _ps_problem(torch, form, seed, rows)
        plan.project_search(form, [pb], th=U.TH[form])
        torch.cuda.synchronize()
        gi, gd = pb["best_idx"].cpu().numpy(), pb["best_dist"].cpu().numpy()
        assert np.array_equal(gi, bi) and np.array_equal(gd, bd), (rows, np.nonzero(gi != bi)[0][:8])
        assert int(pb["n_live"].cpu()[0]) == r["n_live"] and int(pb["n_nonfinite"].cpu()[0]) == 0
        if rows:
            _same(_read(pb), r, "project_search rows")
    # one point set and pool, two keyframes: the batched Fuse's shape
    cam2 = U.random_camera(form, seed + 50)
    r2 = U.ref_project(form, cam2, P, U.TH[form])
    b2 = KW.ref_search(kf, r2["q"], qdesc)
    other = dict(_ps_problem(torch, form, seed, False), camera=cam2, points=pb["points"], qdesc=pb["qdesc"])
    pb["best_idx"].fill_(-9)
    plan.project_search(form, [pb, other], th=U.TH[form])
    torch.cuda.synchronize()
    assert np.array_equal(pb["best_idx"].cpu().numpy(), bi) and np.array_equal(pb["best_dist"].cpu().numpy(), bd)
    assert np.array_equal(other["best_idx"].cpu().numpy(), b2[0])
    assert np.array_equal(other["best_dist"].cpu().numpy(), b2[1])
    assert int(other["n_live"].cpu()[0]) == r2["n_live"]


def test_two_calls_of_one_plan_on_two_streams(gpu):
    """both calls use problem 0's scratch rows, grid and records: the second
    call's stream waits on the device for the first call's kernels"""
    import torch
    cases = ((U.FUSE, 401), (U.SIM3, 402))
    exp = [_ps_expected(f, s) for f, s in cases]
    assert not np.array_equal(exp[0][0], exp[1][0])
    plan = gpu.KeyframePlan(1, NFEAT, NPS)
    pbs = [_ps_problem(torch, f, s, False) for f, s in cases]
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for _ in range(3):
        for (f, _s), pb, st in zip(cases, pbs, streams):
            plan.project_search(f, [pb], th=U.TH[f], stream=st)
    torch.cuda.synchronize()
    for pb, (bi, bd) in zip(pbs, exp):
        assert np.array_equal(pb["best_idx"].cpu().numpy(), bi) and np.array_equal(pb["best_dist"].cpu().numpy(), bd)


# --------------------------------------------------------------------------- the deviation, the handle
@pytest.mark.parametrize("form", U.FORMS)
def test_non_finite_radius(gpu, form):
    import torch
    cam = U.planted_camera()
    P, bad = U.nonfinite_scene()
    n = len(P["pos"])
    ref = U.ref_project(form, cam, P, U.TH_OVERFLOW)
    assert ref["n_nonfinite"] == len(bad) and ref["n_live"] == n - len(bad)
    q = np.full(n, 7, gpu.KF_QUERY_DTYPE)
    level, nlive = np.full(n, 7, np.int32), np.full(1, 7, np.int32)
    with pytest.raises(gpu.OrbxError) as e:
        gpu.keyframe_project(form, [(cam, P)], th=U.TH_OVERFLOW)
    assert e.value.code == gpu.ERR_ARG
    # the C call itself: no output is written
    import ctypes
    c = (gpu.KfCamera * 1)(gpu.kf_camera(cam))
    pp = (gpu.KfPoints * 1)(gpu.KfPoints(*[P[k].ctypes.data for k in U.POINT_FIELDS]))
    npts = np.array([n], np.int32)
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = gpu.lib().orbm_keyframe_project(form, 1, ctypes.cast(c, ctypes.c_void_p), ctypes.cast(pp, ctypes.c_void_p),
                                         vp(npts), None, U.TH_OVERFLOW, 0, vp(q), vp(level), vp(nlive))
    assert rc == gpu.ERR_ARG
    assert (level == 7).all() and nlive[0] == 7 and (q["desc"] == 7).all() and (q["x"] == 7).all()
    pb = _device_problem(torch, cam, _device_points(torch, P), n)
    gpu.KeyframePlan(1, 64, n).project(form, [pb], th=U.TH_OVERFLOW)
    torch.cuda.synchronize()
    assert int(pb["n_nonfinite"].cpu()[0]) == len(bad)
    _same(_read(pb), ref, "neighbours")  # the bad rows inert, every other row as without them


def test_plan_resources_are_counted_and_returned(gpu):
    def live():
        import ctypes
        c = np.zeros(4, np.int32)
        assert gpu.lib().orbx_debug_live_resources(c.ctypes.data_as(ctypes.c_void_p)) == gpu.OK
        return c
    before = live()
    plan = gpu.KeyframePlan(4, 500, 800)
    held = live() - before
    assert held[0] == 5 and held[1] == 2 and held[2] == 0 and held[3] == 2, held
    del plan
    assert np.array_equal(live(), before)
    # a create that fails half way leaves nothing behind, whichever acquisition fails
    # (and the tenth attempt, with all nine made, succeeds)
    import ctypes
    import test_handles_gpu as H

    def create():
        h = ctypes.c_void_p()
        return gpu.lib().orbm_kf_plan_create(4, 500, 800, 0, ctypes.byref(h)), h
    rc, h = H.sweep(gpu, create, 9, handle_of=lambda got: got[1])
    assert h.value and gpu.lib().orbm_kf_plan_destroy(h) == gpu.OK
    assert np.array_equal(live(), before)
