"""Optimizer::PoseOptimization on the GPU (csrc/kernels_poseopt.hip, DESIGN.md
§19) against the DEVICE-order CPU restatement: pose words, flags and counts
bit for bit, NaNs compared as equal, no tolerance."""
import ctypes
import functools

import numpy as np
import pytest

import poseopt_util as U
import projbuild_util as PBU
import test_poseopt as C
import test_projbuild_gpu as PB

pytestmark = pytest.mark.gpu


def _same(got, ref, what):
    T, outlier, nin = got
    assert U.same_bits(T, ref["Tcw"]), (what, T, ref["Tcw"])
    assert np.array_equal(outlier, ref["outlier"]), (what, np.flatnonzero(outlier != ref["outlier"])[:8])
    assert nin == ref["ninliers"], (what, nin, ref["ninliers"])


@functools.lru_cache(maxsize=None)
def _sweep_ref(n):
    cam, obs, _ = U.sweep_scene(n)
    return U.ref_optimize(cam, obs)


@pytest.mark.parametrize("n", U.SIZES)
def test_size_sweep(gpu, n):
    cam, obs, truth = U.sweep_scene(n)
    ref = _sweep_ref(n)
    if n >= 64:  # the restatement itself finds the plant: the comparison is of real work
        assert np.array_equal(ref["outlier"], truth["planted"])
    (got,) = gpu.pose_optimization([(cam, obs)])
    assert len(got[1]) == n
    _same(got, ref, n)


def test_batch_of_67_interleaved_sizes(gpu):
    """every size of the sweep in turn: neighbouring workgroups run unequal
    trip counts, and each problem equals its single-problem result"""
    sizes = [U.SIZES[i % len(U.SIZES)] for i in range(67)]
    got = gpu.pose_optimization([U.sweep_scene(n)[:2] for n in sizes])
    assert len(got) == 67
    for i, (g, n) in enumerate(zip(got, sizes)):
        _same(g, _sweep_ref(n), (i, n))


def test_semantics_cases_through_the_abi(gpu):
    """the cases test_poseopt.py derives by hand, and its branch-coverage set:
    the NaN paths, rho == 0, the solver failure and a round with no active edge"""
    cases = C.coverage_cases()
    refs = [U.ref_optimize(cam, obs) for _, cam, obs in cases]
    names = [c[0] for c in cases]
    assert refs[names.index("negweight")]["counters"]["solver_fail"] > 0
    assert refs[names.index("z0")]["counters"]["end_iters"] == 4
    got = gpu.pose_optimization([(cam, obs) for _, cam, obs in cases])
    for name, g, r in zip(names, got, refs):
        _same(g, r, name)
    for (name, cam, obs), r in zip(cases, refs):  # and one at a time
        _same(gpu.pose_optimization([(cam, obs)])[0], r, name)


@pytest.mark.parametrize("form", ("mask", "index"))
@pytest.mark.parametrize("kind", C.KINDS)
def test_point_forms(gpu, form, kind):
    kw = dict(form=form, stereo=kind, **U.OUTLIER_SCENE)
    cam, obs, _ = U.scene(300, 6, **kw)
    (got,) = gpu.pose_optimization([(cam, obs)])
    _same(got, U.scene_ref(300, 6, **kw), (form, kind))


def test_uright_null_is_all_monocular(gpu):
    cam, obs, _ = U.scene(200, 2, stereo="mono", **U.OUTLIER_SCENE)
    (got,) = gpu.pose_optimization([(cam, dict(obs, uright=None))])
    _same(got, U.scene_ref(200, 2, stereo="mono", **U.OUTLIER_SCENE), "uright NULL")


# --------------------------------------------------------------------------- plan form
def _device_problem(torch, cam, obs):
    t = lambda a: None if a is None else torch.from_numpy(np.array(a, copy=True)).cuda()
    n = len(obs["keys"])
    full = lambda v, dt, *shape: torch.full(shape, v, dtype=dt, device="cuda")
    return dict(camera=cam, keys=t(np.ascontiguousarray(obs["keys"]).view(np.uint8).reshape(n, 28)),
                pos=t(np.asarray(obs["pos"], np.float32).reshape(-1, 3)), uright=t(obs.get("uright")),
                point_index=t(obs.get("point_index")), has_point=t(obs.get("has_point")),
                Tcw_out=full(7.0, torch.float32, 16), outlier=full(9, torch.uint8, max(n, 1)),
                ninliers=full(-3, torch.int32, 1), status=full(-3, torch.int32, 1))


def _read(pb):
    n = pb["keys"].shape[0]
    return (pb["Tcw_out"].cpu().numpy().reshape(4, 4), pb["outlier"].cpu().numpy()[:n], int(pb["ninliers"].cpu()[0]))


def test_plan_form_matches_host_form(gpu):
    import torch
    plan = gpu.PosePlan(4, 1025)
    for n in U.SIZES:
        if n > 1025:
            continue
        cam, obs, _ = U.sweep_scene(n)
        pb = _device_problem(torch, cam, obs)
        plan.optimize([pb])
        torch.cuda.synchronize()
        _same(_read(pb), _sweep_ref(n), n)
        assert int(pb["status"].cpu()[0]) == 0
    sizes = (257, 0, 65, 9)
    pbs = [_device_problem(torch, *U.sweep_scene(n)[:2]) for n in sizes]
    for order in (pbs, pbs[::-1]):
        plan.optimize(order)
        torch.cuda.synchronize()
        for pb, n in zip(pbs, sizes):
            _same(_read(pb), _sweep_ref(n), ("batch", n))
    with pytest.raises(gpu.OrbxError) as e:
        plan.optimize(pbs + pbs[:1])  # nprob > max_problems
    assert e.value.code == gpu.ERR_ARG
    with pytest.raises(gpu.OrbxError) as e:
        gpu.PosePlan(1, 256).optimize(pbs[:1])  # n > max_n
    assert e.value.code == gpu.ERR_ARG


def test_plan_pool_form_with_missing_points(gpu):
    import torch
    kw = dict(form="index", **U.OUTLIER_SCENE)
    cam, obs, truth = U.scene(300, 6, **kw)
    assert (obs["point_index"] == -1).sum() > 20
    pb = _device_problem(torch, cam, obs)
    gpu.PosePlan(1, 300).optimize([pb])
    torch.cuda.synchronize()
    _same(_read(pb), U.scene_ref(300, 6, **kw), "pool")
    assert int(pb["status"].cpu()[0]) == 0


def test_plan_counts_bad_octave_and_index_in_status(gpu):
    import torch
    cam, obs, _ = U.scene(300, 6, form="index", **U.OUTLIER_SCENE)
    idx, keys = obs["point_index"].copy(), obs["keys"].copy()
    live = np.flatnonzero(idx >= 0)
    idx[live[0]], idx[live[1]] = len(obs["pos"]), -2
    keys["octave"][live[2]], keys["octave"][live[3]] = 8, -1
    bad = dict(obs, point_index=idx, keys=keys)
    ref = U.ref_optimize(cam, bad)
    assert ref["counters"]["invalid"] == 4
    pb = _device_problem(torch, cam, bad)
    gpu.PosePlan(1, 300).optimize([pb])
    torch.cuda.synchronize()
    _same(_read(pb), ref, "bad features dropped")
    assert int(pb["status"].cpu()[0]) == 4
    # the others are as in a problem that simply lacks those four points
    idx2 = obs["point_index"].copy()
    idx2[live[:4]] = -1
    (clean,) = gpu.pose_optimization([(cam, dict(obs, point_index=idx2))])
    _same(_read(pb), dict(Tcw=clean[0], outlier=clean[1], ninliers=clean[2]), "equals the clean problem")
    with pytest.raises(gpu.OrbxError) as e:  # the host form refuses them
        gpu.pose_optimization([(cam, bad)])
    assert e.value.code == gpu.ERR_ARG


def test_two_calls_of_one_plan_on_two_streams(gpu):
    """both calls use the plan's one problem table: the second call's stream
    waits on the device for the first call's kernel"""
    import torch
    sizes = (1025, 257)
    plan = gpu.PosePlan(1, 1025)
    pbs = [_device_problem(torch, *U.sweep_scene(n)[:2]) for n in sizes]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    for _ in range(3):
        for pb, s in zip(pbs, streams):
            plan.optimize([pb], stream=s)
    torch.cuda.synchronize()
    for pb, n in zip(pbs, sizes):
        _same(_read(pb), _sweep_ref(n), n)


def test_track_then_optimize_on_one_stream(gpu):
    """orbm_proj_plan_track's match[] is the point_index as it stands: the two
    calls on one stream, nothing read back in between, equal the host forms"""
    import torch
    mode, seed = 1, 301
    cam, P, qdesc, fr = PB._track_scene(mode, seed)
    exp_m, exp_nm, _ = PB._track_expected(gpu, mode, seed)
    assert exp_nm >= 40
    pcam = dict(Tcw=np.concatenate([cam["Rcw"], cam["tcw"].reshape(3, 1)], 1), fx=cam["fx"], fy=cam["fy"],
                cx=cam["cx"], cy=cam["cy"], mbf=cam["mbf"], inv_level_sigma2=U.inv_level_sigma2())
    obs = dict(keys=fr["keys"], uright=fr["uright"], pos=P["pos"], point_index=exp_m)
    (host,) = gpu.pose_optimization([(pcam, obs)])
    _same(host, U.ref_optimize(pcam, obs), "host forms")
    pb = PB._track_problem(torch, mode, cam, P, qdesc, fr, scratch=True)
    n = len(fr["keys"])
    pose = dict(camera=pcam, keys=pb["frame"]["keys"], uright=pb["frame"]["uright"], pos=pb["points"]["pos"],
                point_index=pb["match"], Tcw_out=torch.zeros(16, device="cuda"),
                outlier=torch.full((n,), 9, dtype=torch.uint8, device="cuda"),
                ninliers=torch.full((1,), -3, dtype=torch.int32, device="cuda"),
                status=torch.full((1,), -3, dtype=torch.int32, device="cuda"))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    gpu.ProjPlan(1, 400, PB.NTRACK).track(mode, [pb], stream=s, **PBU.MODE_ARGS[mode], **PB.SEARCH_ARGS[mode])
    gpu.PosePlan(1, 400).optimize([pose], stream=s)
    torch.cuda.synchronize()
    assert np.array_equal(pb["match"].cpu().numpy(), exp_m)
    _same(_read(pose), dict(Tcw=host[0], outlier=host[1], ninliers=host[2]), "track + optimize")
    assert int(pose["status"].cpu()[0]) == 0


# --------------------------------------------------------------------------- argument errors, handles
def _host_call(gpu, cams, obs, nprob, T, outlier, nin):
    return gpu.lib().orbm_pose_optimization(nprob, cams, obs, 0, T, outlier, nin)


def test_host_form_argument_errors_leave_outputs_untouched(gpu):
    cam, obs, _ = U.sweep_scene(64)
    keys = np.ascontiguousarray(obs["keys"])
    pos = np.ascontiguousarray(obs["pos"])
    ur = np.ascontiguousarray(obs["uright"])
    idx = np.arange(64, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    T = np.full(16, 7.0, np.float32)
    outlier = np.full(64, 9, np.uint8)
    nin = np.full(1, -3, np.int32)

    def call(nprob=1, n=64, npos=64, nlevels=8, keys_p=p(keys), pos_p=p(pos), idx_p=None, T_p=p(T), out_p=p(outlier),
             nin_p=p(nin), cams_null=False, obs_null=False):
        c = (gpu.PoseCamera * 1)(gpu.pose_camera(cam))
        c[0].nlevels = nlevels
        o = (gpu.PoseObs * 1)(gpu.PoseObs(n, keys_p, p(ur), pos_p, idx_p, None, npos))
        return _host_call(gpu, None if cams_null else ctypes.cast(c, ctypes.c_void_p),
                          None if obs_null else ctypes.cast(o, ctypes.c_void_p), nprob, T_p, out_p, nin_p)

    bad_idx_hi, bad_idx_lo = idx.copy(), idx.copy()
    bad_idx_hi[5], bad_idx_lo[5] = 64, -2
    bad_oct = keys.copy()
    bad_oct["octave"][63] = 8
    neg_oct = keys.copy()
    neg_oct["octave"][0] = -1
    for what, kw in (("nprob < 0", dict(nprob=-1)), ("n < 0", dict(n=-1)), ("n > 8192", dict(n=8193)),
                     ("npos < 0", dict(npos=-1)), ("npos < n", dict(npos=63)), ("nlevels 0", dict(nlevels=0)),
                     ("nlevels 33", dict(nlevels=33)), ("keys NULL", dict(keys_p=None)),
                     ("pos NULL", dict(pos_p=None)), ("Tcw_out NULL", dict(T_p=None)),
                     ("outlier NULL", dict(out_p=None)), ("ninliers NULL", dict(nin_p=None)),
                     ("cameras NULL", dict(cams_null=True)), ("obs NULL", dict(obs_null=True)),
                     ("index >= npos", dict(idx_p=p(bad_idx_hi))), ("index < -1", dict(idx_p=p(bad_idx_lo))),
                     ("octave >= nlevels", dict(keys_p=p(bad_oct))), ("octave < 0", dict(keys_p=p(neg_oct))),
                     ("octave >= a smaller nlevels", dict(nlevels=3))):
        assert call(**kw) == gpu.ERR_ARG, what
        assert (T == 7.0).all() and (outlier == 9).all() and nin[0] == -3, what
    assert call(nprob=0, cams_null=True, obs_null=True, T_p=None, out_p=None, nin_p=None) == gpu.OK
    assert (T == 7.0).all() and nin[0] == -3
    assert call(n=0, npos=0, keys_p=None, pos_p=None, out_p=None) == gpu.OK  # an empty frame returns 0
    assert nin[0] == 0 and np.array_equal(T[:12].reshape(3, 4), cam["Tcw"])
    assert call() == gpu.OK and nin[0] == _sweep_ref(64)["ninliers"]


def _plan_create(gpu, max_problems=2, max_n=300):
    h = ctypes.c_void_p()
    return gpu.lib().orbm_pose_plan_create(max_problems, max_n, 0, ctypes.byref(h)), h


N_POSE = 4  # the problem table and its staging, the fence's 2 events


def test_pose_plan_lifetime(gpu):
    """as tests/test_handles_gpu.py does for the other plans: the resources come
    back on destroy, and a failing acquisition yields no handle and no leak"""
    import test_handles_gpu as H
    import torch
    L, before = gpu.lib(), H.live(gpu.lib())
    rc, h = _plan_create(gpu)
    assert rc == gpu.OK and H.higher(H.live(L), before)
    cam, obs, _ = U.scene(300, 6, **U.OUTLIER_SCENE)
    pb = _device_problem(torch, cam, obs)
    arr = (gpu.PoseProblem * 1)()
    arr[0].camera = gpu.pose_camera(cam)
    arr[0].obs = gpu.PoseObs(300, pb["keys"].data_ptr(), pb["uright"].data_ptr(), pb["pos"].data_ptr(), None, None, 300)
    arr[0].Tcw_out, arr[0].outlier = pb["Tcw_out"].data_ptr(), pb["outlier"].data_ptr()
    arr[0].ninliers, arr[0].status = pb["ninliers"].data_ptr(), pb["status"].data_ptr()
    stream = torch.cuda.current_stream().cuda_stream
    assert L.orbm_pose_plan_optimize(h, 1, ctypes.cast(arr, ctypes.c_void_p), stream) == gpu.OK
    torch.cuda.synchronize()
    _same(_read(pb), U.scene_ref(300, 6, **U.OUTLIER_SCENE), "raw ABI")
    for what, f in (("Tcw_out", "Tcw_out"), ("ninliers", "ninliers"), ("status", "status"), ("outlier", "outlier")):
        keep = getattr(arr[0], f)
        setattr(arr[0], f, None)
        assert L.orbm_pose_plan_optimize(h, 1, ctypes.cast(arr, ctypes.c_void_p), stream) == gpu.ERR_ARG, what
        setattr(arr[0], f, keep)
    assert L.orbm_pose_plan_optimize(None, 1, ctypes.cast(arr, ctypes.c_void_p), stream) == gpu.ERR_ARG
    assert L.orbm_pose_plan_optimize(h, 1, None, stream) == gpu.ERR_ARG
    assert L.orbm_pose_plan_optimize(h, 0, None, stream) == gpu.OK
    assert L.orbm_pose_plan_destroy(h) == gpu.OK
    assert H.live(L) == before
    assert L.orbm_pose_plan_destroy(None) == gpu.OK
    for bad in (dict(max_problems=0), dict(max_n=0)):
        rc, h = _plan_create(gpu, **bad)
        assert rc == gpu.ERR_ARG and not h.value
    rc, h = _plan_create(gpu, max_n=8193)
    assert rc == gpu.ERR_UNSUPPORTED and not h.value
    assert L.orbm_pose_plan_create(1, 1, 0, None) == gpu.ERR_ARG
    rc, h = H.sweep(gpu, lambda: _plan_create(gpu), N_POSE, handle_of=lambda got: got[1])
    assert h.value and L.orbm_pose_plan_destroy(h) == gpu.OK
    assert H.live(L) == before
