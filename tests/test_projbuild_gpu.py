"""Device-side projection on the GPU (csrc/kernels_projbuild.hip, DESIGN.md
§17) against the CPU restatement: query rows word for word, levels, viewing
cosines and counts with no entry excluded and no tolerance; the fused
project-and-search call against the search on the restatement's live rows."""
import functools

import numpy as np
import pytest

import projbuild_util as U
import projection_util as PU
from projbuild_util import B

pytestmark = pytest.mark.gpu

READS = {1: ("pos", "normal", "min_dist_inv", "max_dist_inv", "max_dist", "skip"),
         2: ("pos", "octave", "angle", "skip"), 3: ("pos", "max_dist", "angle", "skip")}
SEARCH_ARGS = {1: dict(nnratio=0.8, th_dist=100, check_ori=False), 2: dict(nnratio=0.6, th_dist=100, check_ori=True),
               3: dict(nnratio=0.6, th_dist=64, check_ori=True)}


def _words(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, ref, mode, what):
    """got = (q, level, view_cos, n_in_view) against a ref_project dict"""
    q, level, vc, niv = got
    assert np.array_equal(_words(q), _words(ref["q"])), (what, "q", np.nonzero(
        (_words(q).reshape(-1, 7) != _words(ref["q"]).reshape(-1, 7)).any(axis=1))[0][:8])
    assert np.array_equal(level, ref["level"]), (what, "level")
    if mode == 1:
        assert np.array_equal(_words(vc), _words(ref["view_cos"])), (what, "view_cos")
    assert niv == ref["n_in_view"], (what, niv, ref["n_in_view"])


def _only(mode, P):
    """the arrays the mode reads (the others stay NULL)"""
    return {k: P[k] for k in READS[mode]}


def _device_problem(torch, mode, cam, P, scratch=False):
    t = lambda a: torch.from_numpy(np.array(a, copy=True)).cuda()
    n = len(P["pos"])
    full = lambda v, dt, *shape: torch.full(shape, v, dtype=dt, device="cuda")
    pb = dict(camera=cam, points={k: t(v) for k, v in _only(mode, P).items()},
              n_in_view=full(-3, torch.int32, 1), n_nonfinite=full(-3, torch.int32, 1))
    if not scratch:
        pb.update(q=full(0xAB, torch.uint8, max(n, 1), 28), level=full(77, torch.int32, max(n, 1)),
                  view_cos=full(9.0, torch.float32, max(n, 1)) if mode == 1 else None)
    return pb


def _read(pb, mode):
    n = pb["points"]["pos"].shape[0]
    q = pb["q"].cpu().numpy()[:n].reshape(-1).view(PU.PROJ_QUERY_DTYPE)
    return (q, pb["level"].cpu().numpy()[:n], pb["view_cos"].cpu().numpy()[:n] if mode == 1 else None,
            int(pb["n_in_view"].cpu()[0]))


@pytest.mark.parametrize("mode", (1, 2, 3))
@pytest.mark.parametrize("n", U.SIZES)
def test_host_form_matches_restatement(gpu, mode, n):
    cam, P = U.random_scene(mode, n, 100 + mode)
    ref = U.scene_ref(mode, n, 100 + mode, **U.MODE_ARGS[mode])
    (got,) = gpu.project_points(mode, [(cam, _only(mode, P))], **U.MODE_ARGS[mode])
    assert len(got[0]) == n
    _same(got, ref, mode, n)


BATCH = (257, 0, 65)  # unequal sizes, one of them empty


@pytest.mark.parametrize("mode", (1, 2, 3))
def test_host_form_three_problems(gpu, mode):
    scenes = [U.random_scene(mode, n, 200 + mode + i) for i, n in enumerate(BATCH)]
    refs = [U.ref_project(mode, cam, P, **U.MODE_ARGS[mode]) for cam, P in scenes]
    assert refs[0]["n_in_view"] > 0 and refs[2]["n_in_view"] > 0 and refs[1]["n_in_view"] == 0
    got = gpu.project_points(mode, [(cam, _only(mode, P)) for cam, P in scenes], **U.MODE_ARGS[mode])
    for i, (g, r) in enumerate(zip(got, refs)):
        _same(g, r, mode, i)


@pytest.mark.parametrize("mode", (1, 2, 3))
def test_plan_form_matches_restatement(gpu, mode):
    import torch
    plan = gpu.ProjPlan(3, 64, 3000)
    for n in U.SIZES:
        cam, P = U.random_scene(mode, n, 100 + mode)
        pb = _device_problem(torch, mode, cam, P)
        plan.project(mode, [pb], **U.MODE_ARGS[mode])
        torch.cuda.synchronize()
        _same(_read(pb, mode), U.scene_ref(mode, n, 100 + mode, **U.MODE_ARGS[mode]), mode, n)
        assert int(pb["n_nonfinite"].cpu()[0]) == 0
    scenes = [U.random_scene(mode, n, 200 + mode + i) for i, n in enumerate(BATCH)]
    pbs = [_device_problem(torch, mode, cam, P) for cam, P in scenes]
    for order in (pbs, pbs[::-1]):
        plan.project(mode, order, **U.MODE_ARGS[mode])
        torch.cuda.synchronize()
        for i, (pb, (cam, P)) in enumerate(zip(pbs, scenes)):
            _same(_read(pb, mode), U.ref_project(mode, cam, P, **U.MODE_ARGS[mode]), mode, ("batch", i))
    with pytest.raises(gpu.OrbxError) as e:  # a call without q / level is a track call
        plan.project(mode, [dict(pbs[0], q=None)], **U.MODE_ARGS[mode])
    assert e.value.code == gpu.ERR_ARG
    with pytest.raises(gpu.OrbxError) as e:
        plan.project(mode, pbs + pbs[:1], **U.MODE_ARGS[mode])  # nprob > max_problems
    assert e.value.code == gpu.ERR_ARG


PLANTED = [(1, dict(th=1.0, viewing_cos_limit=0.5)), (1, dict(th=3.0, viewing_cos_limit=0.5)),
           (2, dict(th=7.0, level_rule=U.RULE_NEITHER)), (2, dict(th=7.0, level_rule=U.RULE_FORWARD)),
           (2, dict(th=7.0, level_rule=U.RULE_BACKWARD)), (3, dict(th=5.0))]


@pytest.mark.parametrize("mode,kw", PLANTED, ids=lambda v: str(v) if isinstance(v, int) else "-".join(
    "%s%g" % (k[:2], x) for k, x in v.items()))
def test_planted_edges(gpu, mode, kw):
    """the edge cases test_projbuild.py asserts on the restatement, at the
    first and last lane of a wavefront and across a block boundary"""
    import torch
    cam = U.planted_camera()
    thr = gpu.predict_scale_thresholds(cam["log_scale_factor"], 8)
    P, slots = U.planted_points(U.planted_edges(mode, thr, **kw))
    ref = U.ref_project(mode, cam, P, **kw)
    assert {0, 63, 64, 255, 256} <= set(slots) and ref["n_nonfinite"] == 0
    (got,) = gpu.project_points(mode, [(cam, _only(mode, P))], **kw)
    _same(got, ref, mode, "host")
    pb = _device_problem(torch, mode, cam, P)
    gpu.ProjPlan(1, 64, len(P["pos"])).project(mode, [pb], **kw)
    torch.cuda.synchronize()
    _same(_read(pb, mode), ref, mode, "plan")


# --------------------------------------------------------------------------- track
NTRACK = 1025


@functools.lru_cache(maxsize=None)
def _track_scene(mode, seed):
    """(camera, points, map-point descriptors, frame): a 400-feature frame
    around the projections of the restatement's live rows"""
    cam, P = U.random_scene(mode, NTRACK, seed)
    r = U.scene_ref(mode, NTRACK, seed, **U.MODE_ARGS[mode])
    rng = np.random.default_rng(seed + 1)
    live = np.nonzero(r["branch"] == B["live"])[0]
    qdesc = rng.integers(0, 256, (NTRACK, 32)).astype(np.uint8)
    src = rng.choice(live, 400)
    q = r["q"][src]
    xs, ys = q["x"] + rng.uniform(-3, 3, 400), q["y"] + rng.uniform(-3, 3, 400)
    desc = np.array([PU.plant(rng, qdesc[s], rng.integers(0, 40)) for s in src], np.uint8)
    ur = np.where(rng.uniform(size=400) < 0.5, q["xr"] + rng.uniform(-4, 4, 400), -1.0) if mode == 1 else None
    fr = PU.make_frame(xs, ys, desc, octave=np.clip(r["level"][src] + rng.integers(-1, 2, 400), 0, 7),
                       angle=np.mod(q["angle"] + rng.normal(0, 8, 400), 360), uright=ur,
                       occupied=(rng.uniform(size=400) < 0.1).astype(np.uint8), geom="plain")
    qdesc.flags.writeable = False
    return cam, P, qdesc, fr


def _track_problem(torch, mode, cam, P, qdesc, fr, scratch):
    t = lambda a: None if a is None else torch.from_numpy(np.array(a, copy=True)).cuda()
    n = len(fr["keys"])
    pb = _device_problem(torch, mode, cam, P, scratch=scratch)
    pb.update(frame=dict(keys=t(fr["keys"].view(np.uint8).reshape(n, 28)), desc=t(fr["desc"]), uright=t(fr["uright"]),
                         occupied=t(fr["occupied"]), min_x=fr["min_x"], min_y=fr["min_y"],
                         grid_w_inv=fr["grid_w_inv"], grid_h_inv=fr["grid_h_inv"]),
              qdesc=t(qdesc), match=torch.full((n,), 7, dtype=torch.int32, device="cuda"),
              nmatches=torch.full((1,), -5, dtype=torch.int32, device="cuda"))
    return pb


def _track_expected(gpu, mode, seed):
    """the search on the restatement's live rows only, compacted in order,
    its result mapped back through the kept indices"""
    cam, P, qdesc, fr = _track_scene(mode, seed)
    r = U.scene_ref(mode, NTRACK, seed, **U.MODE_ARGS[mode])
    keep = np.nonzero(r["branch"] == B["live"])[0]
    m, nm = gpu.search_by_projection(mode, fr, r["q"][keep], qdesc[keep], **SEARCH_ARGS[mode])
    return np.where(m >= 0, keep[np.maximum(m, 0)], -1).astype(np.int32), nm, keep


@pytest.mark.parametrize("mode", (1, 2, 3))
def test_track_equals_search_on_the_live_rows(gpu, mode):
    import torch
    seed = 300 + mode
    exp_m, exp_nm, keep = _track_expected(gpu, mode, seed)
    assert exp_nm >= 40 and exp_nm == int((exp_m >= 0).sum())
    ref = U.scene_ref(mode, NTRACK, seed, **U.MODE_ARGS[mode])
    plan = gpu.ProjPlan(2, 400, NTRACK)
    for scratch in (False, True):
        pb = _track_problem(torch, mode, *_track_scene(mode, seed), scratch=scratch)
        plan.track(mode, [pb], **U.MODE_ARGS[mode], **SEARCH_ARGS[mode])
        torch.cuda.synchronize()
        m = pb["match"].cpu().numpy()
        assert np.array_equal(m, exp_m), (scratch, np.nonzero(m != exp_m)[0][:8])
        assert int(pb["nmatches"].cpu()[0]) == exp_nm
        assert set(m[m >= 0].tolist()) <= set(keep.tolist())  # inert rows take no feature
        assert int(pb["n_in_view"].cpu()[0]) == ref["n_in_view"] and int(pb["n_nonfinite"].cpu()[0]) == 0
        if not scratch:
            _same(_read(pb, mode), ref, mode, "track rows")
    # more points than the plan's max_nq, more features than its max_n
    for small in (gpu.ProjPlan(1, 400, NTRACK - 1), gpu.ProjPlan(1, 399, NTRACK)):
        with pytest.raises(gpu.OrbxError) as e:
            small.track(mode, [pb], **U.MODE_ARGS[mode], **SEARCH_ARGS[mode])
        assert e.value.code == gpu.ERR_ARG


def test_two_calls_of_one_plan_on_two_streams(gpu):
    """both calls use problem 0's scratch rows, grid and candidate lists: the
    second call's stream waits on the device for the first call's kernels"""
    import torch
    mode = 1
    seeds = (301, 311)
    exp = [_track_expected(gpu, mode, s) for s in seeds]
    assert not np.array_equal(exp[0][0], exp[1][0])
    plan = gpu.ProjPlan(1, 400, NTRACK)
    pbs = [_track_problem(torch, mode, *_track_scene(mode, s), scratch=True) for s in seeds]
    for pb, (m, nm, _) in zip(pbs, exp):  # serial
        plan.track(mode, [pb], **U.MODE_ARGS[mode], **SEARCH_ARGS[mode])
        torch.cuda.synchronize()
        assert np.array_equal(pb["match"].cpu().numpy(), m) and int(pb["nmatches"].cpu()[0]) == nm
        pb["match"].fill_(7)
        pb["nmatches"].fill_(-5)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    for _ in range(3):
        for pb, s in zip(pbs, streams):
            plan.track(mode, [pb], stream=s, **U.MODE_ARGS[mode], **SEARCH_ARGS[mode])
    torch.cuda.synchronize()
    for pb, (m, nm, _) in zip(pbs, exp):
        assert np.array_equal(pb["match"].cpu().numpy(), m) and int(pb["nmatches"].cpu()[0]) == nm


def _rc(gpu, call):
    try:
        call()
    except gpu.OrbxError as e:
        return e.code
    return gpu.OK


def test_lazy_tables_survive_every_failing_acquisition(gpu):
    """the projection's table (device rows and pinned staging) and the query
    rows of track come with a plan's first project / track call.  Whichever of
    these acquisitions fails, the call returns ORBX_ERR_HIP and the plan holds
    what it held before -- a table with its staging or neither (sweep asserts
    both) -- and the next call finds the plan usable"""
    import torch
    import test_handles_gpu as H
    mode, seed = 1, 301
    exp_m, exp_nm, _ = _track_expected(gpu, mode, seed)
    ref = U.scene_ref(mode, NTRACK, seed, **U.MODE_ARGS[mode])
    cam, P, qdesc, fr = _track_scene(mode, seed)
    L, before = gpu.lib(), H.live(gpu.lib())

    def project(plan, expect):
        pb = _device_problem(torch, mode, cam, P)
        H.sweep(gpu, lambda: _rc(gpu, lambda: plan.project(mode, [pb], **U.MODE_ARGS[mode])), expect)
        torch.cuda.synchronize()
        _same(_read(pb, mode), ref, mode, "project")
        assert int(pb["n_nonfinite"].cpu()[0]) == 0

    def track(plan, expect, scratch):
        pb = _track_problem(torch, mode, cam, P, qdesc, fr, scratch=scratch)
        call = lambda: plan.track(mode, [pb], **U.MODE_ARGS[mode], **SEARCH_ARGS[mode])
        H.sweep(gpu, lambda: _rc(gpu, call), expect)
        torch.cuda.synchronize()
        assert np.array_equal(pb["match"].cpu().numpy(), exp_m) and int(pb["nmatches"].cpu()[0]) == exp_nm
        assert int(pb["n_in_view"].cpu()[0]) == ref["n_in_view"]
        if not scratch:
            _same(_read(pb, mode), ref, mode, "track rows")

    plan = gpu.ProjPlan(1, 400, NTRACK)  # A: the table with project, the query rows with track
    created = H.live(L)
    assert sum(created) - sum(before) == H.N_PROJ
    project(plan, 2)
    assert sum(H.live(L)) - sum(created) == 2
    track(plan, 1, scratch=False)
    assert sum(H.live(L)) - sum(created) == 3
    project(plan, 0)  # nothing left to acquire
    del plan
    assert H.live(L) == before
    plan = gpu.ProjPlan(1, 400, NTRACK)  # B: all three with a first track
    track(plan, 3, scratch=True)
    assert sum(H.live(L)) - sum(created) == 3
    track(plan, 0, scratch=False)
    del plan
    assert H.live(L) == before


# --------------------------------------------------------------------------- the deviation
def _nonfinite_scene(mode):
    P, _ = U.planted_points([])
    bad = 64
    if mode == 2:
        P["octave"][bad] = 8  # outside [0, nlevels)
        P["octave"][191] = -1
        return P, (bad, 191)
    P["pos"][bad] = (0.0, 0.0, 0.0)  # zero depth on the axis: u = v = 0 * inf
    return P, (bad,)


@pytest.mark.parametrize("mode", (1, 2, 3))
def test_non_finite_point(gpu, mode):
    import torch
    cam = U.planted_camera()
    P, bad = _nonfinite_scene(mode)
    kw = U.MODE_ARGS[mode]
    ref = U.ref_project(mode, cam, P, **kw)
    assert ref["n_nonfinite"] == len(bad) and all(ref["branch"][b] == B["nonfinite"] for b in bad)
    assert ref["n_in_view"] == len(P["pos"]) - len(bad)
    with pytest.raises(gpu.OrbxError) as e:
        gpu.project_points(mode, [(cam, _only(mode, P))], **kw)
    assert e.value.code == gpu.ERR_ARG
    pb = _device_problem(torch, mode, cam, P)
    gpu.ProjPlan(1, 64, len(P["pos"])).project(mode, [pb], **kw)
    torch.cuda.synchronize()
    assert int(pb["n_nonfinite"].cpu()[0]) == len(bad)
    _same(_read(pb, mode), ref, mode, "neighbours")  # the bad row inert, every other row as without it
    good = dict(P, pos=P["pos"].copy(), octave=P["octave"].copy())
    for b in bad:
        good["pos"][b], good["octave"][b] = P["pos"][0], 1
    (got,) = gpu.project_points(mode, [(cam, _only(mode, good))], **kw)
    keep = np.ones(len(P["pos"]), bool)
    keep[list(bad)] = False
    assert np.array_equal(_words(got[0][keep]), _words(ref["q"][keep])) and got[3] == len(P["pos"])
