"""The six long-lived handles (orbx_plan, orbx_extractor, orbm_plan, orbs_plan,
orbv_vocab, orbm_proj_plan) give back every GPU resource they own
(csrc/owned.h): the process-wide counts of owned device buffers, pinned
buffers, streams and events (orbx_debug_live_resources) return to their
values from before the handle, after a round trip with real calls and after a
failure injected at every single acquisition of every create and lazy
allocation (orbx_debug_fail_acquire; nothing is asked of HIP that it cannot
give).  The C ABI is driven directly so that destruction is explicit."""
import ctypes

import numpy as np
import pytest

import projection_util as P
from orbx import synth

pytestmark = pytest.mark.gpu

W, H = 642, 361    # the smallest frame tests/test_gpu_parity.py plans
W2, H2 = 644, 362  # the extractor's second size
PRM = (1000, 1.2, 1, 20, 7)        # one level; the planner picks the level blur (a d_blur buffer)
PRM_NOBLUR = (500, 1.2, 1, 20, 7)  # 500 x 43 x 48 patch pixels < 8 x the frame's: no d_blur
PRM_EX = (1000, 1.2, 2, 20, 7)     # the extractors: a second level, so a host pyramid buffer
MB, MBF = 386.1448 / 718.856, 386.1448  # a KITTI camera's baseline (tests/test_stereo.py)
MP, PP = (2, 64, 32), (2, 64, 16)  # matcher plan (pairs, kcap, topn); projection plan (problems, n, nq)

# Owned members each call acquires, counted in csrc/:
N_PLAN = 25        # stream, h_err, 12 uploaded tables, d_blur, 10 work buffers (s_aux, ev_aux0/1: profiling builds only)
N_EXTRACTOR = 0    # orbx_extractor_create plans nothing before the first image
N_MATCH = 10       # d_probs, d_nps, d_sel, 7 scratch buffers
N_STEREO = 5       # d_rowoff, d_rows, d_sad, d_err, stream
N_VOCAB = 7        # 5 uploaded tables, d_err, stream
N_PROJ = 8         # the problem table and its staging, the fence's 2 events, 4 scratch buffers
# the extractor's plan has no d_blur (its two levels hold 392797 pixels: 1000 x 43 x 48 < 8 x that);
# + d_img, d_kps, d_desc, d_count, h_res, h_img, h_pyr, s_copy, ev_pyr
N_EXTRACT_NEW = N_PLAN - 1 + 9
N_STEREO_FIRST = N_STEREO + 8  # + d_kl, d_kr, d_dl, d_dr, d_cnt, d_ur, d_dep, d_nm
N_TRANSFORM_GROW = 8           # the one-frame staging of orbv_transform
N_BRIEF_LEVEL = 1              # d_blur


def live(L):
    c = (ctypes.c_int * 4)()
    assert L.orbx_debug_live_resources(c) == 0
    return tuple(c)


def higher(now, before):
    return all(a >= b for a, b in zip(now, before)) and sum(now) > sum(before)


def ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def synth_frames(gpu, torch, w, h, n, first=0):
    f = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    gpu.synth_frames(f, first)
    return f


# ----------------------------------------------------------------- the calls
def plan_create(gpu, prm=PRM, batch=2):
    h = ctypes.c_void_p()
    p = gpu.params(*prm)
    return gpu.lib().orbx_plan_create(ctypes.byref(p), W, H, batch, 0, ctypes.byref(h)), h


def plan_extract(gpu, torch, h, frames, prm=PRM):
    """(counts, keypoint rows, descriptors) of one orbx_plan_extract, on the host"""
    kcap, B = gpu.geometry(gpu.params(*prm), W, H).kcap, frames.shape[0]
    kps = torch.zeros((B, kcap, 28), dtype=torch.uint8, device="cuda")
    desc = torch.zeros((B, kcap, 32), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(B, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert gpu.lib().orbx_plan_extract(h, ptr(frames), B, W * H, W, ptr(kps), ptr(desc), ptr(cnt), s) == gpu.OK
    assert gpu.lib().orbx_plan_check(h, s) == gpu.OK
    c = cnt.cpu().numpy()
    assert (c > 0).all()
    return c, [kps[f, :c[f]].cpu().numpy() for f in range(B)], [desc[f, :c[f]].cpu().numpy() for f in range(B)]


def match_create(gpu):
    h = ctypes.c_void_p()
    return gpu.lib().orbm_plan_create(*MP, 0, ctypes.byref(h)), h


def match_inputs(gpu, torch):
    """two frames per pair: the same keypoints, the second frame's descriptors a few bits off the first's"""
    rng = np.random.default_rng(5)
    npairs, kcap, _ = MP
    k = np.zeros((npairs, kcap), gpu.KEYPOINT_DTYPE)
    k["x"], k["y"] = rng.uniform(0, W, (npairs, kcap)), rng.uniform(0, H, (npairs, kcap))
    k["angle"] = rng.uniform(0, 360, (npairs, kcap))
    k["response"] = rng.uniform(1, 200, (npairs, kcap))
    out = [torch.from_numpy(k.view(np.uint8).reshape(npairs, kcap, 28)).cuda() for _ in range(2)]
    base = rng.integers(0, 256, (npairs, kcap, 32), dtype=np.uint8)
    noisy = base ^ (rng.uniform(size=base.shape) < 0.2).astype(np.uint8)
    out += [torch.from_numpy(base).cuda(), torch.from_numpy(noisy).cuda()]
    out += [torch.tensor([kcap, kcap - 14], dtype=torch.int32, device="cuda"),
            torch.tensor([kcap - 3, kcap], dtype=torch.int32, device="cuda")]
    return out  # kps_a, kps_b, desc_a, desc_b, count_a, count_b


def match_frames(gpu, torch, h, inp):
    ka, kb, da, db, ca, cb = inp
    npairs, kcap, _ = MP
    m = torch.full((npairs, kcap), -9, dtype=torch.int32, device="cuda")
    nm = torch.full((npairs,), -9, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert gpu.lib().orbm_plan_match_frames(h, npairs, ptr(ka), ptr(da), ptr(ca), ptr(kb), ptr(db), ptr(cb),
                                            0.9, 1, ptr(m), ptr(nm), s) == gpu.OK
    torch.cuda.synchronize()
    return m.cpu().numpy(), nm.cpu().numpy()


def stereo_create(gpu, plan):
    h = ctypes.c_void_p()
    return gpu.lib().orbs_plan_create(plan, 2, ctypes.byref(h)), h


def vocab_records():
    return synth.vocabulary(2, 2, seed=3, stop_frac=0.0)


def vocab_create(gpu):
    v = vocab_records()
    a = [np.ascontiguousarray(v[k], t) for k, t in (("parent", np.int32), ("is_leaf", np.int32),
                                                    ("desc", np.uint8), ("weight", np.float64))]
    h = ctypes.c_void_p()
    rc = gpu.lib().orbv_vocab_create(2, 2, 0, 0, len(a[0]), *[x.ctypes.data_as(ctypes.c_void_p) for x in a], 0,
                                     ctypes.byref(h))
    return rc, h


def transform_batch(gpu, torch, v, nframes, kcap=32):
    """one orbv_transform_batch over random descriptors; its status"""
    rng = np.random.default_rng(nframes)
    desc = torch.from_numpy(rng.integers(0, 256, (nframes, kcap, 32), dtype=np.uint8)).cuda()
    cnt = torch.full((nframes,), kcap, dtype=torch.int32, device="cuda")
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")
    o = [i32(nframes, kcap), torch.zeros((nframes, kcap), dtype=torch.float64, device="cuda"), i32(nframes),
         i32(nframes, kcap), i32(nframes, kcap + 1), i32(nframes, kcap), i32(nframes)]
    s = torch.cuda.current_stream().cuda_stream
    rc = gpu.lib().orbv_transform_batch(v, nframes, ptr(desc), ptr(cnt), kcap, 1, *[ptr(t) for t in o], s)
    assert gpu.lib().orbv_check(v, s) == gpu.OK  # synchronises: the tensors outlive the kernels
    return rc


def transform_one(gpu, v, n):
    """one orbv_transform of n descriptors: (status, nbow)"""
    d = np.random.default_rng(n).integers(0, 256, (n, 32), dtype=np.uint8)
    bw, bv = np.zeros(n, np.uint32), np.zeros(n, np.float64)
    fn, fo, ff = np.zeros(n, np.uint32), np.zeros(n + 1, np.uint32), np.zeros(n, np.uint32)
    nb, nf = ctypes.c_int(-1), ctypes.c_int(-1)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = gpu.lib().orbv_transform(v, p(d), n, 1, p(bw), p(bv), ctypes.byref(nb), p(fn), p(fo), p(ff),
                                  ctypes.byref(nf))
    return rc, nb.value


def proj_create(gpu):
    h = ctypes.c_void_p()
    return gpu.lib().orbm_proj_plan_create(*PP, 0, ctypes.byref(h)), h


def proj_search(gpu, torch, h):
    """one orbm_proj_plan_search of two problems: their nmatches"""
    _, n, nq = PP
    t = lambda a: None if a is None else torch.from_numpy(np.array(a, copy=True)).cuda()
    probs = []
    for i, (pn, pq) in enumerate(((n, nq), (n - 7, nq - 3))):
        fr, q, qd = P.random_scene(pn, pq - 1, 2, seed=300 + i)  # + its whole-grid query
        probs.append(dict(keys=t(fr["keys"].view(np.uint8).reshape(pn, 28)), desc=t(fr["desc"].reshape(pn, 32)),
                          uright=t(fr["uright"]), occupied=t(fr["occupied"]),
                          q=t(np.ascontiguousarray(q).view(np.uint8).reshape(pq, 28)), qdesc=t(qd.reshape(pq, 32)),
                          match=torch.full((pn,), 7, dtype=torch.int32, device="cuda"),
                          nmatches=torch.full((1,), -5, dtype=torch.int32, device="cuda"),
                          min_x=fr["min_x"], min_y=fr["min_y"], grid_w_inv=fr["grid_w_inv"],
                          grid_h_inv=fr["grid_h_inv"]))
    plan = gpu.ProjPlan.__new__(gpu.ProjPlan)  # the class's marshalling over this handle; it does not own it
    plan._h = h
    try:
        plan.search(2, probs, **P.MODE_ARGS[2])
        torch.cuda.synchronize()
    finally:
        plan._h = None
    return [int(pb["nmatches"][0]) for pb in probs]


def extractor_create(gpu, prm=PRM_EX):
    h = ctypes.c_void_p()
    p = gpu.params(*prm)
    return gpu.lib().orbx_extractor_create(ctypes.byref(p), 0, ctypes.byref(h)), h


def extract(gpu, e, img, prm=PRM_EX):
    """one orbx_extract: (status, keypoints, descriptors)"""
    h, w = img.shape
    cap = gpu.geometry(gpu.params(*prm), w, h).kcap
    kps, desc, n = np.zeros(cap, gpu.KEYPOINT_DTYPE), np.zeros((cap, 32), np.uint8), ctypes.c_int(-1)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = gpu.lib().orbx_extract(e, p(img), w, h, w, p(kps), cap, p(desc), ctypes.byref(n))
    return rc, kps[:max(n.value, 0)], desc[:max(n.value, 0)]


def stereo_match(gpu, left, right, kl, dl, kr, dr):
    ur, dep, nm = np.zeros(len(kl), np.float32), np.zeros(len(kl), np.float32), ctypes.c_int(-1)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = gpu.lib().orbx_stereo_match(left, right, p(kl), p(dl), len(kl), p(kr), p(dr), len(kr), MB, MBF,
                                     p(ur), p(dep), ctypes.byref(nm))
    return rc, nm.value


# ---------------------------------------------------------------- 1. round trips
def test_plan_round_trip(gpu):
    import torch
    L, before = gpu.lib(), live(gpu.lib())
    rc, h = plan_create(gpu)
    assert rc == gpu.OK and higher(live(L), before)
    plan_extract(gpu, torch, h, synth_frames(gpu, torch, W, H, 2))
    assert L.orbx_plan_set_timing(h, 1) == gpu.OK  # the stage timer's events are the plan's too
    plan_extract(gpu, torch, h, synth_frames(gpu, torch, W, H, 1))
    assert live(L)[3] > before[3]
    assert L.orbx_plan_destroy(h) == gpu.OK
    assert live(L) == before


def test_match_plan_round_trip(gpu):
    import torch
    L, before = gpu.lib(), live(gpu.lib())
    rc, h = match_create(gpu)
    assert rc == gpu.OK and higher(live(L), before)
    m, nm = match_frames(gpu, torch, h, match_inputs(gpu, torch))
    assert (nm > 0).all() and [(r >= 0).sum() for r in m] == list(nm)
    assert L.orbm_plan_destroy(h) == gpu.OK
    assert live(L) == before


def test_stereo_plan_round_trip(gpu):
    import torch
    L = gpu.lib()
    plans = [plan_create(gpu)[1] for _ in range(2)]
    pairs = [synth.stereo_pair(W, H, i) for i in (3, 4)]
    fl, fr = (torch.from_numpy(np.stack([p[i] for p in pairs])).cuda() for i in (0, 1))
    kcap = gpu.geometry(gpu.params(*PRM), W, H).kcap
    side = []
    for p, f in zip(plans, (fl, fr)):
        k = torch.zeros((2, kcap, 28), dtype=torch.uint8, device="cuda")
        d = torch.zeros((2, kcap, 32), dtype=torch.uint8, device="cuda")
        c = torch.zeros(2, dtype=torch.int32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        assert L.orbx_plan_extract(p, ptr(f), 2, W * H, W, ptr(k), ptr(d), ptr(c), s) == gpu.OK
        side.append((k, d, c))
    before = live(L)
    rc, h = stereo_create(gpu, plans[0])
    assert rc == gpu.OK and higher(live(L), before)
    ur = torch.zeros((2, kcap), dtype=torch.float32, device="cuda")
    dep = torch.zeros((2, kcap), dtype=torch.float32, device="cuda")
    nm = torch.full((2,), -1, dtype=torch.int32, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    (kl, dl, cl), (kr, dr, cr) = side
    assert L.orbs_plan_match(h, 2, plans[0], plans[1], ptr(fl), ptr(fr), W * H, W, ptr(kl), ptr(dl), ptr(cl),
                             ptr(kr), ptr(dr), ptr(cr), MB, MBF, ptr(ur), ptr(dep), ptr(nm), s) == gpu.OK
    assert L.orbs_plan_check(h, s) == gpu.OK
    assert (nm.cpu().numpy() > 0).all()
    assert L.orbs_plan_destroy(h) == gpu.OK
    assert live(L) == before
    for p in plans:
        assert L.orbx_plan_destroy(p) == gpu.OK


def test_vocabulary_round_trip(gpu):
    import torch
    L, before = gpu.lib(), live(gpu.lib())
    rc, v = vocab_create(gpu)
    assert rc == gpu.OK and higher(live(L), before)
    assert transform_batch(gpu, torch, v, 1) == gpu.OK
    one = live(L)
    assert transform_batch(gpu, torch, v, 3) == gpu.OK  # outgrows the result buffer: the old one is retired
    assert live(L)[0] == one[0] + 1
    rc, nbow = transform_one(gpu, v, 20)
    assert rc == gpu.OK and nbow > 0
    assert live(L)[0] == one[0] + 1 + N_TRANSFORM_GROW
    assert L.orbv_vocab_destroy(v) == gpu.OK
    assert live(L) == before


def test_proj_plan_round_trip(gpu):
    import torch
    L, before = gpu.lib(), live(gpu.lib())
    rc, h = proj_create(gpu)
    assert rc == gpu.OK and higher(live(L), before)
    assert sum(proj_search(gpu, torch, h)) > 0
    assert L.orbm_proj_plan_destroy(h) == gpu.OK
    assert live(L) == before


def test_extractor_round_trip(gpu):
    L, before = gpu.lib(), live(gpu.lib())
    (rl, left), (rr, right) = extractor_create(gpu), extractor_create(gpu)
    assert rl == gpu.OK and rr == gpu.OK and live(L) == before  # nothing planned yet
    (img, img_r), img2 = synth.stereo_pair(W, H, 3), synth.frame(W2, H2, 1)
    rc, k1, d1 = extract(gpu, left, img)
    assert rc == gpu.OK and len(k1) > 0
    sized = live(L)
    assert higher(sized, before)
    rc, k2, _ = extract(gpu, left, img2)
    assert rc == gpu.OK and len(k2) > 0
    assert live(L) == sized  # the first size's resources went when the second replaced them
    rc, kl, dl = extract(gpu, left, img)
    assert rc == gpu.OK and np.array_equal(kl, k1) and np.array_equal(dl, d1)
    rc, kr, dr = extract(gpu, right, img_r)
    assert rc == gpu.OK
    two = live(L)
    rc, nm = stereo_match(gpu, left, right, kl, dl, kr, dr)
    assert rc == gpu.OK and nm > 0
    assert higher(live(L), two)  # the left extractor's stereo plan
    assert L.orbx_extractor_destroy(left) == gpu.OK
    assert L.orbx_extractor_destroy(right) == gpu.OK
    assert live(L) == before


# ------------------------------------------------- 2. every failing acquisition
def sweep(gpu, call, expect, handle_of=None, destroy=None):
    """Arms the k-th acquisition to fail, k = 1, 2, .., and makes the call,
    until it succeeds: each failing call returns ORBX_ERR_HIP, yields no handle
    and leaves the counts as they were; there are exactly `expect` of them.
    Returns what the succeeding call returned."""
    L = gpu.lib()
    before = live(L)
    try:
        for k in range(1, 201):
            assert L.orbx_debug_fail_acquire(k) == gpu.OK
            got = call()
            rc = got[0] if isinstance(got, tuple) else got
            L.orbx_debug_fail_acquire(0)
            if rc == gpu.OK:
                assert k - 1 == expect, (k - 1, expect)
                return got
            assert rc == gpu.ERR_HIP, (k, rc)
            if handle_of:
                assert not handle_of(got).value, k
            assert live(L) == before, (k, live(L), before)
    finally:
        L.orbx_debug_fail_acquire(0)
    pytest.fail("no acquisition count up to 200 let the call through")


@pytest.mark.parametrize("create,destroy,expect", [
    (plan_create, "orbx_plan_destroy", N_PLAN),
    (extractor_create, "orbx_extractor_destroy", N_EXTRACTOR),
    (match_create, "orbm_plan_destroy", N_MATCH),
    (vocab_create, "orbv_vocab_destroy", N_VOCAB),
    (proj_create, "orbm_proj_plan_destroy", N_PROJ),
], ids=["orbx_plan", "orbx_extractor", "orbm_plan", "orbv_vocab", "orbm_proj_plan"])
def test_create_survives_every_failing_acquisition(gpu, create, destroy, expect):
    before = live(gpu.lib())
    rc, h = sweep(gpu, lambda: create(gpu), expect, handle_of=lambda got: got[1])
    assert h.value
    assert getattr(gpu.lib(), destroy)(h) == gpu.OK
    assert live(gpu.lib()) == before


def test_stereo_create_survives_every_failing_acquisition(gpu):
    L = gpu.lib()
    plan = plan_create(gpu)[1]
    before = live(L)
    rc, h = sweep(gpu, lambda: stereo_create(gpu, plan), N_STEREO, handle_of=lambda got: got[1])
    assert L.orbs_plan_destroy(h) == gpu.OK
    assert live(L) == before
    assert L.orbx_plan_destroy(plan) == gpu.OK


def test_lazy_allocations_survive_every_failing_acquisition(gpu):
    import torch
    L, start = gpu.lib(), live(gpu.lib())
    # the first orbx_extract at a new size, then the first orbx_stereo_match
    left, right = extractor_create(gpu)[1], extractor_create(gpu)[1]
    img, img_r = synth.stereo_pair(W, H, 3)
    rc, kl, dl = sweep(gpu, lambda: extract(gpu, left, img), N_EXTRACT_NEW)
    rc, kr, dr = extract(gpu, right, img_r)
    assert rc == gpu.OK and len(kl) > 0 and len(kr) > 0
    rc, nm = sweep(gpu, lambda: stereo_match(gpu, left, right, kl, dl, kr, dr), N_STEREO_FIRST)
    assert nm > 0
    for e in (left, right):
        assert L.orbx_extractor_destroy(e) == gpu.OK
    assert live(L) == start
    # orbv_transform's staging, the result buffer already large enough for the frame
    v = vocab_create(gpu)[1]
    assert transform_batch(gpu, torch, v, 1) == gpu.OK
    rc, nbow = sweep(gpu, lambda: transform_one(gpu, v, 20), N_TRANSFORM_GROW)
    assert nbow > 0
    assert L.orbv_vocab_destroy(v) == gpu.OK
    assert live(L) == start
    # the level blur's buffer of a plan created without one
    rc, p = plan_create(gpu, PRM_NOBLUR)
    assert rc == gpu.OK
    with_plan = live(L)
    assert sum(with_plan) - sum(start) == N_PLAN - 1
    sweep(gpu, lambda: L.orbx_plan_set_options(p, gpu.ORBX_PLAN_BRIEF_LEVEL), N_BRIEF_LEVEL)
    assert live(L)[0] == with_plan[0] + 1
    plan_extract(gpu, torch, p, synth_frames(gpu, torch, W, H, 1), PRM_NOBLUR)
    assert L.orbx_plan_destroy(p) == gpu.OK
    assert live(L) == start


# ------------------------------------------------------- 3. nothing was bent
def test_results_equal_before_and_after_the_sweep(gpu):
    import torch
    L, start = gpu.lib(), live(gpu.lib())
    frames = synth_frames(gpu, torch, W, H, 1, first=11)
    inp = match_inputs(gpu, torch)
    p0, m0 = plan_create(gpu)[1], match_create(gpu)[1]
    want = plan_extract(gpu, torch, p0, frames), match_frames(gpu, torch, m0, inp)
    p1 = sweep(gpu, lambda: plan_create(gpu), N_PLAN)[1]
    m1 = sweep(gpu, lambda: match_create(gpu), N_MATCH)[1]
    got = plan_extract(gpu, torch, p1, frames), match_frames(gpu, torch, m1, inp)
    for a, b in zip(want[0], got[0]):  # counts, keypoints, descriptors
        assert np.array_equal(np.asarray(a), np.asarray(b))
    for a, b in zip(want[1], got[1]):  # match12, nmatches
        assert np.array_equal(a, b)
    for h in (p0, p1):
        assert L.orbx_plan_destroy(h) == gpu.OK
    for h in (m0, m1):
        assert L.orbm_plan_destroy(h) == gpu.OK
    assert live(L) == start
