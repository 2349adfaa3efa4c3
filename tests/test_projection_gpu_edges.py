"""orbm_search_by_projection and orbm_proj_plan_* (k_grid_build, k_proj_cand,
k_proj_resolve of csrc/kernels_proj.hip) on the planted cases of
tests/projection_util.py: the full match array and nmatches equal the
oracle's, nothing excluded, no tolerance.  Every case first asserts on the CPU,
from the path model's stats, that it reaches the path it names
(tests/test_projection_planted.py shows the model equal to the oracle)."""
import functools

import numpy as np
import pytest

import projection_util as P

pytestmark = pytest.mark.gpu

_REF = {}


def _ref(oracle, name):
    if name not in _REF:
        m, n = oracle.search_by_projection(*P.case(name).args)
        m.flags.writeable = False
        _REF[name] = (m, n)
    return _REF[name]


def _same(got, ref, what=None):
    gm, gn = got
    rm, rn = ref
    assert gn == rn, (what, gn, rn)
    assert np.array_equal(gm, rm), (what, np.nonzero(gm != rm)[0][:10])


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_planted_case_matches_oracle(gpu, oracle, name):
    c = P.case(name)
    P.assert_reaches_its_path(name)
    rm, rn = _ref(oracle, name)
    gm, gn = gpu.search_by_projection(*c.args)
    _same((gm, gn), (rm, rn), name)
    assert gn == int((gm >= 0).sum())
    for feat, qi in c.expect.items():
        assert gm[feat] == qi, (feat, int(gm[feat]), qi)
    px, py, ingrid = P.grid(c.frame)[:3]
    assert not (gm[~ingrid] >= 0).any()


def test_mode1_ignores_check_ori_and_th_dist(gpu):
    for a, b in (("rot-h11-m1-ori", "rot-h11-m1-noori"), ("thr-m1-ratio0.5-th50", "thr-m1-ratio0.5-th200")):
        ca, cb = P.case(a), P.case(b)
        assert (ca.check_ori, ca.th_dist) != (cb.check_ori, cb.th_dist)
        _same(gpu.search_by_projection(*ca.args), gpu.search_by_projection(*cb.args), a)


@functools.lru_cache(maxsize=None)
def _too_large():
    return P.random_scene(P.PJ_MAXN + 1, 1, 2, seed=5)


def test_more_than_maxn_features_is_unsupported(gpu, oracle):
    fr, q, qd = _too_large()
    with pytest.raises(gpu.OrbxError) as e:
        gpu.search_by_projection(2, fr, q, qd)
    assert e.value.code == gpu.ERR_UNSUPPORTED
    with pytest.raises(gpu.OrbxError) as e:
        gpu.ProjPlan(1, P.PJ_MAXN + 1, 1)
    assert e.value.code == gpu.ERR_UNSUPPORTED
    # and the call after the refused one is served
    name = "size-65-m2"
    _same(gpu.search_by_projection(*P.case(name).args), _ref(oracle, name))


@functools.lru_cache(maxsize=None)
def _reuse_scenes():
    return P.random_scene(P.PJ_MAXN, 4095, 2, seed=77), P.random_scene(3, 1, 2, seed=78, geom="distorted")


def test_dropin_workspace_larger_then_smaller(gpu, oracle):
    """the pooled workspace of the drop-in call: n = 8192 with 4096 queries,
    then n = 3 with 2, then the first again"""
    big, small = _reuse_scenes()
    assert len(big[1]) == 4096 and len(small[0]["keys"]) == 3 and len(small[1]) == 2
    args = dict(nnratio=0.6, th_dist=100, check_ori=True)
    rbig = oracle.search_by_projection(2, *big, **args)
    rsmall = oracle.search_by_projection(2, *small, **args)
    assert rbig[1] > 100
    _same(gpu.search_by_projection(2, *big, **args), rbig, "big")
    _same(gpu.search_by_projection(2, *small, **args), rsmall, "small")
    _same(gpu.search_by_projection(2, *big, **args), rbig, "big again")


def _device_problem(torch, fr, q, qd):
    t = lambda a: None if a is None else torch.from_numpy(np.array(a, copy=True)).cuda()
    n, nq = len(fr["keys"]), len(q)
    return dict(keys=t(fr["keys"].view(np.uint8).reshape(n, 28)), desc=t(fr["desc"].reshape(n, 32)),
                uright=t(fr["uright"]), occupied=t(fr["occupied"]),
                q=t(np.ascontiguousarray(q).view(np.uint8).reshape(nq, 28)), qdesc=t(qd.reshape(nq, 32)),
                match=torch.full((max(n, 1),), 7, dtype=torch.int32, device="cuda"),
                nmatches=torch.full((1,), -5, dtype=torch.int32, device="cuda"),
                min_x=fr["min_x"], min_y=fr["min_y"], grid_w_inv=fr["grid_w_inv"], grid_h_inv=fr["grid_h_inv"])


@functools.lru_cache(maxsize=None)
def _batch_inputs(mode):
    """(frame, q, qd) of one call's problems: n = 8192, 1, 1025, 0, 8192 (one
    cell), 65 and a problem without queries, small ones between large ones"""
    out = []
    for name in ("size-8192-m%d", "size-1-m%d", "size-1025-m%d", None, "size-8192-onecell-m%d", "size-65-m%d"):
        if name is None:
            c = P.case("size-65-m%d" % mode)
            empty = P.make_frame([], [], np.zeros((0, 32), np.uint8), geom="distorted",
                                 uright=np.zeros(0, np.float32) if mode == 1 else None)
            out.append((empty, c.q, c.qd))
        else:
            c = P.case(name % mode)
            out.append((c.frame, c.q, c.qd))
    c = P.case("size-63-m%d" % mode)
    out.append((c.frame, c.q[:0], c.qd[:0]))
    return tuple(out)


def _run_plan(torch, plan, mode, probs, refs, what):
    for pb in probs:
        pb["match"].fill_(7)
        pb["nmatches"].fill_(-5)
    plan.search(mode, probs, **P.MODE_ARGS[mode])
    torch.cuda.synchronize()
    for i, (pb, ref) in enumerate(zip(probs, refs)):
        n = pb["keys"].shape[0]
        _same((pb["match"].cpu().numpy()[:n], int(pb["nmatches"].cpu()[0])), ref, (what, i))


@pytest.mark.parametrize("mode", [1, 2, 3])
def test_plan_problems_of_different_sizes_in_one_launch(gpu, oracle, mode):
    import torch
    inputs = _batch_inputs(mode)
    assert [len(fr["keys"]) for fr, _, _ in inputs] == [8192, 1, 1025, 0, 8192, 65, 63]
    assert [len(q) for _, q, _ in inputs] == [301, 301, 301, 301, 121, 301, 0]
    refs = [oracle.search_by_projection(mode, fr, q, qd, **P.MODE_ARGS[mode]) for fr, q, qd in inputs]
    assert refs[3][1] == 0 and refs[6][1] == 0 and all(r[1] > 0 for r in refs[:3] + refs[4:6])  # the empty frame, no queries
    for (fr, q, qd), ref in zip(inputs, refs):  # the drop-in call on the same inputs
        _same(gpu.search_by_projection(mode, fr, q, qd, **P.MODE_ARGS[mode]), ref)
    probs = [_device_problem(torch, *inp) for inp in inputs]
    plan = gpu.ProjPlan(len(probs), P.PJ_MAXN, 301)
    _run_plan(torch, plan, mode, probs, refs, "forward")
    _run_plan(torch, plan, mode, probs[::-1], refs[::-1], "reversed")

    # argument errors leave the plan usable
    def refused(bad):
        with pytest.raises(gpu.OrbxError) as e:
            plan.search(mode, bad, **P.MODE_ARGS[mode])
        assert e.value.code == gpu.ERR_ARG
        _run_plan(torch, plan, mode, probs, refs, "after a refused call")

    refused(probs[:2] + [_device_problem(torch, *_too_large())])          # n > max_n
    c = P.case("size-65-m%d" % mode)
    more = (np.concatenate([c.q, c.q[:1]]), np.concatenate([c.qd, c.qd[:1]]))
    refused([_device_problem(torch, c.frame, *more)] + probs[:1])          # nq > max_nq
    refused(probs + probs[:1])                                             # nprob > max_problems
    refused(probs[:3] + [dict(probs[3], match=None)])                      # null match
