"""orbm_search_for_triangulation (csrc/kernels_tri.hip) against the CPU
restatement of the reference's SearchForTriangulation
(tests/cpp/triangulation_ref.c): every match12 entry and every nmatches equal,
no row excluded, no tolerance.  Inputs are planted (triangulation_util.
make_case) and each case first asserts on the restatement's output that it is
not vacuous."""
import functools
import os
import re

import numpy as np
import pytest

import triangulation_util as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# k_tri_search's tile, mirrored in the binding from csrc/tri_internal.h
# (test_tile_constants_mirror_the_kernel)
ROWS, CHUNK = 64, 64


def test_tile_constants_mirror_the_kernel(orbx_mod):
    txt = open(os.path.join(ROOT, "orb-slam-system_amd", "csrc", "tri_internal.h")).read()
    rows = int(re.search(r"#define TRI_ROWS (\d+)", txt).group(1))
    chunk = int(re.search(r"#define TRI_CHUNK (\d+)", txt).group(1))
    assert (rows, chunk) == (orbx_mod.TRI_ROWS, orbx_mod.TRI_CHUNK) == (ROWS, CHUNK)


def _nodes40(side):
    """40 nodes with gaps on both sides: ids shared, ids only KF1 has (runs of
    them, so lower_bound really jumps) and ids only KF2 has"""
    out = {}
    for j in range(60):
        both, only1, only2 = j % 3 == 0 or j % 10 == 1, j % 3 == 1 and j % 10 != 1, j % 3 == 2 and j % 10 != 1
        if len(out) < 40 and (both or (only1 if side == 1 else only2)):
            out[5 * j + 2] = 3 + (7 * j + 3 * side) % 9
    return out


# name -> (seed, KF1 {node: rows}, [KF2 {node: list length}], keyword arguments of make_case)
CASES = {
    # row blocks: 1, ROWS - 1, ROWS, ROWS + 1 and 4 * ROWS + 1 rows; lists of
    # 1, 2, CHUNK - 1, CHUNK, CHUNK + 1 and 2 * CHUNK + 2 entries; 3 neighbours
    "edges": (11, {3: 1, 7: ROWS - 1, 8: ROWS, 20: ROWS + 1, 21: 4 * ROWS + 1},
              [{3: 1, 7: 2, 8: CHUNK - 1, 20: CHUNK, 21: CHUNK + 1},
               {3: CHUNK + 1, 7: CHUNK, 8: 2, 20: CHUNK - 1, 21: 1},
               {3: 2 * CHUNK + 2, 7: 5, 8: CHUNK, 20: 1, 21: CHUNK - 1}], {}),
    "one_node": (12, {77: 30}, [{77: 30}], {}),
    "nodes40": (13, _nodes40(1), [_nodes40(2)], {}),
    # den = fmaf(a, a, b * b) subnormal for every row (F12 scaled by 2^-58)
    "subnormal": (14, {5: 40, 9: 70}, [{5: 45, 9: 66}], dict(fscale=2.0 ** -58)),
    "boundary": (15, {2: 50, 4: 50, 6: 50}, [{2: 50, 4: 50, 6: 50}], {}),
    "small": (25, {1: 9, 4: 5}, [{1: 7, 4: 6}], {}),
}
# 20 neighbours with different n2 (CreateNewMapPoints' neighbour loop)
CASES["batch20"] = (17, {3 * j + 1: 6 + (5 * j) % 17 for j in range(12)},
                    [{3 * j + 1: 1 + (7 * j + 3 * p) % 23 for j in range(12) if (j + p) % 5} for p in range(20)],
                    {})


@functools.lru_cache(maxsize=None)
def case(name):
    """(kf1, kf2 list, F12 list, restatement match12, nmatches, stats): made
    once, shared and left unchanged"""
    seed, n1, n2, kw = CASES[name]
    kf1, kf2s, Fs = T.make_case(seed, n1, n2, **kw)
    if name == "boundary":
        assert T.plant_boundary(kf1, kf2s[0], Fs[0], count=10) >= 5
    m, nm, st = T.ref_batch(kf1, kf2s, Fs)
    return kf1, kf2s, Fs, m, nm, st


def _assert_not_vacuous(name):
    kf1, kf2s, Fs, m, nm, st = case(name)
    assert nm.sum() > 0 and (m >= 0).sum() == nm.sum()
    assert (m == -2).any(), "no rotation reset"
    assert sum(s["multi"] for s in st) > 0, "no row with two or more acceptances"
    assert 0 < sum(s["accepted"] for s in st) < sum(s["evals"] for s in st)
    if name == "boundary":
        assert st[0]["flips"] > 0, "no decision the unfused arithmetic would flip"
        mw = T.ref_search(kf1, kf2s[0], Fs[0], contracted=False)[0]
        assert not np.array_equal(mw, m[0]), "the unfused form gives the same matches"
    if name == "subnormal":
        F = Fs[0].reshape(3, 3)
        x, y = kf1["keys"]["x"], kf1["keys"]["y"]
        a = x * F[0, 0] + y * F[1, 0] + F[2, 0]
        b = x * F[0, 1] + y * F[1, 1] + F[2, 1]
        den = (a * a + b * b).astype(np.float32)
        assert ((den > 0) & (den < np.finfo(np.float32).tiny)).all()
    if name == "edges":
        assert set(np.concatenate([k["keys"]["octave"] for k in kf2s]).tolist()) == set(range(8))


def _assert_equal(got, want):
    gm, gn = got
    wm, wn = want
    assert gm.shape == wm.shape and gn.shape == wn.shape
    bad = np.argwhere(gm != wm)
    assert bad.size == 0, "match12 differs at %s: got %s, want %s" % (
        bad[:8].tolist(), gm[gm != wm][:8].tolist(), wm[gm != wm][:8].tolist())
    assert np.array_equal(gn, wn), (gn.tolist(), wn.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_matches_restatement(gpu, name):
    _assert_not_vacuous(name)
    kf1, kf2s, Fs, m, nm, _ = case(name)
    _assert_equal(gpu.search_for_triangulation(kf1, kf2s, Fs), (m, nm))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edges", "batch20"])
def test_batched_equals_single_calls(gpu, name):
    """nkf2 = 1 is the reference's call; the batch is the same nkf2 times."""
    kf1, kf2s, Fs, m, nm, _ = case(name)
    assert len(kf2s) in (3, 20)
    for p, (k, F) in enumerate(zip(kf2s, Fs)):
        _assert_equal(gpu.search_for_triangulation(kf1, [k], [F]), (m[p:p + 1], nm[p:p + 1]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["edges", "nodes40"])
def test_without_orientation_check(gpu, name):
    kf1, kf2s, Fs, m1, _, _ = case(name)
    m, nm, _ = T.ref_batch(kf1, kf2s, Fs, check_ori=False)
    assert nm.sum() > 0 and not (m == -2).any() and not np.array_equal(m, m1)
    _assert_equal(gpu.search_for_triangulation(kf1, kf2s, Fs, check_ori=False), (m, nm))


@pytest.mark.gpu
def test_only_stereo_is_empty(gpu):
    kf1, kf2s, Fs, m1, _, _ = case("edges")
    m, nm, _ = T.ref_batch(kf1, kf2s, Fs, only_stereo=True)
    assert (m == -1).all() and (nm == 0).all() and (m1 >= 0).any()
    _assert_equal(gpu.search_for_triangulation(kf1, kf2s, Fs, only_stereo=True), (m, nm))


def _empty_frame():
    return dict(keys=np.zeros(0, T.KEYPOINT_DTYPE), desc=np.zeros((0, 32), np.uint8), has_mp=None,
                node_id=np.zeros(0, np.uint32), off=np.zeros(1, np.uint32), feat=np.zeros(0, np.uint32),
                level_sigma2=T.level_sigma2())


@pytest.mark.gpu
def test_empty_shapes(gpu):
    kf1, kf2s, Fs, m, nm, _ = case("small")
    # n1 = 0
    gm, gn = gpu.search_for_triangulation(_empty_frame(), kf2s, Fs)
    assert gm.shape == (1, 0) and gn.tolist() == [0]
    # nkf2 = 0
    gm, gn = gpu.search_for_triangulation(kf1, [], [])
    assert gm.shape == (0, len(kf1["keys"])) and gn.shape == (0,)
    # a neighbour with n = 0 between two real ones
    k3, F3 = [kf2s[0], _empty_frame(), kf2s[0]], [Fs[0], Fs[0], Fs[0]]
    want = T.ref_batch(kf1, k3, F3)[:2]
    assert want[1][0] > 0 and want[1][1] == 0
    _assert_equal(gpu.search_for_triangulation(kf1, k3, F3), want)
    # no common node
    other = dict(kf2s[0], node_id=kf2s[0]["node_id"] + np.uint32(100))
    want = T.ref_batch(kf1, [other], Fs)[:2]
    assert (want[0] == -1).all()
    _assert_equal(gpu.search_for_triangulation(kf1, [other], Fs), want)
    # every KF1 row has a MapPoint; has_mp = NULL on both sides
    full = dict(kf1, has_mp=np.ones(len(kf1["keys"]), np.uint8))
    want = T.ref_batch(full, kf2s, Fs)[:2]
    assert (want[0] == -1).all()
    _assert_equal(gpu.search_for_triangulation(full, kf2s, Fs), want)
    bare1, bare2 = dict(kf1, has_mp=None), [dict(kf2s[0], has_mp=None)]
    want = T.ref_batch(bare1, bare2, Fs)[:2]
    assert want[1][0] > 0 and not np.array_equal(want[0], m)
    _assert_equal(gpu.search_for_triangulation(bare1, bare2, Fs), want)


@pytest.mark.gpu
def test_repeated_kf2_indices_are_accepted(gpu):
    """nothing is claimed in KF2, so a KF2 feature listed twice is harmless"""
    kf1, kf2s, Fs, _, _, _ = case("small")
    k2 = dict(kf2s[0])
    k2["feat"] = np.concatenate([k2["feat"], k2["feat"][-3:]]).astype(np.uint32)
    k2["off"] = k2["off"].copy()
    k2["off"][-1] += 3
    want = T.ref_batch(kf1, [k2], Fs)[:2]
    assert want[1][0] > 0
    _assert_equal(gpu.search_for_triangulation(kf1, [k2], Fs), want)


@pytest.mark.gpu
def test_workspace_reuse_larger_then_smaller(gpu):
    """two calls in a row on the pooled workspace: the smaller call sees
    nothing of the larger one's rows or histogram"""
    for name in ("batch20", "small", "edges", "one_node"):
        kf1, kf2s, Fs, m, nm, _ = case(name)
        _assert_equal(gpu.search_for_triangulation(kf1, kf2s, Fs), (m, nm))


def _err(gpu, kf1, kf2s, Fs, code, **kw):
    with pytest.raises(gpu.OrbxError) as e:
        gpu.search_for_triangulation(kf1, kf2s, Fs, **kw)
    assert e.value.code == code


@pytest.mark.gpu
def test_argument_errors(gpu):
    kf1, kf2s, Fs, _, _, _ = case("small")
    k2 = kf2s[0]

    def edit(k, field, fn):
        a = k[field].copy()
        fn(a)
        return dict(k, **{field: a})

    def set_(i, v):
        return lambda a: a.__setitem__(i, v)

    # a feat index >= n, on each side
    _err(gpu, edit(kf1, "feat", set_(2, len(kf1["keys"]))), kf2s, Fs, gpu.ERR_ARG)
    _err(gpu, kf1, [edit(k2, "feat", set_(0, len(k2["keys"])))], Fs, gpu.ERR_ARG)
    # a KF2 octave outside [0, nlevels)
    for bad in (-1, 8):
        keys = k2["keys"].copy()
        keys["octave"][3] = bad
        _err(gpu, kf1, [dict(k2, keys=keys)], Fs, gpu.ERR_ARG)
    # a KF1 feature listed twice
    _err(gpu, edit(kf1, "feat", set_(1, int(kf1["feat"][0]))), kf2s, Fs, gpu.ERR_ARG)
    # node ids not ascending (equal, descending), on each side
    assert len(kf1["node_id"]) == 2
    _err(gpu, edit(kf1, "node_id", set_(1, int(kf1["node_id"][0]))), kf2s, Fs, gpu.ERR_ARG)
    _err(gpu, kf1, [edit(k2, "node_id", set_(0, int(k2["node_id"][1]) + 1))], Fs, gpu.ERR_ARG)
    # a bad device ordinal
    _err(gpu, kf1, kf2s, Fs, gpu.ERR_NO_DEVICE, device=gpu.device_count())
    _err(gpu, kf1, kf2s, Fs, gpu.ERR_NO_DEVICE, device=-1)
    # nkf2 < 0 (below the binding)
    import ctypes
    keep = []
    b1 = gpu.tri_struct(kf1, keep)
    nm = ctypes.c_int(0)
    m = np.zeros(len(kf1["keys"]), np.int32)
    assert gpu.lib().orbm_search_for_triangulation(ctypes.byref(b1), -1, None, None, 0, 1, 0,
                                                   m.ctypes.data_as(ctypes.c_void_p),
                                                   ctypes.byref(nm)) == gpu.ERR_ARG
    # and the call still works afterwards
    _assert_equal(gpu.search_for_triangulation(kf1, kf2s, Fs), case("small")[3:5])
