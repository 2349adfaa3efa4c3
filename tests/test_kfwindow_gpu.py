"""orbm_keyframe_search (csrc/kernels_kfwin.hip) against the CPU restatement
of the search ORBmatcher::Fuse / SearchBySim3 share (tests/cpp/kfwindow_ref.c):
every best_idx and best_dist equal, no entry excluded, no tolerance.  Inputs
are planted (kfwindow_util) and each case first asserts on the restatement
alone that it is not vacuous."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import kfwindow_util as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# k_kfwin_search's lanes per query, mirrored in the binding from
# csrc/kfwin_internal.h (test_group_size_mirrors_the_kernel)
G = 8
COUNTS = (0, 1, G - 1, G, G + 1, 2 * G + 1)


def test_group_size_mirrors_the_kernel(orbx_mod):
    txt = open(os.path.join(ROOT, "orb-slam-system_amd", "csrc", "kfwin_internal.h")).read()
    g = int(re.search(r"#define KFW_G (\d+)", txt).group(1))
    maxn = int(re.search(r"#define KFW_MAXN (\d+)", txt).group(1))
    assert (g, maxn) == (orbx_mod.KFW_G, orbx_mod.KFW_MAXN) == (G, 8192)
    assert g < 64 and g & (g - 1) == 0
    assert orbx_mod.KF_QUERY_DTYPE == K.KF_QUERY_DTYPE


def _planted(seed, n, nq, **kw):
    rng = np.random.RandomState(seed)
    fkw = {k: kw.pop(k) for k in ("xmax", "dup") if k in kw}
    kf = K.make_frame(rng, n, **fkw)
    q, qd = K.make_queries(rng, kf, nq, **kw)
    return kf, q, qd


def _append(kf, xs, ys, octv, desc):
    keys = np.concatenate([kf["keys"], K.make_keys(xs, ys, octv)])
    return K.frame_dict(keys, np.concatenate([kf["desc"], desc]))


def _extra_queries(q, qd, rows, descs=None):
    """rows of (x, y, radius, level) appended, each with a pool row of its own:
    descs[i], or a nearly-zero descriptor where that is None"""
    e = np.zeros(len(rows), K.KF_QUERY_DTYPE)
    for i, r in enumerate(rows):
        e[i] = tuple(r) + (len(qd) + i,)
    ed = np.zeros((len(rows), 32), np.uint8)
    ed[:, 0] = np.arange(len(rows)) & 0xFF
    for i, d in enumerate(descs or []):
        if d is not None:
            ed[i] = d
    return np.concatenate([q, e]), np.concatenate([qd, ed])


@functools.lru_cache(maxsize=None)
def case_columns():
    kf, q, qd = _planted(11, 300, 400, xmax=400)
    rng = np.random.RandomState(111)
    sf = K.scale_factors()
    rows, descs = [], []
    # one column: k features within 2 px of a cell centre, nothing else near
    for j, k in enumerate(COUNTS):
        cx, cy = 440.0 + 30.0 * j, 100.0
        d = rng.randint(0, 256, (k, 32)).astype(np.uint8)
        if k >= 3:
            d[k - 1] = d[1]  # the query's own descriptor twice: a tied minimum at a later rank
        kf = _append(kf, cx + rng.uniform(-2, 2, k), cy + rng.uniform(-2, 2, k), np.zeros(k, np.int32), d)
        rows += [(cx, cy, 3.0, 0), (cx, cy, 3.0, -1)]
        descs += [d[1] if k >= 3 else None] * 2
    # several columns: 40 features over three to four columns and two rows
    k = 40
    kf = _append(kf, 500.0 + rng.uniform(-16, 16, k), 300.0 + rng.uniform(-6, 6, k),
                 rng.randint(6, 8, k).astype(np.int32), rng.randint(0, 256, (k, 32)).astype(np.uint8))
    rows += [(500.0 + dx, 300.0, float(np.float32(3.0) * sf[7]), lv) for dx in (-8.0, 0.0, 6.0)
             for lv in (7, 6, -1)]
    nplanted = len(q)
    q, qd = _extra_queries(q, qd, rows, descs)
    return kf, q, qd, nplanted


@functools.lru_cache(maxsize=None)
def case_borders():
    kf, q, qd = _planted(12, 400, 500, border=0.35)
    rows = [(1e30, 50.0, 3.0, 0), (-1e30, 50.0, 3.0, 0), (100.0, 1e30, 3.0, 0), (100.0, 100.0, 1e30, -1),
            (100.0, 100.0, 2000.0, -1), (320.0, 240.0, 0.0, 0), (320.0, 240.0, -1.0, 0)]
    q, qd = _extra_queries(q, qd, rows)
    return kf, q, qd


@functools.lru_cache(maxsize=None)
def case_ties():
    return _planted(13, 400, 500, dup=0.5)


@functools.lru_cache(maxsize=None)
def case_gate():
    return _planted(14, 400, 600, levels=[-1, 0, 1, 2, 3, 4, 5, 6, 7])


@functools.lru_cache(maxsize=None)
def case_many():
    return _planted(15, 500, 5000)


@functools.lru_cache(maxsize=None)
def case_max_n():
    return _planted(16, 8192, 64)


BATCH_N = [0, 700, 1, 63, 64, 65, 300, 511, 512, 513, 650, 129]
BATCH_NQ = [50, 300, 0, 7, 8, 9, 33, 256, 31, 0, 100, 1]


@functools.lru_cache(maxsize=None)
def case_batch():
    """12 keyframes, one pool: 40 rows nobody uses in front, every problem's
    own rows after them, and a fifth of the queries of every problem moved to
    a row that belongs to another problem's query"""
    rng = np.random.RandomState(17)
    kfs, qs, pools = [], [], [rng.randint(0, 256, (40, 32)).astype(np.uint8)]
    base = 40
    for n, nq in zip(BATCH_N, BATCH_NQ):
        kf = K.make_frame(rng, n)
        q, qd = K.make_queries(rng, kf, nq)
        q["desc"] += base
        base += nq
        kfs.append(kf)
        qs.append(q)
        pools.append(qd)
    pool = np.concatenate(pools)
    for p, q in enumerate(qs):
        for j in range(0, len(q), 5):
            q["desc"][j] = int(rng.randint(40, len(pool)))
    used = np.bincount(np.concatenate([q["desc"] for q in qs]), minlength=len(pool))
    assert (used[:40] == 0).all() and (used > 1).sum() > 20
    return kfs, qs, pool


@functools.lru_cache(maxsize=None)
def ref_of(name):
    c = CASES[name]()
    return K.ref_search(c[0], c[1], c[2])


CASES = dict(columns=case_columns, borders=case_borders, ties=case_ties, gate=case_gate,
             many_queries=case_many, max_n=case_max_n)


def _compare(got, want_bi, want_bd):
    bi, bd = got
    assert bi.dtype == np.int32 and bd.dtype == np.int32
    assert np.array_equal(bi, want_bi), np.flatnonzero(bi != want_bi)[:10]
    assert np.array_equal(bd, want_bd), np.flatnonzero(bd != want_bd)[:10]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_equals_restatement(gpu, name):
    c = CASES[name]()
    kf, q, qd = c[0], c[1], c[2]
    bi, bd, st = ref_of(name)
    K.assert_not_vacuous(kf, bi, bd, st)
    if name == "columns":
        ex = slice(c[3], None)
        one = st["visited"][ex][:2 * len(COUNTS)]
        assert one.tolist() == [k for k in COUNTS for _ in (0, 1)]  # exactly k in the window's columns
        assert st["boxed"][ex][:2 * len(COUNTS)].tolist() == one.tolist()
        assert (st["visited"][ex][2 * len(COUNTS):] > 2 * G + 1).all()  # several columns and rows
        assert (st["at_best"][ex] >= 2).sum() >= 3
    if name == "borders":
        x, y, r = q["x"], q["y"], q["radius"]
        for inside, beyond in ((x < r, x < 0), (x > K.W - r, x > K.W), (y < r, y < 0),
                               (y > K.H - r, y > K.H)):
            assert (inside & ~beyond).sum() >= 3 and beyond.sum() >= 3
    if name == "ties":
        assert (st["lower_loser"] > 0).sum() >= 10
    if name == "gate":
        assert sorted(set(q["level"].tolist())) == [-1, 0, 1, 2, 3, 4, 5, 6, 7]
    if name == "max_n":
        assert len(kf["keys"]) == gpu.KFW_MAXN and len(q) == 64
    _compare(gpu.keyframe_search([kf], [q], qd)[0], bi, bd)


@pytest.mark.gpu
def test_max_n_plus_one_is_unsupported(gpu):
    kf, q, qd = case_max_n()
    big = K.frame_dict(np.concatenate([kf["keys"], kf["keys"][:1]]),
                       np.concatenate([kf["desc"], kf["desc"][:1]]))
    with pytest.raises(gpu.OrbxError) as e:
        gpu.keyframe_search([big], [q], qd)
    assert e.value.code == gpu.ERR_UNSUPPORTED


@pytest.mark.gpu
def test_batch_equals_restatement_and_one_call_per_problem(gpu):
    kfs, qs, pool = case_batch()
    want = K.ref_batch(kfs, qs, pool)
    bi = np.concatenate([w[0] for w in want])
    bd = np.concatenate([w[1] for w in want])
    st = {k: np.concatenate([w[2][k] for w in want]) for k in K.STAT_NAMES}
    allkeys = dict(keys=np.concatenate([k["keys"] for k in kfs]))
    K.assert_not_vacuous(allkeys, bi, bd, st)
    got = gpu.keyframe_search(kfs, qs, pool)
    assert len(got) == len(kfs)
    for p in range(len(kfs)):
        assert len(got[p][0]) == BATCH_NQ[p]
        _compare(got[p], want[p][0], want[p][1])
    # batched equals one call per problem
    for p in range(len(kfs)):
        one = gpu.keyframe_search([kfs[p]], [qs[p]], pool)[0]
        assert np.array_equal(one[0], got[p][0]) and np.array_equal(one[1], got[p][1])


@pytest.mark.gpu
def test_workspace_reuse_larger_then_smaller(gpu):
    kf, q, qd = case_many()
    bi, bd, _ = ref_of("many_queries")
    _compare(gpu.keyframe_search([kf], [q], qd)[0], bi, bd)
    kf2, q2, qd2 = case_ties()
    bi2, bd2, _ = ref_of("ties")
    _compare(gpu.keyframe_search([kf2], [q2[:37]], qd2)[0], bi2[:37], bd2[:37])
    _compare(gpu.keyframe_search([kf], [q], qd)[0], bi, bd)


@pytest.mark.gpu
def test_empty_shapes(gpu):
    kf, q, qd = case_ties()
    empty = K.frame_dict(np.zeros(0, K.KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8))
    assert gpu.keyframe_search([], [], qd) == []
    assert gpu.keyframe_search([], [], np.zeros((0, 32), np.uint8)) == []
    got = gpu.keyframe_search([empty], [q[:9]], qd)[0]
    assert got[0].tolist() == [-1] * 9 and got[1].tolist() == [K.INT_MAX] * 9
    got = gpu.keyframe_search([kf, empty, kf], [q[:0], q[:0], q[:0]], qd)
    assert [len(g[0]) for g in got] == [0, 0, 0]
    # a problem without queries between two with
    bi, bd, _ = ref_of("ties")
    got = gpu.keyframe_search([kf, kf, empty, kf], [q[:5], q[:0], q[:0], q[5:40]], qd)
    _compare(got[0], bi[:5], bd[:5])
    _compare(got[3], bi[5:40], bd[5:40])
    assert len(got[1][0]) == 0 and len(got[2][0]) == 0


def _raw(gpu, kf, q, qoff, qd, nprob=None, device=0):
    keep = []
    arr = (gpu.KfFrame * 1)(gpu.kf_struct(kf, keep))
    q = np.ascontiguousarray(q, gpu.KF_QUERY_DTYPE)
    qoff = np.ascontiguousarray(qoff, np.int32)
    bi = np.zeros(max(len(q), 1), np.int32)
    bd = np.zeros(max(len(q), 1), np.int32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    return gpu.lib().orbm_keyframe_search(1 if nprob is None else nprob, ctypes.cast(arr, ctypes.c_void_p),
                                          p(q), p(qoff), p(qd), len(qd), device, p(bi), p(bd))


@pytest.mark.gpu
def test_argument_errors_then_a_good_call(gpu):
    kf, q, qd = case_ties()
    q = q[:20].copy()
    ok = [0, 20]
    assert _raw(gpu, kf, q, ok, qd) == gpu.OK
    assert _raw(gpu, kf, q, ok, qd, nprob=-1) == gpu.ERR_ARG
    assert _raw(gpu, kf, q, [1, 20], qd) == gpu.ERR_ARG
    assert _raw(gpu, kf, q, [-1, 20], qd) == gpu.ERR_ARG
    assert _raw(gpu, kf, q, [0, -1], qd) == gpu.ERR_ARG
    for row in (-1, len(qd)):
        b = q.copy()
        b["desc"][7] = row
        assert _raw(gpu, kf, b, ok, qd) == gpu.ERR_ARG
    for field in ("x", "y", "radius"):
        for v in (np.nan, np.inf, -np.inf):
            b = q.copy()
            b[field][3] = v
            assert _raw(gpu, kf, b, ok, qd) == gpu.ERR_ARG
    assert _raw(gpu, kf, q, ok, qd, device=99) == gpu.ERR_NO_DEVICE
    assert _raw(gpu, kf, q, ok, qd, device=-1) == gpu.ERR_NO_DEVICE
    bi, bd, _ = ref_of("ties")
    _compare(gpu.keyframe_search([kf], [q], qd)[0], bi[:20], bd[:20])
