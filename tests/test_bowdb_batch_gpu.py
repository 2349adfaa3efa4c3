"""orbv_db_query_batch and orbv_db_query_batch_device on the GPU: every segment
of a batched call equal to the CPU restatement (tests/cpp/bowdb_ref.c, one
query at a time) and, byte for byte, to orbv_db_query on the same handle --
over database sizes around the wavefront and the order kernel's tile (256
slots), planted bins, the word gate, erase / re-add / clear / growth /
compaction histories, the argument checks, the device form (rows with garbage
beyond n, a small cap, a refused row, a non-default stream, the chain from
orbv_transform_batch, the ordering against a store that grows) and the
handle's resources."""
import ctypes
import functools
import gc

import numpy as np
import pytest

import bowdb_util as U
from orbx import synth

pytestmark = pytest.mark.gpu

SIZES = (1, 63, 64, 65, 200, 255, 256, 257, 1023, 1024, 1025, 2500)
KF_WORDS_BELOW = 900  # keyframes draw their words below this; the words above share nothing


@functools.lru_cache(maxsize=None)
def vocab(gpu, scoring):
    v = gpu.Vocabulary.from_records(synth.vocabulary(k=10, L=3), scoring=scoring)
    assert v.info()["nwords"] == U.NWORDS
    return v


@functools.lru_cache(maxsize=None)
def big_vocab(gpu):
    v = gpu.Vocabulary.from_records(synth.vocabulary(k=10, L=4))
    assert v.info()["nwords"] == 10000
    return v


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def code_of(gpu, call):
    try:
        call()
    except gpu.OrbxError as ex:
        return ex.code
    return gpu.OK


def p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@functools.lru_cache(maxsize=None)
def keyframes(n):
    return U.random_keyframes(7000 + n, n, 40, KF_WORDS_BELOW)


@functools.lru_cache(maxsize=None)
def queries(n):
    """the six queries of one call, for the database of n keyframes"""
    rng = np.random.default_rng(31 + n)
    q0 = U.random_bow(rng, 40, KF_WORDS_BELOW)
    if n == 1:  # the single keyframe shares two words with it
        kw = keyframes(1)[0][0]
        rest = rng.choice(np.setdiff1d(np.arange(KF_WORDS_BELOW), kw), 38, replace=False)
        q0 = (np.union1d(rest, kw[:2]).astype(np.uint32), q0[1])
    one = U.bow([keyframes(n)[0][0][5]], [0.75])
    apart = np.sort(rng.choice(np.arange(KF_WORDS_BELOW, U.NWORDS), 30, replace=False)).astype(np.uint32)
    return [q0, U.bow([], []), one, U.random_bow(rng, 257), (apart, rng.uniform(0.01, 1.0, 30)),
            (q0[0].copy(), q0[1].copy())]


def gate_filter(ids, nc, sc):
    if len(nc) == 0:
        return ids, nc, sc
    keep = nc > int(np.float32(nc.max()) * np.float32(0.8))
    return ids[keep], nc[keep], sc[keep]


def assert_segment(got, want, what):
    assert got[0].tolist() == want[0].tolist(), what
    assert got[1].tolist() == want[1].tolist(), what
    assert np.array_equal(bits(got[2]), bits(want[2])), what


def assert_batch_equal(db, ref, qs, what="", gated=False, single=True):
    """one batched call against the restatement and (ungated) orbv_db_query; the segments"""
    res = db.query_batch(qs, gated=gated)
    assert len(res) == len(qs)
    for i, q in enumerate(qs):
        want = ref.query(q)
        if gated:
            want = gate_filter(*want)
        assert_segment(res[i], want, (what, i))
        if single and not gated:
            for a, b in zip(res[i], db.query(q)):
                assert a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, i)
    return res


def filled(kfs, scoring, gpu, ids=None, **kw):
    db, ref = gpu.KeyFrameDatabase(vocab(gpu, scoring), **kw), U.RefDb(U.NWORDS, scoring)
    for i, b in enumerate(kfs):
        kid = ids[i] if ids is not None else 1000 + 3 * i
        db.add(kid, b)
        ref.add(kid, b)
    return db, ref


# ------------------------------------------------------------------ parity over sizes
@pytest.mark.parametrize("n,scoring", [(n, 0) for n in SIZES] + [(65, 1), (1025, 1)])
def test_batch_parity(gpu, n, scoring):
    kfs, qs = keyframes(n), queries(n)
    ref = U.RefDb(U.NWORDS, scoring)
    for i, b in enumerate(kfs):
        ref.add(1000 + 3 * i, b)
    # on the inputs and the restatement alone, before the GPU is touched
    assert [len(q[0]) for q in qs] == [len(qs[0][0]), 0, 1, 257, 30, len(qs[0][0])]
    assert len(ref.query(qs[4])[0]) == 0 and len(ref.query(qs[2])[0]) >= 1 and len(ref.query(qs[0])[0]) >= 1
    if n >= 200:
        sharing, apart, groups = U.sharing_stats(kfs, qs[0])
        ids = ref.query(qs[0])[0].tolist()
        assert len(ids) == sharing
        assert sharing >= 20 and apart >= 5 and groups >= 3, (sharing, apart, groups)
        assert ids != sorted(ids)
    db = gpu.KeyFrameDatabase(vocab(gpu, scoring))
    for i, b in enumerate(kfs):
        db.add(1000 + 3 * i, b)
    res = assert_batch_equal(db, ref, qs, n)
    assert len(res[1][0]) == 0 and len(res[4][0]) == 0
    assert_segment(res[5], res[0], "the first query again")


def test_more_queries_than_a_grid_dimension(gpu):
    """beyond 65,535 queries a workgroup takes several: every segment is still its own query's"""
    kfs = keyframes(63)[:6]
    db, ref = filled(kfs, 0, gpu)
    mix = np.union1d(kfs[1][0][30:], kfs[5][0][:4]).astype(np.uint32)
    base = [(kfs[0][0][:7].copy(), kfs[0][1][:7].copy()), U.bow([kfs[3][0][2]], [0.5]), U.bow([], []),
            (mix, np.full(len(mix), 0.125))]
    want = [ref.query(q) for q in base]
    assert [len(x[0]) >= 1 for x in want] == [True, True, False, True] and len({tuple(x[0].tolist()) for x in want}) >= 3
    nq = 65535 + 70
    res = db.query_batch([base[i % 4] for i in range(nq)], gated=False)
    assert len(res) == nq
    for i in list(range(0, nq, 97)) + list(range(65500, nq)):
        assert_segment(res[i], want[i % 4], i)
    counts = np.array([len(r[0]) for r in res])
    assert np.array_equal(counts, np.array([len(want[i % 4][0]) for i in range(nq)]))


# ------------------------------------------------------------------ planted bins
def test_planted_bins(gpu):
    rng = np.random.default_rng(5)
    qw = (5 * np.arange(40) + 3).astype(np.uint32)  # 3 .. 198
    q = (qw, rng.uniform(0.01, 1.0, 40))
    other = np.setdiff1d(np.arange(200, KF_WORDS_BELOW), qw)

    def kf(common):
        w = np.sort(np.concatenate([common, rng.choice(other, 20, replace=False)])).astype(np.uint32)
        return w, rng.uniform(0.01, 1.0, len(w))

    kfs = [kf([3]) for _ in range(300)]                 # one bin, longer than any tile
    kfs += [kf([198]) for _ in range(20)]               # only the query's last word
    kfs += [kf([]) for _ in range(10)]                  # nothing
    kfs += [kf([3, 198]) for _ in range(5)]             # the first bin again, added last
    ids = list(range(len(kfs)))
    db, ref = filled(kfs, 0, gpu, ids)
    first_bin = list(range(300)) + list(range(330, 335))
    want = first_bin + list(range(300, 320))
    assert ref.query(q)[0].tolist() == want             # on the restatement alone
    res = assert_batch_equal(db, ref, [q, q], "planted")
    assert res[0][0].tolist() == want
    for d in (db, ref):
        d.erase(150)
        d.add(150, kfs[150])
    want = [i for i in first_bin if i != 150] + [150] + list(range(300, 320))
    assert ref.query(q)[0].tolist() == want
    res = assert_batch_equal(db, ref, [q, U.bow([198], [0.5]), q], "to the back of the bin")
    assert res[0][0].tolist() == want
    assert res[1][0].tolist() == list(range(300, 320)) + list(range(330, 335))


def test_rank_limits_of_the_longest_query(gpu):
    rng = np.random.default_rng(6)
    qw = np.arange(1000, 1000 + 8192, dtype=np.uint32)  # the limit: ranks 0 .. 8191
    q = (qw, np.full(8192, 1.0 / 8192))
    outside = np.concatenate([np.arange(0, 1000), np.arange(9192, 10000)])

    def kf(common):
        w = np.sort(np.concatenate([common, rng.choice(outside, 12, replace=False)])).astype(np.uint32)
        return w, rng.uniform(0.01, 1.0, len(w))

    kfs = [kf([qw[-1]]) if i % 2 == 0 else kf([qw[0]]) for i in range(12)] + [kf([]), kf([qw[0], qw[-1]]), kf([qw[4000]])]
    db, ref = gpu.KeyFrameDatabase(big_vocab(gpu)), U.RefDb(10000, 0)
    for i, b in enumerate(kfs):
        db.add(i, b)
        ref.add(i, b)
    want = [1, 3, 5, 7, 9, 11, 13, 14, 0, 2, 4, 6, 8, 10]
    assert ref.query(q)[0].tolist() == want
    res = assert_batch_equal(db, ref, [q, U.bow([qw[-1]], [1.0]), q], "rank 0 and rank 8191")
    assert res[0][0].tolist() == want and res[0][1].tolist() == [1] * 6 + [2, 1] + [1] * 6


# ------------------------------------------------------------------ the gate
def test_gate(gpu):
    n = 257
    kfs, qs = list(keyframes(n)), queries(n)
    rng = np.random.default_rng(8)
    # three keyframes close to the first query, so that its gate keeps several
    for take in (36, 34, 33):
        w = np.sort(rng.choice(qs[0][0], take, replace=False)).astype(np.uint32)
        kfs.insert(int(rng.integers(50, 200)), (w, rng.uniform(0.01, 1.0, take)))
    db, ref = filled(kfs, 0, gpu)
    lost = kept2 = 0
    for q in qs:  # on the restatement alone
        full = ref.query(q)
        g = gate_filter(*full)
        lost += len(g[0]) < len(full[0])
        kept2 += len(g[0]) < len(full[0]) and len(g[0]) >= 2
    assert lost >= 2 and kept2 >= 1
    assert_batch_equal(db, ref, qs, "gated", gated=True)
    assert_batch_equal(db, ref, qs, "ungated after gated")


def test_gate_whole_number_products(gpu):
    """maxima 5 and 10: 5 * 0.8f and 10 * 0.8f are 4 and 8 after the float
    rounding, and the gate is a strict comparison"""
    assert int(np.float32(5) * np.float32(0.8)) == 4 and int(np.float32(10) * np.float32(0.8)) == 8
    rng = np.random.default_rng(9)
    qa = (np.arange(10, 30, dtype=np.uint32), rng.uniform(0.01, 1.0, 20))
    qb = (np.arange(110, 130, dtype=np.uint32), rng.uniform(0.01, 1.0, 20))
    other = np.arange(300, KF_WORDS_BELOW)
    kfs, counts = [], []
    for base, top in ((10, 5), (110, 10)):
        for k in list(range(1, top + 1)) * 2:
            common = base + rng.choice(20, k, replace=False)
            w = np.sort(np.concatenate([common, rng.choice(other, 10, replace=False)])).astype(np.uint32)
            kfs.append((w, rng.uniform(0.01, 1.0, len(w))))
            counts.append((base, k))
    order = rng.permutation(len(kfs))
    kfs, counts = [kfs[i] for i in order], [counts[i] for i in order]
    db, ref = filled(kfs, 0, gpu, list(range(len(kfs))))
    res = assert_batch_equal(db, ref, [qa, qb], "5 and 10", gated=True)
    assert sorted(res[0][1].tolist()) == [5, 5]
    assert sorted(res[1][1].tolist()) == [9, 9, 10, 10]
    assert sorted(res[0][0].tolist()) == [i for i, c in enumerate(counts) if c == (10, 5)]
    assert sorted(res[1][0].tolist()) == [i for i, c in enumerate(counts) if c[0] == 110 and c[1] > 8]
    full = assert_batch_equal(db, ref, [qa, qb], "5 and 10, all")
    assert len(full[0][0]) == 10 and len(full[1][0]) == 20


# ------------------------------------------------------------------ histories
def test_batch_history(gpu):
    kfs, qs = keyframes(200), queries(200)
    group = U.tie_group(kfs, qs[0], 3)
    db, ref = gpu.KeyFrameDatabase(vocab(gpu, 0)), U.RefDb()
    assert all(len(s[0]) == 0 for s in assert_batch_equal(db, ref, qs, "empty database"))
    for i, b in enumerate(kfs):
        db.add(i, b)
        ref.add(i, b)
    before = assert_batch_equal(db, ref, qs, "filled")[0][0].tolist()
    mid = group[1]
    for d in (db, ref):
        d.erase(mid)
    res = assert_batch_equal(db, ref, qs, "erased")  # a dead slot in the middle
    assert all(mid not in s[0].tolist() for s in res)
    assert res[0][0].tolist() == [i for i in before if i != mid]
    for d in (db, ref):
        d.add(mid, kfs[mid])
    back = assert_batch_equal(db, ref, qs, "re-added")[0][0].tolist()
    tied = [i for i in back if i in group]
    assert tied == [g for g in group if g != mid] + [mid] and back != before
    for d in (db, ref):
        d.erase(123456)  # absent
    assert assert_batch_equal(db, ref, qs, "absent erased")[0][0].tolist() == back
    for d in (db, ref):
        d.clear()
    assert all(len(s[0]) == 0 for s in assert_batch_equal(db, ref, qs, "cleared"))
    for d in (db, ref):
        d.add(5, kfs[group[0]])
    assert assert_batch_equal(db, ref, qs, "after clear")[0][0].tolist() == [5]


def test_batch_growth_and_compaction(gpu):
    kfs = U.random_keyframes(900, 360, 40, KF_WORDS_BELOW)
    qs = queries(257)
    db = gpu.KeyFrameDatabase(vocab(gpu, 0), reserve_words=1)
    ref = U.RefDb()
    for i in range(300):
        db.add(i, kfs[i])
        ref.add(i, kfs[i])
    assert_batch_equal(db, ref, qs, "grown")
    for i in range(300):
        if i % 3 == 1:
            db.erase(i)
            ref.erase(i)
    res = assert_batch_equal(db, ref, qs, "dead slots in the middle")  # 100 tombstones, not compacted yet
    assert len(res[0][0]) > 20 and all(i % 3 != 1 for s in res for i in s[0].tolist())
    for i in range(300):
        if i % 3 == 2:
            db.erase(i)
            ref.erase(i)
    assert db.size() == 100
    left = assert_batch_equal(db, ref, qs, "compacted")[0][0]
    assert len(left) > 10
    for i in range(300, 360):
        db.add(i, kfs[i])
        ref.add(i, kfs[i])
    db.add(1, kfs[1])  # an erased id again: behind everything
    ref.add(1, kfs[1])
    assert_batch_equal(db, ref, qs, "grown again")


# ------------------------------------------------------------------ arguments
def raw_batch(gpu, h, qs, flags=0, cap=None, off=None, outs=True, nq=None):
    """orbv_db_query_batch as it stands; -> (status, out_off, ids, nc, sc)"""
    qs = [U.bow(*q) for q in qs]
    o = np.zeros(len(qs) + 1, np.uint32)
    o[1:] = np.cumsum([len(w) for w, _ in qs])
    if off is not None:
        o = np.asarray(off, np.uint32)
    qw = np.concatenate([w for w, _ in qs] + [np.zeros(1, np.uint32)])
    qv = np.concatenate([v for _, v in qs] + [np.zeros(1, np.float64)])
    cap = 64 if cap is None else cap
    out = np.full(len(o) + 1, 0xABCD, np.uint32)
    ids, nc, sc = np.full(max(cap, 1), 77, np.uint64), np.full(max(cap, 1), 77, np.int32), np.full(max(cap, 1), 77.0)
    rc = gpu.lib().orbv_db_query_batch(h, len(o) - 1 if nq is None else nq, p(o), p(qw), p(qv), flags, cap, p(out),
                                       p(ids) if outs else None, p(nc) if outs else None, p(sc) if outs else None)
    return rc, out, ids, nc, sc


def test_batch_argument_checks(gpu):
    v = vocab(gpu, 0)
    db = gpu.KeyFrameDatabase(v)
    good = U.bow([3, 9, 500], [0.2, 0.3, 0.5])
    db.add(1, good)
    db.add(2, U.bow([9, 11], [0.5, 0.5]))
    db.add(3, U.bow([11, 500], [0.5, 0.5]))
    h = db._h
    st = lambda *a, **k: raw_batch(gpu, *a, **k)[0]
    assert st(h, [good, good]) == gpu.OK
    assert st(None, [good]) == gpu.ERR_ARG
    assert st(h, [good], nq=-1) == gpu.ERR_ARG
    assert st(h, [good], cap=-1) == gpu.ERR_ARG
    assert st(h, [good], flags=2) == gpu.ERR_ARG and st(h, [good], flags=3) == gpu.ERR_ARG
    assert st(h, [good, good], off=[1, 3, 6]) == gpu.ERR_ARG   # q_off[0] != 0
    assert st(h, [good, good], off=[0, 4, 3]) == gpu.ERR_ARG   # descending
    for bad in (U.bow([3, 500, 9], [0.2, 0.3, 0.5]), U.bow([3, 3, 9], [0.2, 0.3, 0.5]),
                U.bow([3, 9, U.NWORDS], [0.2, 0.3, 0.5])):
        assert st(h, [good, bad]) == gpu.ERR_ARG and st(h, [bad, good]) == gpu.ERR_ARG
    assert st(h, [good], outs=False) == gpu.ERR_ARG            # entries are due
    assert st(h, [U.bow([700], [1.0])], outs=False) == gpu.OK  # none are
    # nq == 0, and empty queries: out_off is still filled
    rc, out, _, _, _ = raw_batch(gpu, h, [])
    assert rc == gpu.OK and out[0] == 0
    rc, out, ids, _, _ = raw_batch(gpu, h, [U.bow([], []), U.bow([], [])])
    assert rc == gpu.OK and out[:3].tolist() == [0, 0, 0] and ids[0] == 77
    # capacity: the exact offsets come back and no entry is written
    qs = [U.bow([9], [1.0]), U.bow([], []), U.bow([3, 11, 500], [0.3, 0.3, 0.4])]
    rc, out, ids, nc, sc = raw_batch(gpu, h, qs, cap=4)
    assert rc == gpu.ERR_CAPACITY and out[:4].tolist() == [0, 2, 2, 5]
    assert set(ids.tolist()) == {77} and set(nc.tolist()) == {77} and set(sc.tolist()) == {77.0}
    rc, out, ids, nc, sc = raw_batch(gpu, h, qs, cap=int(out[3]))
    assert rc == gpu.OK and out[:4].tolist() == [0, 2, 2, 5]
    assert ids.tolist() == [1, 2, 1, 2, 3] and nc.tolist() == [1, 1, 2, 1, 2]
    got = db.query_batch(qs)  # the binding's retry does the same
    assert [s[0].tolist() for s in got] == [[1, 2], [], [1, 2, 3]]
    # over 8192 words in one query
    bdb = gpu.KeyFrameDatabase(big_vocab(gpu))
    bdb.add(1, good)
    w = U.bow(np.arange(8193), np.full(8193, 1.0 / 8193))
    assert code_of(gpu, lambda: bdb.query_batch([good, w])) == gpu.ERR_UNSUPPORTED
    # nq * slots >= 2^31: 2500 slots and empty queries
    kfs = keyframes(2500)
    wide = gpu.KeyFrameDatabase(v)
    for i, b in enumerate(kfs):
        wide.add(i, b)
    nq = (1 << 31) // 2500 + 1
    assert nq * 2500 >= 1 << 31 > (nq - 1) * 2500
    off = np.zeros(nq + 1, np.uint32)
    out = np.zeros(nq + 1, np.uint32)
    one = np.zeros(1, np.uint32)
    L = gpu.lib()
    assert L.orbv_db_query_batch(wide._h, nq, p(off), p(one), p(one), 0, 0, p(out), None, None, None) == gpu.ERR_UNSUPPORTED
    assert L.orbv_db_query_batch(wide._h, nq - 1, p(off), p(one), p(one), 0, 0, p(out), None, None, None) == gpu.OK


# ------------------------------------------------------------------ the device form
def rows(torch, qs, qstride, seed=3):
    """the queries as [nq][qstride] tensors with garbage beyond n"""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 31, (len(qs), qstride)).astype(np.int32)
    v = rng.uniform(-5, 5, (len(qs), qstride))
    n = np.zeros(len(qs), np.int32)
    for i, (qw, qv) in enumerate(qs):
        w[i, :len(qw)] = qw.astype(np.int32)
        v[i, :len(qw)] = qv
        n[i] = len(qw)
    return torch.from_numpy(w).cuda(), torch.from_numpy(v).cuda(), torch.from_numpy(n).cuda()


def sentinel_outputs(torch, nq, cap):
    return dict(kf_id=torch.full((nq, cap), -7, dtype=torch.int64, device="cuda"),
                ncommon=torch.full((nq, cap), -7, dtype=torch.int32, device="cuda"),
                score=torch.full((nq, cap), -7.0, dtype=torch.float64, device="cuda"),
                nsharing=torch.full((nq,), -7, dtype=torch.int32, device="cuda"))


def host_of(o):
    return {k: t.cpu().numpy() for k, t in o.items()}


def close_l2(scoring, s):
    s = np.asarray(s, np.float64)
    if scoring != 1:
        return s
    return np.array([1.0 if x >= 1 else 1.0 - np.sqrt(1.0 - x) for x in s], np.float64)


def assert_rows_equal(o, want, cap, scoring=0, untouched=()):
    for i, (ids, nc, sc) in enumerate(want):
        if i in untouched:
            assert o["nsharing"][i] == -1
            assert (o["kf_id"][i] == -7).all() and (o["ncommon"][i] == -7).all() and (o["score"][i] == -7.0).all()
            continue
        k = min(len(ids), cap)
        assert o["nsharing"][i] == len(ids), i
        assert o["kf_id"][i, :k].astype(np.uint64).tolist() == ids[:k].tolist(), i
        assert o["ncommon"][i, :k].tolist() == nc[:k].tolist(), i
        assert np.array_equal(bits(close_l2(scoring, o["score"][i, :k])), bits(sc[:k])), i
        assert (o["kf_id"][i, k:] == -7).all() and (o["score"][i, k:] == -7.0).all()  # beyond: not written


@pytest.mark.parametrize("n,scoring,gated", [(257, 0, False), (1025, 1, False), (257, 0, True)])
def test_device_form(gpu, n, scoring, gated):
    import torch
    kfs, qs = keyframes(n), queries(n)
    db, ref = filled(kfs, scoring, gpu)
    want = db.query_batch(qs, gated=gated)
    for i, q in enumerate(qs):  # the host form is the restatement (test_batch_parity); here once more
        r = ref.query(q)
        assert_segment(want[i], gate_filter(*r) if gated else r, i)
    w, v, cnt = rows(torch, qs, 260)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    # ample cap, on a stream of its own
    o = db.query_batch_device_into(w, v, cnt, sentinel_outputs(torch, len(qs), n), gated=gated, stream=s)
    s.synchronize()
    assert_rows_equal(host_of(o), want, n, scoring)
    # cap below the longest row's count: the full count, the first cap entries
    small = max(len(x[0]) for x in want) // 2
    assert small >= 1
    o = db.query_batch_device_into(w, v, cnt, sentinel_outputs(torch, len(qs), small), gated=gated, stream=s)
    s.synchronize()
    assert_rows_equal(host_of(o), want, small, scoring)
    # n[q] > qstride: -1 and the row as it was; n[q] < 0: empty
    cnt2 = cnt.clone()
    cnt2[3] = 261
    cnt2[2] = -4
    o = db.query_batch_device_into(w, v, cnt2, sentinel_outputs(torch, len(qs), n), gated=gated)
    torch.cuda.synchronize()
    empty = (np.zeros(0, np.uint64), np.zeros(0, np.int32), np.zeros(0))
    assert_rows_equal(host_of(o), want[:2] + [empty] + want[3:], n, scoring, untouched=(3,))
    # the allocating binding
    o = host_of(db.query_batch_device(w, v, cnt, 16, gated=gated))
    torch.cuda.synchronize()
    assert o["nsharing"].tolist() == [len(x[0]) for x in want] and o["kf_id"].shape == (len(qs), 16)
    assert code_of(gpu, lambda: db.query_batch_device(torch.zeros((1, 8193), dtype=torch.int32, device="cuda"),
                                                      torch.zeros((1, 8193), dtype=torch.float64, device="cuda"),
                                                      cnt[:1], 4)) == gpu.ERR_UNSUPPORTED


def test_device_form_on_an_empty_database(gpu):
    import torch
    qs = queries(65)
    w, v, cnt = rows(torch, qs, 260)
    cnt[3] = 300  # refused whatever the database holds
    db = gpu.KeyFrameDatabase(vocab(gpu, 0))
    empty = (np.zeros(0, np.uint64), np.zeros(0, np.int32), np.zeros(0))
    for step in range(2):  # never filled; filled and cleared (slots gone, the table to upload)
        o = db.query_batch_device_into(w, v, cnt, sentinel_outputs(torch, len(qs), 8))
        torch.cuda.synchronize()
        assert_rows_equal(host_of(o), [empty] * len(qs), 8, untouched=(3,))
        for i, b in enumerate(keyframes(65)):
            db.add(i, b)
        db.clear()
    assert db.size() == 0 and all(len(s[0]) == 0 for s in db.query_batch(qs))


def test_chain_from_transform_batch(gpu):
    import torch
    voc = vocab(gpu, 0)
    rng = np.random.default_rng(12)
    db = gpu.KeyFrameDatabase(voc)
    for i in range(120):
        bowv, _ = voc.transform(rng.integers(0, 256, (48, 32), dtype=np.uint8), 2)
        db.add(i, bowv)
    B, kcap = 5, 64
    desc = rng.integers(0, 256, (B, kcap, 32), dtype=np.uint8)
    counts = np.array([64, 50, 0, 7, 64], np.int32)
    t = voc.transform_batch(torch.from_numpy(desc).cuda(), torch.from_numpy(counts).cuda(), 2)
    o = db.query_batch_device(t["bow_word"], t["bow_value"], t["nbow"], 120)
    voc.check()
    torch.cuda.synchronize()
    o = host_of(o)
    total = 0
    for f in range(B):
        bowv, _ = voc.transform(desc[f, :counts[f]], 2)
        ids, nc, sc = db.query(bowv)
        k = len(ids)
        total += k
        assert o["nsharing"][f] == k
        assert o["kf_id"][f, :k].astype(np.uint64).tolist() == ids.tolist()
        assert o["ncommon"][f, :k].tolist() == nc.tolist()
        assert np.array_equal(bits(o["score"][f, :k]), bits(sc))
    assert total > 100 and o["nsharing"][2] == 0


def test_device_form_ordering_against_a_growing_store(gpu):
    import torch
    kfs, qs = keyframes(257), queries(257)
    db, ref = filled(kfs, 0, gpu, reserve_words=1)
    want = [ref.query(q) for q in qs]
    extra = (np.union1d(qs[0][0][:3], kfs[0][0]).astype(np.uint32), None)
    extra = (extra[0], np.full(len(extra[0]), 0.01))
    w, v, cnt = rows(torch, qs, 260)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    o = db.query_batch_device_into(w, v, cnt, sentinel_outputs(torch, len(qs), 300), stream=s)
    for k in range(300):  # at once: adds that force the store to grow (10280 words so far, 16384 held)
        db.add(50000 + k, extra)
    s.synchronize()
    assert_rows_equal(host_of(o), want, 300)
    for k in range(300):
        ref.add(50000 + k, extra)
    after = ref.query(qs[0])
    assert len(after[0]) == len(want[0][0]) + 300
    o = db.query_batch_device_into(w, v, cnt, sentinel_outputs(torch, len(qs), 600), stream=s)
    s.synchronize()
    assert_rows_equal(host_of(o), [ref.query(q) for q in qs], 600)
    assert_batch_equal(db, ref, qs, "the host form after the device form")


# ------------------------------------------------------------------ the handle
def live(L):
    c = (ctypes.c_int * 4)()
    assert L.orbx_debug_live_resources(c) == 0
    return tuple(c)


def test_batch_handle_round_trip(gpu):
    import torch
    L, v = gpu.lib(), vocab(gpu, 0)
    kfs, qs = keyframes(65), queries(65)
    w, x, cnt = rows(torch, qs, 260)
    outs = sentinel_outputs(torch, len(qs), 65)
    db = gpu.KeyFrameDatabase(v)  # the call arenas of the process are warm after this one
    db.add(1, kfs[0])
    db.query_batch(qs)
    del db
    gc.collect()
    torch.cuda.synchronize()
    before = live(L)
    h = ctypes.c_void_p()
    assert L.orbv_db_create(v._h, 0, 0, ctypes.byref(h)) == gpu.OK and h.value
    made = live(L)
    assert made[0] == before[0] + 3 and made[2] == before[2] + 1 and made[3] == before[3]
    for i, (kw, kv) in enumerate(kfs):
        assert L.orbv_db_add(h, i, p(kw), p(kv), len(kw)) == gpu.OK
    assert raw_batch(gpu, h, qs, cap=400)[0] == gpu.OK
    first = live(L)
    assert first[0] == made[0] + 1 and first[3] == made[3] + 1 and first[2] == made[2]  # the records, the event
    s = torch.cuda.current_stream().cuda_stream
    dev = lambda: L.orbv_db_query_batch_device(h, len(qs), w.data_ptr(), x.data_ptr(), cnt.data_ptr(), 260, 0, 65,
                                               outs["kf_id"].data_ptr(), outs["ncommon"].data_ptr(),
                                               outs["score"].data_ptr(), outs["nsharing"].data_ptr(), s)
    assert dev() == gpu.OK and live(L) == first
    assert raw_batch(gpu, h, qs, cap=400)[0] == gpu.OK and dev() == gpu.OK
    assert live(L) == first  # a second call of the same size acquires nothing
    assert L.orbv_db_destroy(h) == gpu.OK  # with the device form's work in flight
    assert live(L) == before
