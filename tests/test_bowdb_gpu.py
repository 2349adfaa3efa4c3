"""orbv_score and the orbv_db_* keyframe database on the GPU, bit-equal to the
CPU restatement (tests/cpp/bowdb_ref.c): every supported scoring over the
chunk boundaries of the kernel (64 words per step), planted order-sensitive
values, the chi-square guard, the query's ids / order / counts / scores over
database sizes around a wavefront's worth of keyframes, erase / re-add / clear
histories, growth from one word and compaction, the argument checks and the
handle's resources."""
import ctypes
import functools
import gc

import numpy as np
import pytest

import bowdb_util as U
from orbx import synth

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def vocab(gpu, scoring):
    v = gpu.Vocabulary.from_records(synth.vocabulary(k=10, L=3), scoring=scoring)
    assert v.info()["nwords"] == U.NWORDS
    return v


def bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


def code_of(gpu, call):
    """the status a call raises (OK if none); unlike a kept pytest.raises
    result it leaves no reference cycle through the caller's frame, so the
    caller's handles go when it returns"""
    try:
        call()
    except gpu.OrbxError as ex:
        return ex.code
    return gpu.OK


def assert_scores_equal(got, want, what=""):
    assert np.array_equal(bits(got), bits(want)), (what, got, want)


# ------------------------------------------------------------------ orbv_score
@pytest.mark.parametrize("scoring", U.SCORINGS)
def test_score_lengths_and_placement(gpu, scoring):
    v = vocab(gpu, scoring)
    pairs = U.length_pairs()
    by_a = {}
    for a, b in pairs:  # one call per a: its nvec = len(LENGTHS) vectors
        by_a.setdefault(len(a[0]), (a, []))[1].append(b)
    nonzero = 0
    for na, (a, bs) in by_a.items():
        want = [U.ref_score(scoring, a, b) for b in bs]
        assert_scores_equal(v.score(a, bs), want, na)
        nonzero += sum(1 for w in want if w != 0)
    assert nonzero >= 30
    for name, (a, b) in U.placement_pairs().items():
        want = U.ref_score(scoring, a, b)
        ncommon = len(np.intersect1d(a[0], b[0]))
        assert ncommon == dict(disjoint=0, identical=150, first=1, last=1, chunk64=64)[name]
        assert_scores_equal(v.score(a, [b]), [want], name)
        assert_scores_equal(v.score(b, [a]), [U.ref_score(scoring, b, a)], name)


@pytest.mark.parametrize("nvec", [1, 4, 5, 300])
def test_score_vector_counts(gpu, nvec):
    v = vocab(gpu, 0)
    rng = np.random.default_rng(nvec)
    a = U.random_bow(rng, 90)
    bs = [U.random_bow(rng, int(rng.integers(0, 140))) for _ in range(nvec)]
    want = [U.ref_score(0, a, b) for b in bs]
    assert nvec == 1 or len(set(want)) > 1
    assert_scores_equal(v.score(a, bs), want)


@pytest.mark.parametrize("scoring", U.SCORINGS)
def test_score_planted_order_sensitive_values(gpu, scoring):
    a, b = U.planted_order_pair(scoring)
    want = U.ref_score(scoring, a, b)
    t = U.ref_terms(scoring, a, b)
    # on the CPU first: any other order of the same terms is another double
    assert U.close(scoring, U.sum_forward(t)) == want
    assert U.close(scoring, U.sum_reverse(t)) != want
    assert U.close(scoring, U.sum_tree(t)) != want
    if scoring in (1, 5):
        assert U.close(scoring, U.sum_fma(a, b)) != want
    assert_scores_equal(vocab(gpu, scoring).score(a, [b]), [want])


def test_score_chi_square_guard(gpu):
    a = U.bow([3, 8, 20, 77], [0.5, 0.25, 0.125, 0.75])
    b = U.bow([3, 8, 20, 90], [0.5, -0.25, 0.375, 0.1])
    assert len(U.ref_terms(2, a, b)) == 2  # word 8 is common and adds nothing
    want = U.ref_score(2, a, b)
    assert np.isfinite(want)
    assert_scores_equal(vocab(gpu, 2).score(a, [b]), [want])


@pytest.mark.parametrize("scoring", [3, 4])
def test_unsupported_scorings(gpu, scoring):
    v = vocab(gpu, scoring)
    a = U.bow([1, 2], [0.5, 0.5])
    assert code_of(gpu, lambda: v.score(a, [a])) == gpu.ERR_UNSUPPORTED
    assert code_of(gpu, lambda: gpu.KeyFrameDatabase(v)) == gpu.ERR_UNSUPPORTED


# --------------------------------------------------------------- orbv_db_query
def assert_query_equal(db, ref, q, what=""):
    ids, nc, sc = db.query(q)
    rids, rnc, rsc = ref.query(q)
    assert ids.tolist() == rids.tolist(), what
    assert nc.tolist() == rnc.tolist(), what
    assert_scores_equal(sc, rsc, what)
    return ids


QUERY = U.random_bow(np.random.default_rng(77), 40)


@functools.lru_cache(maxsize=None)
def keyframes(n):
    return U.random_keyframes(501 + n, n)  # the single keyframe of n = 1 shares a word with QUERY


@pytest.mark.parametrize("scoring", [0, 1])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
def test_query_parity(gpu, n, scoring):
    kfs = keyframes(n)
    ref = U.RefDb(U.NWORDS, scoring)
    for i, b in enumerate(kfs):
        ref.add(1000 + 3 * i, b)
    if n == 1:
        assert len(ref.query(QUERY)[0]) == 1
    if n == 200:  # on the restatement and the inputs alone, before the GPU is touched
        sharing, apart, groups = U.sharing_stats(kfs, QUERY)
        assert len(ref.query(QUERY)[0]) == sharing
        assert sharing >= 20 and apart >= 5 and groups >= 3, (sharing, apart, groups)
    db = gpu.KeyFrameDatabase(vocab(gpu, scoring))
    for i, b in enumerate(kfs):
        db.add(1000 + 3 * i, b)
    assert db.size() == n
    ids = assert_query_equal(db, ref, QUERY, n)
    if n == 200:
        assert len(ids) >= 20 and ids.tolist() != sorted(ids.tolist())
    assert_query_equal(db, ref, U.bow([], []), "empty query")
    assert len(db.query(U.bow([], []))[0]) == 0


def test_history(gpu):
    kfs = keyframes(200)
    group = U.tie_group(kfs, QUERY, 3)
    db, ref = gpu.KeyFrameDatabase(vocab(gpu, 0)), U.RefDb()
    assert len(db.query(QUERY)[0]) == 0  # empty database
    for i, b in enumerate(kfs):
        db.add(i, b)
        ref.add(i, b)
    before = assert_query_equal(db, ref, QUERY).tolist()
    mid = group[1]
    for d in (db, ref):
        d.erase(mid)
    gone = assert_query_equal(db, ref, QUERY, "erased").tolist()
    assert gone == [i for i in before if i != mid]
    for d in (db, ref):
        d.add(mid, kfs[mid])
    back = assert_query_equal(db, ref, QUERY, "re-added").tolist()
    tied = [i for i in back if i in group]
    assert tied == [g for g in group if g != mid] + [mid] and back != before  # to the back of its group
    for d in (db, ref):
        d.erase(123456)  # absent: a no-op
    assert db.size() == 200 and assert_query_equal(db, ref, QUERY).tolist() == back
    for d in (db, ref):
        d.clear()
    assert db.size() == 0 and len(assert_query_equal(db, ref, QUERY, "cleared")) == 0
    for d in (db, ref):
        d.add(5, kfs[group[0]])
    assert assert_query_equal(db, ref, QUERY, "after clear").tolist() == [5]


def test_growth_and_compaction(gpu):
    kfs = U.random_keyframes(900, 360)
    db = gpu.KeyFrameDatabase(vocab(gpu, 0), reserve_words=1)
    fresh = gpu.KeyFrameDatabase(vocab(gpu, 0))
    ref = U.RefDb()
    for i in range(300):
        db.add(i, kfs[i])
        ref.add(i, kfs[i])
    assert_query_equal(db, ref, QUERY, "grown")
    for i in range(300):
        if i % 3:
            db.erase(i)
            ref.erase(i)
    assert db.size() == 100
    left = assert_query_equal(db, ref, QUERY, "compacted")
    assert len(left) > 10
    for i in range(300, 360):
        db.add(i, kfs[i])
        ref.add(i, kfs[i])
    db.add(1, kfs[1])  # an erased id again: behind everything
    ref.add(1, kfs[1])
    assert_query_equal(db, ref, QUERY, "grown again")
    for i in list(range(0, 300, 3)) + list(range(300, 360)) + [1]:  # the surviving history
        fresh.add(i, kfs[i])
    for a, b in zip(db.query(QUERY), fresh.query(QUERY)):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_argument_checks(gpu):
    L, v = gpu.lib(), vocab(gpu, 0)
    db = gpu.KeyFrameDatabase(v)
    good = U.bow([3, 9, 500], [0.2, 0.3, 0.5])
    db.add(1, good)
    db.add(2, U.bow([9, 11], [0.5, 0.5]))
    for bad in (U.bow([3, 500, 9], [0.2, 0.3, 0.5]), U.bow([3, 3, 9], [0.2, 0.3, 0.5]),
                U.bow([3, 9, U.NWORDS], [0.2, 0.3, 0.5])):
        for call in (lambda: db.add(7, bad), lambda: db.query(bad), lambda: v.score(bad, [good]),
                     lambda: v.score(good, [good, bad])):
            assert code_of(gpu, call) == gpu.ERR_ARG
    assert code_of(gpu, lambda: db.add(1, good)) == gpu.ERR_ARG  # a duplicate id
    assert db.size() == 2
    # cap too small: the required count comes back
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    ids, nc, sc, n = np.zeros(2, np.uint64), np.zeros(2, np.int32), np.zeros(2, np.float64), ctypes.c_int(-1)
    q = U.bow([9], [1.0])
    assert L.orbv_db_query(db._h, p(q[0]), p(q[1]), 1, 1, p(ids), p(nc), p(sc), ctypes.byref(n)) == gpu.ERR_CAPACITY
    assert n.value == 2
    assert L.orbv_db_query(db._h, p(q[0]), p(q[1]), 1, 2, p(ids), p(nc), p(sc), ctypes.byref(n)) == gpu.OK
    assert n.value == 2 and ids.tolist() == [1, 2] and nc.tolist() == [1, 1]
    # over 8192 words (a vocabulary large enough to hold them)
    big = gpu.Vocabulary.from_records(synth.vocabulary(k=10, L=4))
    assert big.info()["nwords"] == 10000
    w = U.bow(np.arange(8193), np.full(8193, 1.0 / 8193))
    bdb = gpu.KeyFrameDatabase(big)
    for call in (lambda: bdb.add(1, w), lambda: bdb.query(w), lambda: big.score(w, [good]),
                 lambda: big.score(good, [w])):
        assert code_of(gpu, call) == gpu.ERR_UNSUPPORTED
    ok = U.bow(np.arange(8192), np.full(8192, 1.0 / 8192))  # the limit itself
    bdb.add(1, ok)
    ids, nc, sc = bdb.query(ok)
    assert ids.tolist() == [1] and nc.tolist() == [8192]
    assert_scores_equal(sc, [U.ref_score(0, ok, ok)])


# ------------------------------------------------------------------ the handle
def live(L):
    c = (ctypes.c_int * 4)()
    assert L.orbx_debug_live_resources(c) == 0
    return tuple(c)


def test_handle_round_trip(gpu):
    L, v = gpu.lib(), vocab(gpu, 0)
    gc.collect()  # earlier tests' handles held by reference cycles (pytest.raises) go now, not between the counts
    before = live(L)
    h = ctypes.c_void_p()
    assert L.orbv_db_create(v._h, 0, 0, ctypes.byref(h)) == gpu.OK and h.value
    made = live(L)
    assert made[0] == before[0] + 3 and made[2] == before[2] + 1  # words, values, slots; the stream
    assert L.orbv_db_destroy(h) == gpu.OK
    assert live(L) == before
    # with live keyframes, after growth, a compaction and a query
    assert L.orbv_db_create(v._h, 1, 0, ctypes.byref(h)) == gpu.OK
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for i, (w, x) in enumerate(keyframes(65)):
        assert L.orbv_db_add(h, i, p(w), p(x), len(w)) == gpu.OK
    for i in range(40):
        assert L.orbv_db_erase(h, i) == gpu.OK
    n = ctypes.c_int(-1)
    assert L.orbv_db_size(h, ctypes.byref(n)) == gpu.OK and n.value == 25
    ids, nc, sc = np.zeros(25, np.uint64), np.zeros(25, np.int32), np.zeros(25, np.float64)
    assert L.orbv_db_query(h, p(QUERY[0]), p(QUERY[1]), 40, 25, p(ids), p(nc), p(sc), ctypes.byref(n)) == gpu.OK
    assert n.value > 0
    assert live(L) == made  # growth and compaction replace buffers, they do not add any
    assert L.orbv_db_destroy(h) == gpu.OK
    assert live(L) == before
    assert L.orbv_db_destroy(None) == gpu.OK
    assert L.orbv_db_create(None, 0, 0, ctypes.byref(h)) == gpu.ERR_ARG and not h.value
