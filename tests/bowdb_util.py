"""Shared by the DBoW2 score / KeyFrameDatabase tests: the CPU restatement
(tests/cpp/bowdb_ref.c, built once per process with gcc and loaded with
ctypes), the random and planted BowVectors, other summation orders of the same
terms, and the non-vacuity checks.  No GPU, no orbx import."""
import ctypes
import functools
from fractions import Fraction

import numpy as np

import native
from native import ROOT, ptr as _ptr  # noqa: F401

SCORINGS = (0, 1, 2, 5)  # L1_NORM, L2_NORM, CHI_SQUARE, DOT_PRODUCT
NWORDS = 1000            # synth.vocabulary(k=10, L=3)
# seeds of planted_order_pair's inexact terms, per scoring: the first for which
# the other summation orders all give another double (the tests assert it)
PLANT_SEED = {0: 0, 1: 182, 2: 2, 5: 0}  # L2's closing sqrt hides most one-ulp differences of the sum


@functools.lru_cache(maxsize=None)
def ref_lib():
    lib = native.ref_lib("bowdb_ref.c")
    vp, ci, u64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint64
    lib.bowref_score.restype, lib.bowref_score.argtypes = ctypes.c_double, [ci, vp, vp, ci, vp, vp, ci]
    lib.bowref_terms.restype, lib.bowref_terms.argtypes = ci, [ci, vp, vp, ci, vp, vp, ci, vp]
    lib.bowref_db_create.restype, lib.bowref_db_create.argtypes = vp, [ctypes.c_uint32, ci]
    lib.bowref_db_add.restype, lib.bowref_db_add.argtypes = ci, [vp, u64, vp, vp, ci]
    lib.bowref_db_erase.restype, lib.bowref_db_erase.argtypes = ci, [vp, u64]
    lib.bowref_db_clear.restype, lib.bowref_db_clear.argtypes = None, [vp]
    lib.bowref_db_destroy.restype, lib.bowref_db_destroy.argtypes = None, [vp]
    lib.bowref_db_size.restype, lib.bowref_db_size.argtypes = ci, [vp]
    lib.bowref_db_query.restype, lib.bowref_db_query.argtypes = ci, [vp, vp, vp, ci, ci, vp, vp, vp]
    return lib


def bow(words, values):
    return np.ascontiguousarray(words, np.uint32), np.ascontiguousarray(values, np.float64)


def ref_score(scoring, a, b):
    (aw, av), (bw, bv) = bow(*a), bow(*b)
    return ref_lib().bowref_score(scoring, _ptr(aw), _ptr(av), len(aw), _ptr(bw), _ptr(bv), len(bw))


def ref_terms(scoring, a, b):
    """the terms of the restatement's sum, in its order"""
    (aw, av), (bw, bv) = bow(*a), bow(*b)
    t = np.zeros(max(min(len(aw), len(bw)), 1), np.float64)
    n = ref_lib().bowref_terms(scoring, _ptr(aw), _ptr(av), len(aw), _ptr(bw), _ptr(bv), len(bw), _ptr(t))
    return t[:n]


class RefDb:
    """the restatement's literal inverted file"""

    def __init__(self, nwords=NWORDS, scoring=0):
        self._lib = ref_lib()  # held: __del__ may run while the module is torn down
        self._h = self._lib.bowref_db_create(nwords, scoring)

    def __del__(self):
        if getattr(self, "_h", None):
            self._lib.bowref_db_destroy(self._h)
            self._h = None

    def add(self, kf_id, b):
        w, v = bow(*b)
        assert ref_lib().bowref_db_add(self._h, kf_id, _ptr(w), _ptr(v), len(w)) == 0

    def erase(self, kf_id):
        return ref_lib().bowref_db_erase(self._h, kf_id)

    def clear(self):
        ref_lib().bowref_db_clear(self._h)

    def size(self):
        return ref_lib().bowref_db_size(self._h)

    def query(self, b):
        w, v = bow(*b)
        cap = max(self.size(), 1)
        ids, nc, sc = np.zeros(cap, np.uint64), np.zeros(cap, np.int32), np.zeros(cap, np.float64)
        n = ref_lib().bowref_db_query(self._h, _ptr(w), _ptr(v), len(w), cap, _ptr(ids), _ptr(nc), _ptr(sc))
        return ids[:n].copy(), nc[:n].copy(), sc[:n].copy()


# --------------------------------------------------------------------------- inputs
def random_bow(rng, n, nwords=NWORDS, signed=False):
    """n distinct words below nwords, ascending; values in (0, 1), or in (-1, 1)
    (values need not be normalised)"""
    w = np.sort(rng.choice(nwords, size=n, replace=False)).astype(np.uint32)
    v = rng.uniform(-1.0 if signed else 0.0, 1.0, n)
    v[v == 0.0] = 0.5
    return w, v.astype(np.float64)


def random_keyframes(seed, n, words=40, nwords=NWORDS):
    rng = np.random.default_rng(seed)
    return [random_bow(rng, words, nwords) for _ in range(n)]


LENGTHS = (0, 1, 63, 64, 65, 128, 129, 257)


def length_pairs(seed=11, nwords=NWORDS):
    """(a, b) for every (na, nb) of LENGTHS x LENGTHS (so both ways round); b
    takes about half of its words from a where it can"""
    rng = np.random.default_rng(seed)
    out = []
    for na in LENGTHS:
        for nb in LENGTHS:
            a = random_bow(rng, na, nwords, signed=True)
            take = rng.choice(a[0], size=min(na, nb) // 2, replace=False) if na else np.zeros(0, np.uint32)
            rest = np.setdiff1d(np.arange(nwords, dtype=np.uint32), a[0])
            extra = rng.choice(rest, size=nb - len(take), replace=False)
            w = np.sort(np.concatenate([take, extra])).astype(np.uint32)
            out.append((a, (w, rng.uniform(-1, 1, nb))))
    return out


def placement_pairs(seed=12, nwords=NWORDS):
    """name -> (a, b): disjoint, identical, one common word first in both, one
    last in both, 64 hits in one 64-word chunk of b"""
    rng = np.random.default_rng(seed)
    v = lambda n: rng.uniform(-1, 1, n)
    ev, od = np.arange(0, 400, 2, dtype=np.uint32), np.arange(1, 400, 2, dtype=np.uint32)
    ident = random_bow(rng, 150, nwords, signed=True)
    out = {
        "disjoint": ((ev, v(200)), (od, v(200))),
        "identical": (ident, (ident[0].copy(), ident[1].copy())),
        # word 3 first in both, nothing else common
        "first": ((np.concatenate([[3], ev[10:80]]).astype(np.uint32), v(71)),
                  (np.concatenate([[3], od[10:110]]).astype(np.uint32), v(101))),
        # word 999 last in both
        "last": ((np.concatenate([ev[:70], [999]]).astype(np.uint32), v(71)),
                 (np.concatenate([od[:130], [999]]).astype(np.uint32), v(131))),
        # b's second chunk (entries 64..127) is words 500..563, all in a
        "chunk64": ((np.arange(480, 600, dtype=np.uint32), v(120)),
                    (np.concatenate([od[:64], np.arange(500, 564), [900, 901, 902]]).astype(np.uint32), v(131))),
    }
    return out


def planted_order_pair(scoring):
    """A pair whose common terms have mixed magnitude (1, 2^-53, -1 patterns),
    so that the left-to-right double sum differs from the reverse and from a
    pairwise tree, and (L2 / dot product) the products are inexact so that a
    fused multiply-add differs too.  Other words in between are not common."""
    t = 2.0 ** -53
    rng = np.random.default_rng(PLANT_SEED[scoring])

    def pair(m):
        """a (vi, wi) whose term is exactly m (L1: -|m|)"""
        if scoring == 0:
            return abs(m) / 2, abs(m)  # |vi - wi| - |vi| - |wi| = -wi for 0 < vi = wi / 2
        if scoring == 2:
            return (2 * m, 2 * m) if m > 0 else (-m, m / 2)  # vi wi / (vi + wi)
        return m, 1.0

    rnd = lambda: (float(rng.uniform(-1, 1)), float(rng.uniform(-1, 1)))  # inexact terms
    vals = [pair(1.0), pair(t), pair(t), rnd(), pair(t), pair(t), pair(-1.0), rnd(), pair(t), rnd(), pair(t),
            pair(-0.5), rnd(), pair(t), rnd(), pair(t), rnd()]
    if scoring == 1:  # a power of two keeps every relation; the sum stays below 1: the sqrt step is taken
        vals = [(p[0] * 0.125, p[1]) for p in vals]
    a = [(10 + 7 * i, p[0]) for i, p in enumerate(vals)]
    b = [(10 + 7 * i, p[1]) for i, p in enumerate(vals)]
    a += [(5, 0.7), (400, 0.2)]   # not common
    b += [(6, 0.3), (401, 0.9)]
    a.sort()
    b.sort()
    return bow([w for w, _ in a], [x for _, x in a]), bow([w for w, _ in b], [x for _, x in b])


# --------------------------------------------------------------------------- other orders
def close(scoring, s):
    """the closing step of the scoring on an accumulated sum, in double"""
    s = np.float64(s)
    if scoring == 0:
        return float(-s / np.float64(2.0))
    if scoring == 1:
        return 1.0 if s >= 1 else float(np.float64(1.0) - np.sqrt(np.float64(1.0) - s))
    if scoring == 2:
        return float(np.float64(2.0) * s)
    return float(s)


def sum_forward(t):
    s = np.float64(0.0)
    for x in t:
        s = s + np.float64(x)
    return float(s)


def sum_reverse(t):
    return sum_forward(list(t)[::-1])


def sum_tree(t):
    """pairwise: neighbours first, as a butterfly over lanes would"""
    t = [np.float64(x) for x in t]
    if not t:
        return 0.0
    while len(t) > 1:
        t = [t[i] + t[i + 1] if i + 1 < len(t) else t[i] for i in range(0, len(t), 2)]
    return float(t[0])


def round_fraction(fr):
    """the double nearest to a Fraction (ties to even): Python's true division
    of big integers is correctly rounded"""
    return fr.numerator / fr.denominator


def sum_fma(a, b):
    """the L2 / dot-product sum with each step fused: s = round(s + vi * wi)"""
    (aw, av), (bw, bv) = bow(*a), bow(*b)
    bm = dict(zip(bw.tolist(), bv.tolist()))
    s = 0.0
    for w, x in zip(aw.tolist(), av.tolist()):
        if w in bm:
            s = round_fraction(Fraction(s) + Fraction(x) * Fraction(bm[w]))
    return s


def exact_terms(scoring, a, b):
    """an independent statement of each scoring's terms: exact rational
    arithmetic rounded once per operation the expression has"""
    (aw, av), (bw, bv) = bow(*a), bow(*b)
    common = np.intersect1d(aw, bw)
    am, bm = dict(zip(aw.tolist(), av.tolist())), dict(zip(bw.tolist(), bv.tolist()))
    R, F = round_fraction, Fraction
    out = []
    for w in common.tolist():
        vi, wi = am[w], bm[w]
        if scoring == 0:
            t = R(F(abs(R(F(vi) - F(wi)))) - F(abs(vi)))
            out.append(R(F(t) - F(abs(wi))))
        elif scoring == 2:
            den = R(F(vi) + F(wi))
            if den != 0.0:
                out.append(R(F(R(F(vi) * F(wi))) / F(den)))
        else:
            out.append(R(F(vi) * F(wi)))
    return out


def exact_score(scoring, a, b):
    s = 0.0
    for t in exact_terms(scoring, a, b):
        s = round_fraction(Fraction(s) + Fraction(t))
    return close(scoring, s)


# --------------------------------------------------------------------------- non-vacuity
def sharing_stats(kfs, query):
    """on the inputs alone: (sharing, not sharing, groups of >= 2 keyframes
    with the same smallest common word)"""
    first = []
    for w, _ in kfs:
        c = np.intersect1d(w, query[0])
        first.append(int(c[0]) if len(c) else -1)
    first = np.array(first)
    sharing = int((first >= 0).sum())
    vals, cnt = np.unique(first[first >= 0], return_counts=True)
    return sharing, len(kfs) - sharing, int((cnt >= 2).sum())


def tie_group(kfs, query, size=3):
    """indices of keyframes (in add order) that share their smallest common
    word with the query, the first group of at least `size`"""
    groups = {}
    for i, (w, _) in enumerate(kfs):
        c = np.intersect1d(w, query[0])
        if len(c):
            groups.setdefault(int(c[0]), []).append(i)
    for f in sorted(groups):
        if len(groups[f]) >= size:
            return groups[f]
    raise AssertionError("no tie group of %d keyframes" % size)
