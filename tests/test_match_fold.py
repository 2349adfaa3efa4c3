"""Folded lists of the batched frame-pair matcher (MatchPlan, fold=True):
selected keypoints of a frame with byte-identical descriptors are computed
once, in pairs of a representative and one follower (k_match_select builds the
fold table, k_match_expand2 / k_match_cand_mfma run over representatives and
expand the followers when a row's candidate list is written out).

Every case is a frame pair of one batched call, topn = kcap, with 6 live
descriptor dwords (zero_tail) and with 8.  Lists are built from a list of
distinct descriptors with the planted structure of test_match_tile_edges.py
(a cluster of rows around one base descriptor, candidates at exact distances
with ties across tile boundaries and lane halves, near copies, random filler
at distance ~128 / ~96) and a placement: which list positions hold copies of
which distinct descriptor.  Every case must give the oracle's match12 and
nmatches, with fold and without, and the follower counts of fold_stats must
equal a CPU model of the fold (the hash of csrc/match_fold_hash.h, built for
the host from tests/cpp/match_fold_hash.c).
"""
import ctypes

import numpy as np
import pytest

import native

KCAP = 130
NNR = 0.75
CAP = 66  # orbm_dcap(0.75): candidates at or above it cannot change a decision


# --------------------------------------------------------------------------
# the fold on the CPU
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def foldhash():
    L = native.ref_lib("match_fold_hash.c")
    L.fold_slots.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.fold_slots.restype = None
    return L


def _slots(L, desc, rnd, hbits):
    w = np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)
    out = np.zeros(len(w), np.uint32)
    if len(w):
        L.fold_slots(w.ctypes.data, len(w), rnd, hbits, out.ctypes.data)
    return out


def fold_model(L, desc, hbits):
    """k_match_select's fold of one list: {representative position: follower position}"""
    fol = {}
    pending = list(range(len(desc)))
    for rnd in range(L.fold_rounds()):
        if not pending:
            break
        s = [int(x) for x in _slots(L, desc[pending], rnd, hbits)]
        claim = {}
        for j, sj in zip(pending, s):  # ascending positions: the first is the smallest
            claim.setdefault(sj, j)
        losers = []
        for j, sj in zip(pending, s):
            c = claim[sj]
            if c == j:
                continue
            if np.array_equal(desc[j], desc[c]):
                fol.setdefault(c, j)
            else:
                losers.append(j)
        pending = losers
    return fol


def ideal_followers(desc):
    """groups of two or more identical descriptors: one follower each"""
    if len(desc) == 0:
        return 0
    _, cnt = np.unique(np.ascontiguousarray(desc).reshape(len(desc), 32), axis=0, return_counts=True)
    return int((cnt >= 2).sum())


# --------------------------------------------------------------------------
# case construction
# --------------------------------------------------------------------------
def _flip(d, bits):
    d = d.copy()
    for b in bits:
        d[int(b) // 8] ^= np.uint8(1 << (int(b) % 8))
    return d


def _rand(rng, n, six):
    d = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    if six:
        d[:, 24:] = 0
    return d


def _distinct(n1, n2, six, seed):
    """distinct descriptors of list1 and list2 with the planted structure, and the base"""
    rng = np.random.default_rng(seed)
    d1, d2 = _rand(rng, max(n1, 1), six), _rand(rng, max(n2, 1), six)
    base = _rand(rng, 1, six)[0]
    ncl = min(len(d1), 12)
    seen = {()}
    d1[0] = base
    for i in range(1, ncl):  # 1..3 flipped bits among 0..15, all different
        b = ()
        while b in seen:
            b = tuple(sorted(int(x) for x in rng.choice(16, 1 + (i - 1) % 3, replace=False)))
        seen.add(b)
        d1[i] = _flip(base, b)
    N2 = len(d2)
    planted = {}
    g = lambda w: list(16 + rng.choice(144, w, replace=False))
    for pos, w in ((31, 20), (32, 20), (63, 20), (64, 20), (3, 12), (7, 12), (N2 - 2, 30)):
        if 0 <= pos < N2 and pos not in planted:
            planted[pos] = _flip(base, g(w))
    free = [int(p) for p in rng.permutation(N2) if p not in planted]
    for i in range(min(ncl, len(free))):
        planted[free[i]] = _flip(d1[i], list(160 + rng.choice(32, 1 + i % 2, replace=False)))
    for pos, d in planted.items():
        d2[pos] = d
    return d1[:n1], d2[:n2], base


def _singles(m):
    return [(i,) for i in range(m)]


def _pairs_from(fixed, n):
    """the fixed pairs, the other positions paired in order"""
    used = {p for g in fixed for p in g}
    rest = [p for p in range(n) if p not in used]
    groups = list(fixed) + [tuple(rest[i:i + 2]) for i in range(0, len(rest), 2)]
    return sorted(groups)


def _pairs_adjacent(m):
    return [(2 * u, 2 * u + 1) for u in range(m)]


def _pairs_tile(m):  # followers across the 32-position tile boundaries
    return _pairs_from([(31, 32)] + ([(63, 64)] if 2 * m > 64 else []), 2 * m)


def _pairs_halves(m):  # positions p and p + 4: the two lane halves of a tile
    return _pairs_from([(b + i, b + i + 4) for b in range(0, 2 * m - 7, 8) for i in range(4)], 2 * m)


def _groups_random(sizes, rng):
    perm = [int(p) for p in rng.permutation(sum(sizes))]
    groups, at = [], 0
    for s in sizes:
        groups.append(tuple(sorted(perm[at:at + s])))
        at += s
    return sorted(groups)


def _expand(du, groups):
    """distinct descriptor i (in the order of the groups' first positions) at the positions of group i"""
    assert len(groups) == len(du), (len(groups), len(du))
    n = sum(len(g) for g in groups)
    d = np.zeros((n, 32), np.uint8)
    for i, grp in enumerate(groups):
        for p in grp:
            d[p] = du[i]
    return d


def _case(name, d1, d2, rng, groups1=None, groups2=None, angles=True, **kw):
    n1, n2 = len(d1), len(d2)
    a1 = rng.choice([10.0, 11.0, 200.0], n1).astype(np.float32) if angles else np.full(n1, 10.0, np.float32)
    a2 = rng.choice([10.0, 12.0, 100.0], n2).astype(np.float32) if angles else np.full(n2, 10.0, np.float32)
    c = dict(name=name, d1=d1, a1=a1, d2=d2, a2=a2, groups1=groups1, groups2=groups2)
    c.update(kw)
    return c


def _placed(name, n1u, g1, n2u, g2, six, seed, **kw):
    d1u, d2u, _ = _distinct(n1u, n2u, six, seed)
    rng = np.random.default_rng(seed + 7)
    return _case(name, _expand(d1u, g1), _expand(d2u, g2), rng, g1, g2, **kw)


def _cut_case(kind, six, seed):
    """Row 8 of list1 is B; list2 holds B ^ g_i with disjoint g_i (distances add up).
    kind 7: six singles (2, 3, 4, 5, 6, 8 bits) and one twin pair (12 bits): 7
    representatives under the cap, 8 keys.  Rows 0..4 take the first five
    singles; row 8 then takes the sixth (8 < 0.75 * 12).
    kind 8: five singles (2..6 bits), the twin pair R2 | F2 (10 bits) at
    positions 3 | 40, a single R' (10 bits) at position 5, a twin pair at 20
    bits: 8 representatives under the cap; the whole list's 8 smallest keys end
    (10, 3) (10, 5) (10, 40), the follower behind R'.  Rows 0..5 take the
    singles and R'; row 8 then sees R2 and F2 at the same distance and takes
    nothing, while representatives alone would give it R2 (10 < 0.75 * 20)."""
    rng = np.random.default_rng(seed)
    n1, n2 = 40, 70
    d1, d2 = _rand(rng, n1, six), _rand(rng, n2, six)
    B = _rand(rng, 1, six)[0]
    bits = [int(b) for b in rng.permutation(192)]
    take = lambda w: _flip(B, [bits.pop() for _ in range(w)])
    if kind == 7:
        singles = [take(w) for w in (2, 3, 4, 5, 6, 8)]
        r2 = take(12)
        for i, s in enumerate(singles):
            d2[10 + i] = s
        d2[3], d2[40] = r2, r2
        for i in range(5):
            d1[i] = singles[i]
        followers2 = [40]
    else:
        singles = [take(w) for w in (2, 3, 4, 5, 6)]
        r2, rp, r7 = take(10), take(10), take(20)
        for i, s in enumerate(singles):
            d2[10 + i] = s
        d2[3], d2[5], d2[40], d2[50], d2[60] = r2, rp, r2, r7, r7
        for i in range(5):
            d1[i] = singles[i]
        d1[5] = rp
        followers2 = [40, 60]
    d1[8] = B
    return _case("cut%d" % kind, d1, d2, rng, angles=False, B=B, followers2=followers2)


def _colliding(L, base, hbits, rng):
    """two distinct descriptors, 20 bits from base each, in one slot in both rounds"""
    cand = np.stack([_flip(base, 16 + rng.choice(144, 20, replace=False)) for _ in range(4096)])
    key = _slots(L, cand, 0, hbits).astype(np.int64) * (1 << hbits) + _slots(L, cand, 1, hbits)
    first = {}
    for i, k in enumerate(key):
        j = first.setdefault(int(k), i)
        if j != i and not np.array_equal(cand[i], cand[j]):
            return cand[j], cand[i]
    raise AssertionError("no colliding pair among 4096 descriptors")


def _build_cases(L, six):
    hbits = L.fold_hbits(KCAP)
    S = 5000 * six
    rngs = np.random.default_rng(S + 99)
    cases = []
    # 1. no duplicates at all
    cases.append(_placed("plain33x65", 33, _singles(33), 65, _singles(65), six, S + 1))
    cases.append(_placed("plain129x97", 129, _singles(129), 97, _singles(97), six, S + 2))
    # 2. every list2 entry duplicated once; folded counts 31, 32, 33
    for m in (31, 32, 33):
        for pname, place in (("adj", _pairs_adjacent), ("tile", _pairs_tile), ("halves", _pairs_halves)):
            cases.append(_placed("dup2_%s_%d" % (pname, m), 33, _singles(33), m, place(m), six, S + 10 * m + len(pname)))
    # 3. duplicates in one list only, and a third of the entries of both lists
    cases.append(_placed("dup1only", 45, _groups_random([2] * 20 + [1] * 25, rngs), 65, _singles(65), six, S + 3))
    cases.append(_placed("dup2only", 65, _singles(65), 45, _groups_random([2] * 20 + [1] * 25, rngs), six, S + 4))
    cases.append(_placed("thirds", 43, _groups_random([2] * 22 + [1] * 21, rngs), 43,
                         _groups_random([1] * 21 + [2] * 22, rngs), six, S + 5))
    # 4. groups of 3 and 5 in both lists: one follower each
    sizes = [3, 5, 1, 2, 3, 1, 5, 2] + [1] * 30
    cases.append(_placed("groups35", len(sizes), _groups_random(sizes, rngs), len(sizes),
                         _groups_random(sizes[::-1], rngs), six, S + 6, exact_stats=True))
    # 5. a list of one descriptor only (two copies: folded count 1; forty: one
    # follower, 39 representatives), lists of 1 and 0 entries
    cases.append(_placed("two2", 33, _singles(33), 1, [(0, 1)], six, S + 20, exact_stats=True))
    cases.append(_placed("two1", 1, [(0, 1)], 40, _singles(40), six, S + 21, exact_stats=True))
    cases.append(_placed("forty2", 33, _singles(33), 1, [tuple(range(40))], six, S + 22, exact_stats=True))
    cases.append(_placed("forty1", 1, [tuple(range(40))], 33, _singles(33), six, S + 23, exact_stats=True))
    cases.append(_placed("one2", 33, _singles(33), 1, _singles(1), six, S + 24))
    cases.append(_placed("one1", 1, _singles(1), 33, _singles(33), six, S + 25))
    cases.append(_placed("none2", 33, _singles(33), 0, [], six, S + 26))
    cases.append(_placed("none1", 0, [], 33, _singles(33), six, S + 27))
    # 6. list1: representative and follower on the two sides of a multiple of
    # 32, and in the first and the last row tile
    cases.append(_placed("rows_tile", 65, _pairs_from([(31, 32), (63, 64), (5, 129)], 130), 65, _singles(65),
                         six, S + 7))
    # 7, 8. the candidate list's cut
    cases.append(_cut_case(7, six, S + 8))
    cases.append(_cut_case(8, six, S + 9))
    # 10. two distinct descriptors of one hash slot, in both lists
    d1u, d2u, base = _distinct(33, 65, six, S + 30)
    ca, cb = _colliding(L, base, hbits, np.random.default_rng(S + 31))
    d1u, d2u = d1u.copy(), d2u.copy()
    d2u[20], d2u[45], d1u[20], d1u[25] = ca, cb, ca, cb
    cases.append(_case("collide", d1u, d2u, np.random.default_rng(S + 32), collide=(ca, cb)))
    return cases


def _bow(desc, ang, feat):
    return dict(desc=desc, angle=ang, valid=None, node_id=np.array([5], np.uint32),
                off=np.array([0, len(feat)], np.uint32), feat=np.asarray(feat).astype(np.uint32))


def _oracle(oracle, d1, a1, f1, d2, a2, f2):
    pad = lambda d: d if len(d) else np.zeros((1, 32), np.uint8)  # no feature refers to the pad row
    pa = lambda a: a if len(a) else np.zeros(1, np.float32)
    rm, rnm = oracle.search_by_bow(_bow(pad(d1), pa(a1), f1), _bow(pad(d2), pa(a2), f2), NNR, True)
    return rm[:len(d1)].copy(), int(rnm)


@pytest.fixture(scope="module")
def cases(oracle, foldhash):
    """per six: the cases, each with the oracle's answer and the model's follower counts"""
    out = {}
    hbits = foldhash.fold_hbits(KCAP)
    for six in (True, False):
        cs = _build_cases(foldhash, six)
        for c in cs:
            n1, n2 = len(c["d1"]), len(c["d2"])
            c["rm"], c["rnm"] = _oracle(oracle, c["d1"], c["a1"], np.arange(n1), c["d2"], c["a2"], np.arange(n2))
            c["fol1"] = fold_model(foldhash, c["d1"], hbits)
            c["fol2"] = fold_model(foldhash, c["d2"], hbits)
        out[six] = cs
    return out


# --------------------------------------------------------------------------
# CPU-only checks
# --------------------------------------------------------------------------
def test_colliding_pair_collides(cases, foldhash):
    hbits = foldhash.fold_hbits(KCAP)
    for six in (True, False):
        c = next(c for c in cases[six] if c["name"] == "collide")
        a, b = c["collide"]
        assert not np.array_equal(a, b)
        for rnd in range(foldhash.fold_rounds()):
            s = _slots(foldhash, np.stack([a, b]), rnd, hbits)
            assert s[0] == s[1] < (1 << hbits), (six, rnd, s)
        assert not c["fol1"] and not c["fol2"]  # they do not fold
        assert np.array_equal(c["d2"][20], a) and np.array_equal(c["d2"][45], b)


def test_expected_followers(cases):
    """the model's follower counts against the cases' construction"""
    for six in (True, False):
        for c in cases[six]:
            for side in "12":
                d, fol, groups = c["d" + side], c["fol" + side], c["groups" + side]
                ideal = ideal_followers(d)
                assert len(fol) <= ideal, (six, c["name"], side)
                for r, f in fol.items():  # a follower is the next copy after its representative
                    same = [p for p in range(len(d)) if np.array_equal(d[p], d[r])]
                    assert same[0] == r and same[1] == f, (six, c["name"], side, r, f)
                if groups is not None:  # the placement's groups are the data's
                    assert ideal == sum(len(g) >= 2 for g in groups), (six, c["name"], side)
                if c.get("exact_stats") or c["name"].startswith("plain"):
                    assert len(fol) == ideal, (six, c["name"], side)
            if c["name"].startswith("plain"):
                assert not c["fol1"] and not c["fol2"]
            if c["name"].startswith("dup2_"):
                m = int(c["name"].rsplit("_", 1)[1])
                assert len(c["d2"]) == 2 * m and ideal_followers(c["d2"]) == m
            if c["name"] == "groups35":
                assert ideal_followers(c["d1"]) == 6 and len(c["fol1"]) == 6 and len(c["fol2"]) == 6
            if c["name"] in ("forty1", "forty2"):
                assert len(c["fol1"]) + len(c["fol2"]) == 1
        # a pair is missed when an earlier, different descriptor holds its slot: with
        # at least four slots per entry that is at most a quarter of the pairs
        tot = sum(len(c["fol1"]) + len(c["fol2"]) for c in cases[six])
        ideal = sum(ideal_followers(c["d1"]) + ideal_followers(c["d2"]) for c in cases[six])
        assert 4 * tot >= 3 * ideal and tot > 340, (six, tot, ideal)


def test_cases_are_not_vacuous(cases, oracle):
    """the planted structure gives matches, ties, full lists and a cut that discriminates"""
    for six in (True, False):
        by = {c["name"]: c for c in cases[six]}
        assert sum(c["rnm"] for c in cases[six]) > 60
        for name in ("plain33x65", "dup1only", "thirds", "groups35", "rows_tile", "collide"):
            assert by[name]["rnm"] >= 3, (six, name, by[name]["rnm"])
        dist = lambda c: np.unpackbits(c["d1"][:, None, :] ^ c["d2"][None, :, :], axis=2).sum(2)
        for name in ("dup2_adj_33", "dup2_tile_33", "dup2_halves_33", "rows_tile"):
            # more than ORBM_T keys under the cap in a row, twins among them
            dd = dist(by[name])
            assert (dd < CAP).sum(1).max() > 8, (six, name)
        # a tie of two representatives across the folded tile boundary 31 | 32
        c = by["dup2_adj_33"]
        dd = dist(c)
        assert dd[0, 62] == dd[0, 63] == dd[0, 64] == dd[0, 65] == 20
        # 7: seven representatives, eight keys under the cap; the row takes the sixth single
        c = by["cut7"]
        under = np.flatnonzero(dist(c)[8] < CAP)
        assert len(under) == 8 and len({c["d2"][p].tobytes() for p in under}) == 7
        assert c["rm"][8] == 15 and c["fol2"] == {3: 40}
        # 8: eight representatives, eleven keys; the 8 smallest end R2, R', F2
        c = by["cut8"]
        dd = dist(c)[8]
        under = np.flatnonzero(dd < CAP)
        assert len(under) == 10 and len({c["d2"][p].tobytes() for p in under}) == 8
        keys = sorted((int(dd[p]), int(p)) for p in under)
        assert keys[5:8] == [(10, 3), (10, 5), (10, 40)] and keys[8][0] == 20
        assert c["fol2"] == {3: 40, 50: 60}
        # representatives only, followers dropped: row 8 would take R2
        reps = np.array([p for p in range(len(c["d2"])) if p not in c["followers2"]])
        nm, _ = _oracle(oracle, c["d1"], c["a1"], np.arange(len(c["d1"])), c["d2"], c["a2"], reps)
        assert c["rm"][8] == -1 and nm[8] == 3
        assert all(c["rm"][i] == 10 + i for i in range(5)) and c["rm"][5] == 5


# --------------------------------------------------------------------------
# GPU
# --------------------------------------------------------------------------
def _run(gpu, pairs, kcap, topn, six, fold, shared=None):
    """pairs: (d1, a1, r1, d2, a2, r2) per pair -> match12, nmatches, fold_stats"""
    import torch
    P = len(pairs)
    ka = np.zeros((P, kcap), gpu.KEYPOINT_DTYPE)
    kb = np.zeros((P, kcap), gpu.KEYPOINT_DTYPE)
    da = np.zeros((P, kcap, 32), np.uint8)
    db = np.zeros((P, kcap, 32), np.uint8)
    ca = np.zeros(P, np.int32)
    cb = np.zeros(P, np.int32)
    for p, (d1, a1, r1, d2, a2, r2) in enumerate(pairs):
        n1, n2 = len(d1), len(d2)
        ka["angle"][p, :n1], kb["angle"][p, :n2] = a1, a2
        ka["response"][p, :n1], kb["response"][p, :n2] = r1, r2
        da[p, :n1], db[p, :n2] = d1, d2
        ca[p], cb[p] = n1, n2
    dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(a.shape + (-1,)) if a.dtype == gpu.KEYPOINT_DTYPE
                                     else a).cuda()
    mp = gpu.MatchPlan(P, kcap, topn=topn, zero_tail=six, fold=fold)
    mp.match(P, dev(ka), dev(da), dev(ca), dev(kb), dev(db), dev(cb), NNR, True)
    torch.cuda.synchronize()
    return mp.match12.cpu().numpy(), mp.nmatches.cpu().numpy(), mp.fold_stats()


@pytest.mark.gpu
@pytest.mark.parametrize("six", [True, False])
def test_match_plan_fold(gpu, cases, six):
    """all cases as the pairs of one call (list position = feature index)"""
    cs = cases[six]
    pairs = [(c["d1"], c["a1"], 1.0, c["d2"], c["a2"], 1.0) for c in cs]
    m12, nm, st = _run(gpu, pairs, KCAP, KCAP, six, True)
    m12n, nmn, stn = _run(gpu, pairs, KCAP, KCAP, six, False)
    print("fold_stats", st, "unfolded", stn)
    for p, c in enumerate(cs):
        n1 = len(c["d1"])
        assert nm[p] == c["rnm"], (six, c["name"], nm[p], c["rnm"])
        assert np.array_equal(m12[p, :n1], c["rm"]), (six, c["name"])
    assert np.array_equal(nm, nmn) and np.array_equal(m12, m12n)
    e1, e2 = sum(len(c["d1"]) for c in cs), sum(len(c["d2"]) for c in cs)
    assert st == (e1, sum(len(c["fol1"]) for c in cs), e2, sum(len(c["fol2"]) for c in cs))
    assert stn == (e1, 0, e2, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("six", [True, False])
def test_match_plan_fold_stats_per_case(gpu, cases, six):
    """the cases whose follower counts the construction fixes, one call each"""
    for name in ("plain33x65", "groups35", "two2", "forty1"):
        c = next(c for c in cases[six] if c["name"] == name)
        m12, nm, st = _run(gpu, [(c["d1"], c["a1"], 1.0, c["d2"], c["a2"], 1.0)], KCAP, KCAP, six, True)
        assert st == (len(c["d1"]), ideal_followers(c["d1"]), len(c["d2"]), ideal_followers(c["d2"])), (six, name, st)
        assert nm[0] == c["rnm"] and np.array_equal(m12[0, :len(c["d1"])], c["rm"]), (six, name)


def _select(resp, topn):
    """the plan's selection: top-n by (response desc, index asc), in index order"""
    order = sorted(range(len(resp)), key=lambda i: (-resp[i], i))[:topn]
    return np.array(sorted(order), np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("six", [True, False])
def test_match_plan_fold_selection_cut(gpu, oracle, foldhash, six):
    """count > topn with the response cut between a representative and its twin
    (by response in frame A, by index among equal responses in frame B), and
    count < topn"""
    kcap, topn = 100, 40
    hbits = foldhash.fold_hbits(topn)
    d1, d2, _ = _distinct(90, 90, six, 7000 + six)
    d1, d2 = d1.copy(), d2.copy()
    rng = np.random.default_rng(7100 + six)
    a1 = rng.choice([10.0, 11.0, 200.0], 90).astype(np.float32)
    a2 = rng.choice([10.0, 12.0, 100.0], 90).astype(np.float32)
    r1 = np.ones(90, np.float32)
    r1[:39] = 10.0
    r1[64] = 10.0
    d1[50], r1[50] = d1[10], 5.0  # the twin of 10 falls under the cut
    d1[20] = d1[12]               # a twin pair above it
    r2 = np.ones(90, np.float32)
    r2[:30] = 10.0
    r2[30:50] = 5.0               # the cut takes 30..39 of these
    d2[80], r2[80] = d2[33], 5.0  # the twin of 33: same response, beyond the cut by index
    d2[20] = d2[3]
    s1, s2 = _select(r1, topn), _select(r2, topn)
    assert 10 in s1 and 50 not in s1 and 33 in s2 and 80 not in s2 and len(s1) == len(s2) == topn
    rm, rnm = _oracle(oracle, d1, a1, s1, d2, a2, s2)
    # count < topn: the first 30 of each
    rm3, rnm3 = _oracle(oracle, d1[:30], a1[:30], np.arange(30), d2[:30], a2[:30], np.arange(30))
    assert rnm + rnm3 >= 3
    pairs = [(d1, a1, r1, d2, a2, r2), (d1[:30], a1[:30], r1[:30], d2[:30], a2[:30], r2[:30])]
    exp = (topn + 30, len(fold_model(foldhash, d1[s1], hbits)) + len(fold_model(foldhash, d1[:30], hbits)),
           topn + 30, len(fold_model(foldhash, d2[s2], hbits)) + len(fold_model(foldhash, d2[:30], hbits)))
    assert exp[1] == 2 and exp[3] == 2  # (12, 20) twice and (3, 20) twice; never (10, 50) or (33, 80)
    for fold in (True, False):
        m12, nm, st = _run(gpu, pairs, kcap, topn, six, fold)
        assert nm[0] == rnm and np.array_equal(m12[0, :90], rm), (six, fold)
        assert nm[1] == rnm3 and np.array_equal(m12[1, :30], rm3), (six, fold)
        assert st == (exp if fold else (exp[0], 0, exp[2], 0)), (six, fold, st)


SHIFT_KCAP = 70


def _shifted_frames(oracle, six):
    """P + 1 frames, a third of each one's entries twins; pair p = frame p + 1 against frame p"""
    d1u, d2u, _ = _distinct(33, 33, six, 8000 + six)
    rng = np.random.default_rng(8100 + six)
    third = lambda m: _groups_random([2] * (m // 3) + [1] * (m - m // 3), rng)
    lists = [_expand(d2u, third(33)), _expand(d1u, third(33)), _expand(d2u, third(33)),
             _expand(d1u[:31], third(31)), _expand(d2u[:32], _singles(32))]
    angles = [rng.choice([10.0, 11.0, 200.0], len(x)).astype(np.float32) for x in lists]
    ref = [_oracle(oracle, lists[p + 1], angles[p + 1], np.arange(len(lists[p + 1])),
                   lists[p], angles[p], np.arange(len(lists[p]))) for p in range(len(lists) - 1)]
    return lists, angles, ref


def test_shifted_frames_are_not_vacuous(oracle):
    for six in (True, False):
        lists, _, ref = _shifted_frames(oracle, six)
        assert max(len(x) for x in lists) <= SHIFT_KCAP
        assert sum(r[1] for r in ref) >= 6 and all(r[1] >= 1 for r in ref), [r[1] for r in ref]
        assert sum(ideal_followers(x) for x in lists) == 11 + 11 + 11 + 10


@pytest.mark.gpu
@pytest.mark.parametrize("six", [True, False])
def test_match_plan_fold_shifted_sides(gpu, oracle, foldhash, six):
    """side B as side A one frame back: two views of one buffer of P + 1 frames,
    and the same data in two separate buffers"""
    import torch
    kcap = SHIFT_KCAP
    lists, angles, ref = _shifted_frames(oracle, six)
    P = len(lists) - 1
    k = np.zeros((P + 1, kcap), gpu.KEYPOINT_DTYPE)
    d = np.zeros((P + 1, kcap, 32), np.uint8)
    cnt = np.array([len(x) for x in lists], np.int32)
    for f, x in enumerate(lists):
        k["angle"][f, :len(x)] = angles[f]
        k["response"][f, :len(x)] = 1.0
        d[f, :len(x)] = x
    kd = torch.from_numpy(k.view(np.uint8).reshape(k.shape + (-1,))).cuda()
    dd, cd = torch.from_numpy(d).cuda(), torch.from_numpy(cnt).cuda()
    res = []
    for fold in (True, False):
        for views in (True, False):
            mp = gpu.MatchPlan(P, kcap, topn=kcap, zero_tail=six, fold=fold)
            if views:
                args = (kd[1:], dd[1:], cd[1:], kd, dd, cd)
            else:
                args = (kd[1:].clone(), dd[1:].clone(), cd[1:].clone(), kd[:P].clone(), dd[:P].clone(), cd[:P].clone())
            mp.match(P, *args, NNR, True)
            torch.cuda.synchronize()
            m12, nm, st = mp.match12.cpu().numpy(), mp.nmatches.cpu().numpy(), mp.fold_stats()
            for p in range(P):
                assert nm[p] == ref[p][1], (six, fold, views, p, nm[p], ref[p][1])
                assert np.array_equal(m12[p, :cnt[p + 1]], ref[p][0]), (six, fold, views, p)
            res.append(st)
    assert res[0] == res[1] and res[2] == res[3], res
    nf = [len(fold_model(foldhash, x, foldhash.fold_hbits(kcap))) for x in lists]
    assert res[0] == (int(cnt[1:].sum()), sum(nf[1:]), int(cnt[:P].sum()), sum(nf[:P])), (res[0], nf)
    assert res[2] == (res[0][0], 0, res[0][2], 0)
    assert sum(nf) >= 40
