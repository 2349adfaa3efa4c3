"""Tile edges of the MFMA candidate kernel (k_match_cand_mfma, positions in
the accumulator): its keys are local to a 32-position tile and get the tile's
start added only when they are inserted, so the places where that can go
wrong are the tile boundaries, the two lane halves (positions p and p + 4 of
a tile belong to lanes l and l + 32), the last, partial tile and rows with
more candidates under the distance cap than a list holds (ORBM_T = 8).

Every case plants, around one base descriptor B:
  * a cluster of up to 12 rows B ^ f_i (0..3 flipped bits among bits 0..15);
  * candidates B ^ g at list positions 31|32 and 63|64 (weight 20 each: a
    four-way tie across two tile boundaries), 3|7 (weight 12: a tie across
    the lane halves) and n2 - 2 (weight 30), with g among bits 16..159, so
    that d(row i, candidate) = |f_i| + |g| exactly -- ties by construction;
  * per cluster row a near copy (1..2 more bits among 160..191) at a position
    of its own, so that rows compete for each other's best candidates and a
    cluster row sees more than 8 candidates under the cap;
  * one unrelated row whose only candidate sits in the list's last tile.
Everything else is random (distance ~128, far above the cap).  The drop-in
call and the batched plan form, with 6 live dwords (bytes 24..31 zero) and
with 8, must return the oracle's matches and count.
"""
import numpy as np
import pytest

N1S = (1, 33, 129)
N2S = (1, 31, 32, 33, 63, 64, 65, 97)
# + one list long enough for the 4-way column split of a small launch
SHAPES = [(n1, n2) for n1 in N1S for n2 in N2S] + [(33, 289)]


def _flip(d, bits):
    d = d.copy()
    for b in bits:
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def _case(n1, n2, six, seed):
    """(desc1, angle1, desc2 by list position, angle2, the lone row's position or None)"""
    rng = np.random.default_rng(seed)
    d1 = rng.integers(0, 256, (n1, 32), dtype=np.uint8)
    d2 = rng.integers(0, 256, (n2, 32), dtype=np.uint8)
    base = rng.integers(0, 256, 32, dtype=np.uint8)
    if six:
        d1[:, 24:] = 0
        d2[:, 24:] = 0
        base[24:] = 0
    ncl = min(n1, 12)
    f = [list(rng.choice(16, i % 4, replace=False)) for i in range(ncl)]
    for i in range(ncl):
        d1[i] = _flip(base, f[i])
    planted = {}
    g = lambda w: list(16 + rng.choice(144, w, replace=False))
    for pos, w in ((31, 20), (32, 20), (63, 20), (64, 20), (3, 12), (7, 12), (n2 - 2, 30)):
        if 0 <= pos < n2 and pos not in planted:
            planted[pos] = _flip(base, g(w))
    # a row whose only candidate sits in the last (partial) tile: its last
    # position that holds no tie candidate (n2 = 33, 65: that tile is one tie position alone)
    lone = next((p for p in range(n2 - 1, 32 * ((n2 - 1) // 32) - 1, -1) if p not in planted), None)
    if n1 > ncl and lone is not None:
        planted[lone] = _flip(d1[n1 - 1], list(rng.choice(160, 3, replace=False)))
    else:
        lone = None
    free = [p for p in rng.permutation(n2) if p not in planted]
    for i in range(min(ncl, len(free))):
        planted[int(free[i])] = _flip(d1[i], list(160 + rng.choice(32, 1 + i % 2, replace=False)))
    for pos, d in planted.items():
        d2[pos] = d
    # angles: a few rotation bins, so the orientation histogram keeps and drops some
    a1 = rng.choice([10.0, 11.0, 200.0], n1).astype(np.float32)
    a2 = rng.choice([10.0, 12.0, 100.0], n2).astype(np.float32)
    return d1, a1, d2, a2, lone


def _bow(desc, ang, feat):
    return dict(desc=desc, angle=ang, valid=None, node_id=np.array([5], np.uint32),
                off=np.array([0, len(feat)], np.uint32), feat=feat.astype(np.uint32))


@pytest.fixture(scope="module")
def cases(oracle):
    """case data and the oracle's answer in list order (feat = identity), per (six, shape)"""
    out = {}
    for six in (True, False):
        for s, (n1, n2) in enumerate(SHAPES):
            d1, a1, d2, a2, lone = _case(n1, n2, six, 1000 * six + s)
            rm, rnm = oracle.search_by_bow(_bow(d1, a1, np.arange(n1)), _bow(d2, a2, np.arange(n2)), 0.75, True)
            out[six, n1, n2] = (d1, a1, d2, a2, lone, rm.copy(), int(rnm))
    return out


def test_cases_are_not_vacuous(cases):
    """CPU only: the planted structure gives matches, ties and full lists"""
    for (six, n1, n2), (d1, a1, d2, a2, lone, rm, rnm) in cases.items():
        if lone is not None:
            # the lone row takes its candidate, in the last tile (-2: taken,
            # then dropped by the rotation histogram)
            assert lone >= 32 * ((n2 - 1) // 32) and rm[n1 - 1] in (lone, -2), (six, n1, n2)
        else:
            assert n1 <= 12 or n2 in (33, 65)
        if n1 >= 33 and n2 >= 33:
            assert rnm >= 3, (six, n1, n2, rnm)
            dist = np.unpackbits(d1[:12, None, :] ^ d2[None, :, :], axis=2).sum(2)
            assert (dist < 66).sum(1).max() > 8, (six, n1, n2)  # more than ORBM_T under the cap (66 at 0.75)
            assert dist[0, 31] == dist[0, 32] == 20 and dist[0, 3] == dist[0, 7] == 12


@pytest.mark.gpu
@pytest.mark.parametrize("six", [True, False])
def test_search_by_bow_tile_edges(gpu, oracle, cases, six):
    for n1, n2 in SHAPES:
        d1, a1, d2, a2, _, rm, rnm = cases[six, n1, n2]
        # list position j holds feature perm[j]: the kernel's positions are list positions
        perm = np.random.default_rng(n1 * 1000 + n2).permutation(n2)
        d2f = np.empty_like(d2)
        d2f[perm] = d2
        a2f = np.empty_like(a2)
        a2f[perm] = a2
        m, nm = gpu.search_by_bow(_bow(d1, a1, np.arange(n1)), _bow(d2f, a2f, perm), 0.75, True)
        ref = np.where(rm >= 0, perm[np.maximum(rm, 0)], rm)
        assert nm == rnm, (six, n1, n2, nm, rnm)
        assert np.array_equal(m, ref), (six, n1, n2)
        # and against the oracle on the permuted problem itself
        om, onm = oracle.search_by_bow(_bow(d1, a1, np.arange(n1)), _bow(d2f, a2f, perm), 0.75, True)
        assert onm == nm and np.array_equal(om, m), (six, n1, n2)


@pytest.mark.gpu
@pytest.mark.parametrize("six", [True, False])
def test_match_plan_tile_edges(gpu, oracle, cases, six):
    """all shapes as the pairs of one batched call (single node, every feature:
    list position = feature index)"""
    import torch
    P, kcap = len(SHAPES), max(max(s) for s in SHAPES)
    ka = np.zeros((P, kcap), gpu.KEYPOINT_DTYPE)
    kb = np.zeros((P, kcap), gpu.KEYPOINT_DTYPE)
    da = np.zeros((P, kcap, 32), np.uint8)
    db = np.zeros((P, kcap, 32), np.uint8)
    ca = np.zeros(P, np.int32)
    cb = np.zeros(P, np.int32)
    for p, (n1, n2) in enumerate(SHAPES):
        d1, a1, d2, a2, _, rm, rnm = cases[six, n1, n2]
        ka["angle"][p, :n1], kb["angle"][p, :n2] = a1, a2
        ka["response"][p, :n1], kb["response"][p, :n2] = 1.0, 1.0
        da[p, :n1], db[p, :n2] = d1, d2
        ca[p], cb[p] = n1, n2
    dev = lambda a: torch.from_numpy(a.view(np.uint8).reshape(a.shape + (-1,)) if a.dtype == gpu.KEYPOINT_DTYPE
                                     else a).cuda()
    mp = gpu.MatchPlan(P, kcap, topn=kcap, zero_tail=six)
    mp.match(P, dev(ka), dev(da), dev(ca), dev(kb), dev(db), dev(cb), 0.75, True)
    torch.cuda.synchronize()
    m12 = mp.match12.cpu().numpy()
    nm = mp.nmatches.cpu().numpy()
    for p, (n1, n2) in enumerate(SHAPES):
        rm, rnm = cases[six, n1, n2][5:]
        assert nm[p] == rnm, (six, n1, n2, nm[p], rnm)
        assert np.array_equal(m12[p, :n1], rm), (six, n1, n2)
