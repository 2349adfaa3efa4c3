"""DBoW2 vocabulary transform: planted edge cases of k_bow_descend,
k_bow_assemble, orbv_transform / orbv_transform_batch and the text loader
(TemplatedVocabulary.h:1126-1259, 1338-1424).

Every case has two parts.  CPU: the oracle equals the plain restatement of
tests/vocab_util.py on all five arrays, and the case is what it claims (the
non-vacuity figures come from the restatement or the oracle, never from the
library).  GPU: the library equals the oracle bit for bit -- word, node and
feature ids as integers, BowVector values as uint64 -- through orbv_transform
and, where a case says so, through orbv_transform_batch on the same
descriptors uploaded as one frame.

What the cases reach that random vocabularies of k <= 10 do not: the second
trip of k_bow_descend's 16-lane child loop (k 17, 20; 40 root children), the
first-minimum tie between lanes and between trips, scorings 2-4 and all 24
scoring x weighting pairs, k_bow_assemble at n = 1, around 1024 (one to two
entries per thread), 8192, with norm == 0, with one word, and in a batch with
counts 0, 1 and kcap side by side, the unset-NodeId rule for stopped and kept
features and the latched error's reset.
"""
import functools

import numpy as np
import pytest

import vocab_util as vu
from orbx import synth


def _rnd(seed, n):
    return np.random.default_rng(seed).integers(0, 256, (n, 32), dtype=np.uint8)


def _oracle(oracle, voc, scoring, weighting, d, levelsup):
    """the oracle's transform, or None where it reports the unset NodeId"""
    try:
        return oracle.Vocabulary(voc, scoring, weighting).transform(d, levelsup)
    except oracle.OracleError:
        return None


def _plain(descent, scoring, weighting):
    try:
        return vu.as_arrays(*vu.plain_assemble(descent, scoring, weighting))
    except vu.UnsetNodeId:
        return None


def _cpu(oracle, voc, scoring, weighting, d, levelsup, descent=None):
    """oracle == plain restatement; -> (oracle result or None, descent)"""
    if descent is None:
        descent = vu.plain_descend(voc, d, levelsup)
    r = _oracle(oracle, voc, scoring, weighting, d, levelsup)
    p = _plain(descent, scoring, weighting)
    assert (r is None) == (p is None)
    if r is not None:
        vu.same(r, p)
    return r, descent


def _batch(gpu, gv, frames, kcap, levelsup, fill_seed=99):
    """orbv_transform_batch over the frames (rows past a frame's count hold
    random bytes) -> per frame the arrays in orbv_transform's form"""
    import torch
    B = len(frames)
    desc = _rnd(fill_seed, B * kcap).reshape(B, kcap, 32)
    for f, d in enumerate(frames):
        desc[f, :len(d)] = d
    counts = np.array([len(d) for d in frames], np.int32)
    o = gv.transform_batch(torch.from_numpy(desc).cuda(), torch.from_numpy(counts).cuda(), levelsup)
    gv.check()
    h = {k: v.cpu().numpy() for k, v in o.items()}
    out = []
    for f in range(B):
        nb, nf = int(h["nbow"][f]), int(h["nfv"][f])
        off = h["fv_off"][f, :nf + 1].astype(np.uint32)
        out.append(((h["bow_word"][f, :nb].astype(np.uint32), h["bow_value"][f, :nb].copy()),
                    dict(node_id=h["fv_node"][f, :nf].astype(np.uint32), off=off,
                         feat=h["fv_feat"][f, :int(off[-1])].astype(np.uint32))))
    return out


def _gpu(gpu, oracle, voc, scoring, weighting, d, levelsup, batch=False, gv=None):
    """library == oracle, or ORBX_ERR_ARG where the oracle reports the unset NodeId"""
    gv = gv or gpu.Vocabulary.from_records(voc, scoring, weighting)
    r = _oracle(oracle, voc, scoring, weighting, d, levelsup)
    if r is None:
        with pytest.raises(gpu.OrbxError) as e:
            gv.transform(d, levelsup)
        assert e.value.code == gpu.ERR_ARG
        return gv
    vu.same(gv.transform(d, levelsup), r)
    if batch and len(d):
        vu.same(_batch(gpu, gv, [d], len(d), levelsup)[0], r)
    return gv


# --------------------------------------------------------------------------- 1. branching factor
BRANCH_K = [1, 15, 16, 17, 20]


@pytest.mark.parametrize("k", BRANCH_K)
def test_branching_factor_cpu(oracle, k):
    voc = synth.vocabulary(k, 3, seed=k)
    d = _rnd(1, 2000)
    r, descent = _cpu(oracle, voc, 0, 0, d, 1)
    late = sum(f["path"][0][0] >= 16 for f in descent)  # level 1: second trip of the lane loop
    if k > 16:
        assert late >= 50
    else:
        assert late == 0
    if k == 1:
        (bw, bv), fv = r
        assert len(bw) == 1 and len(fv["node_id"]) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("k", BRANCH_K)
def test_branching_factor_gpu(gpu, oracle, k):
    _gpu(gpu, oracle, synth.vocabulary(k, 3, seed=k), 0, 0, _rnd(1, 2000), 1, batch=True)


# --------------------------------------------------------------------------- 2. ties across the lane group
TWINS = [(0, 16), (2, 18), (3, 19), (15, 16)]
SAME_TRIP = (4, 9)      # both twins in the first trip, in two lanes
TIE_ALL = 9             # level-1 node whose 20 children are all one descriptor


@functools.lru_cache(maxsize=None)
def _tie_case(swap=False):
    """k 20, L 2.  Lane j of a descriptor's 16 scores children j and j + 16.
    (0, 16), (2, 18), (3, 19): the later twin is the same lane's second trip;
    (15, 16): lane 15's first trip against lane 0's second; (4, 9): two lanes
    of one trip.  (0, 16) and (15, 16) both write child 16 and exclude each
    other in one node, so there are two vocabularies: in the first the root
    and node 5 take the first three pairs and nodes 6 and 7 the last three,
    in the second (swap) the other way round, so that the root and level 1
    each see all four pairs; all of them take (4, 9), and node 9's children
    are all one descriptor.
    -> (voc, desc, planted [(feature, level, lower index)])"""
    voc = synth.vocabulary(20, 2, seed=22 if swap else 21, stop_frac=0)
    first, last = TWINS[:3] + [SAME_TRIP], TWINS[1:] + [SAME_TRIP]
    if swap:
        first, last = last, first
    sets = {0: first, 5: first, 6: last, 7: last}
    for node, pairs in sets.items():
        voc = vu.with_twin_children(voc, node, pairs)
    voc = vu.with_twin_children(voc, TIE_ALL, [(0, b) for b in range(1, 20)])
    sets[TIE_ALL] = [(0, 19)]
    rows, planted = [], []
    for node, pairs in sets.items():
        ch = vu.children_of(voc, node)
        for a, b in pairs:
            for _ in range(10):
                planted.append((len(rows), 0 if node == 0 else 1, a))
                rows.append(voc["desc"][ch[a]])
    return voc, np.concatenate([np.stack(rows), _rnd(2, 500)]), tuple(planted), sets


@pytest.mark.parametrize("swap", [False, True])
def test_ties_cpu(oracle, swap):
    voc, d, planted, sets = _tie_case(swap)
    assert len(planted) == 10 * (4 * 4 + 1)
    assert ((15, 16) in sets[0]) == swap and ((0, 16) in sets[0]) != swap
    for scoring, weighting in ((0, 0), (1, 2)):
        r, descent = _cpu(oracle, voc, scoring, weighting, d, 1)
    for i, level, lower in planted:
        pick, tie = descent[i]["path"][level]
        assert tie and pick == lower, (i, level, lower, pick, tie)
    # the oracle alone: a copy of twin (2, 18) of node 5 lands in record 2's word
    assert (2, 18) in sets[5]
    ch = vu.children_of(voc, 5)
    words = np.cumsum(voc["is_leaf"] > 0) - 1
    (bw, _), _ = oracle.Vocabulary(voc).transform(voc["desc"][ch[18]][None], 1)
    assert bw.tolist() == [words[ch[2]]]


@pytest.mark.gpu
@pytest.mark.parametrize("swap", [False, True])
def test_ties_gpu(gpu, oracle, swap):
    voc, d, _, _ = _tie_case(swap)
    _gpu(gpu, oracle, voc, 0, 0, d, 1, batch=True)
    _gpu(gpu, oracle, voc, 1, 2, d, 1)


# --------------------------------------------------------------------------- 3. more children than k
@functools.lru_cache(maxsize=None)
def _wide_root():
    """the loader never checks a node's child count against k: 40 root children
    under a header k of 10; the 30 appended ones are leaves at level 1"""
    voc = vu.with_extra_root_children(synth.vocabulary(10, 2, seed=9, stop_frac=0), 30,
                                      np.random.default_rng(9))
    n = len(voc["parent"])
    return voc, vu.with_weights(voc, np.arange(n - 30, n), 0.0), _rnd(9, 700)


def test_more_children_than_k_cpu(oracle):
    voc, stopped, d = _wide_root()
    assert voc["k"] == 10 and len(vu.children_of(voc, 0)) == 40
    r, descent = _cpu(oracle, voc, 0, 0, d, 1)
    nwords = int((voc["is_leaf"] > 0).sum())
    (bw, _), _ = r
    assert len(set(bw.tolist()) & set(range(nwords - 30, nwords))) >= 10
    # levelsup 0: the appended leaves sit above NodeId level 2 -> unset NodeId
    assert _cpu(oracle, voc, 0, 0, d, 0)[0] is None
    # stopped features never read the NodeId
    r, descent = _cpu(oracle, stopped, 0, 0, d, 0)
    assert r is not None
    assert sum(f["nid"] is None for f in descent) >= 10


@pytest.mark.gpu
def test_more_children_than_k_gpu(gpu, oracle):
    voc, stopped, d = _wide_root()
    _gpu(gpu, oracle, voc, 0, 0, d, 1, batch=True)
    gv = _gpu(gpu, oracle, voc, 0, 0, d, 0)       # ORBX_ERR_ARG
    _gpu(gpu, oracle, voc, 0, 0, d, 1, gv=gv)     # and the next call is good again
    _gpu(gpu, oracle, stopped, 0, 0, d, 0, batch=True)


# --------------------------------------------------------------------------- 4. depth and levelsup
DEPTH = [(2, 10, 3, 0.0, lu) for lu in (0, 4, 9, 10, 11)] + \
        [(6, 5, 5, 0.3, lu) for lu in range(6)]


@pytest.mark.parametrize("k,L,seed,prune,levelsup", DEPTH)
def test_depth_and_levelsup_cpu(oracle, k, L, seed, prune, levelsup):
    voc = synth.vocabulary(k, L, seed=seed, prune=prune)
    r, descent = _cpu(oracle, voc, 0, 0, _rnd(4, 600), levelsup)
    if levelsup >= L:  # NodeId level <= 0: every kept feature under the root
        assert r[1]["node_id"].tolist() == [0]
    if prune == 0.0:
        assert r is not None and all(len(f["path"]) == L for f in descent)


@pytest.mark.gpu
@pytest.mark.parametrize("k,L,seed,prune,levelsup", DEPTH)
def test_depth_and_levelsup_gpu(gpu, oracle, k, L, seed, prune, levelsup):
    _gpu(gpu, oracle, synth.vocabulary(k, L, seed=seed, prune=prune), 0, 0, _rnd(4, 600), levelsup)


# --------------------------------------------------------------------------- 5. scoring x weighting
COMBOS = [(s, w) for s in range(6) for w in range(4)]


@functools.lru_cache(maxsize=None)
def _combo_case():
    voc = vu.with_weights(synth.vocabulary(6, 2, seed=7), [40, 41], [-1.0, np.nan])  # w > 0 fails
    return voc, _rnd(3, 700)


def test_all_scorings_and_weightings_cpu(oracle):
    voc, d = _combo_case()
    assert voc["is_leaf"][40] and voc["is_leaf"][41]
    descent = vu.plain_descend(voc, d, 1)
    res = {c: _cpu(oracle, voc, c[0], c[1], d, 1, descent)[0] for c in COMBOS}
    kept = [f for f in descent if f["weight"] > 0]
    per_word = np.bincount([f["word"] for f in kept])
    assert (per_word >= 2).sum() >= 20  # summation order and the first-value rule matter
    assert len(kept) < len(d)           # and some features are stopped
    assert sum(f["weight"] < 0 for f in descent) >= 5          # the negative weight is reached,
    assert sum(np.isnan(f["weight"]) for f in descent) >= 5    # and the NaN one
    for w in range(4):
        for s in (2, 3, 4):  # chi-square, KL, Bhattacharyya normalise like L1
            vu.same(res[(s, w)], res[(0, w)])
        assert not np.array_equal(res[(1, w)][0][1], res[(0, w)][0][1])
        assert not np.array_equal(res[(5, w)][0][1], res[(0, w)][0][1])


@pytest.mark.gpu
@pytest.mark.parametrize("scoring,weighting", COMBOS)
def test_all_scorings_and_weightings_gpu(gpu, oracle, scoring, weighting):
    voc, d = _combo_case()
    _gpu(gpu, oracle, voc, scoring, weighting, d, 1, batch=True)


# --------------------------------------------------------------------------- 6. degenerate contents
def _empty_vocabulary():
    return dict(k=10, L=3, parent=np.zeros(0, np.int32), is_leaf=np.zeros(0, np.int32),
                desc=np.zeros((0, 32), np.uint8), weight=np.zeros(0, np.float64))


@functools.lru_cache(maxsize=None)
def _degenerate_cases():
    """-> [(name, voc, scoring, weighting, desc, levelsup)]"""
    cases = []
    allstop = synth.vocabulary(6, 2, seed=6, stop_frac=1.0)
    for s in range(6):  # norm == 0 (or no division for the dot product): empty vectors
        cases.append(("stopped-s%d" % s, allstop, s, 0, _rnd(6, 300), 1))
    cases.append(("no-records", _empty_vocabulary(), 0, 0, _rnd(6, 40), 1))
    voc = synth.vocabulary(10, 4, seed=8, stop_frac=0)
    leaves = np.flatnonzero(voc["is_leaf"] > 0)
    one = np.repeat(voc["desc"][leaves[123]][None], 1025, 0)
    cases.append(("one-word-tfidf", voc, 0, 0, one, 2))  # one thread's 1025 in-order additions
    cases.append(("one-word-idf", voc, 0, 2, one, 2))
    cases.append(("one-word-l2", voc, 1, 0, one, 2))
    # copies of 1025 different leaves; a copy can still descend into another
    # word (a sibling subtree nearer than its own), so leaves are taken until
    # 1025 of them land in words of their own
    cand = voc["desc"][np.random.default_rng(8).choice(leaves, 1200, replace=False)]
    seen, rows = set(), []
    for i, f in enumerate(vu.plain_descend(voc, cand, 2)):
        if f["word"] not in seen and len(rows) < 1025:
            seen.add(f["word"])
            rows.append(i)
    cases.append(("each-word-once", voc, 0, 0, cand[rows], 2))
    cases.append(("each-word-once-l2", voc, 1, 1, cand[rows], 2))
    return cases


def test_degenerate_contents_cpu(oracle):
    for name, voc, s, w, d, lu in _degenerate_cases():
        r, descent = _cpu(oracle, voc, s, w, d, lu)
        (bw, bv), fv = r
        if name.startswith("stopped") or name == "no-records":
            assert len(bw) == 0 and len(fv["node_id"]) == 0 and fv["off"].tolist() == [0], name
        elif name.startswith("one-word"):
            assert len(bw) == 1 and fv["feat"].tolist() == list(range(1025)), name
            wt = descent[0]["weight"]
            acc = 0.0
            for _ in range(1025):
                acc += wt
            assert acc != 1025 * wt  # the in-order sum is not the product: order shows
            assert bv.tolist() == [1.0]
        else:
            assert len(bw) == 1025 and len(fv["feat"]) == 1025, name


@pytest.mark.gpu
def test_degenerate_contents_gpu(gpu, oracle):
    for name, voc, s, w, d, lu in _degenerate_cases():
        _gpu(gpu, oracle, voc, s, w, d, lu, batch=True)


def test_one_word_raw_sum_cpu(oracle):
    """the 1025 in-order additions, seen un-normalised (dot product divides by
    the one word); under IDF the single weight"""
    name, voc, _, _, one, lu = _degenerate_cases()[7]
    assert name == "one-word-tfidf"
    (bw, bv), _ = _cpu(oracle, voc, 5, 0, one, lu)[0]
    wt = vu.plain_descend(voc, one[:1], lu)[0]["weight"]
    acc = 0.0
    for _ in range(1025):
        acc += wt
    assert bv.tolist() == [acc]
    (bw, bv), _ = _cpu(oracle, voc, 5, 2, one, lu)[0]
    assert bv.tolist() == [wt]


@pytest.mark.gpu
def test_one_word_raw_sum_gpu(gpu, oracle):
    _, voc, _, _, one, lu = _degenerate_cases()[7]
    _gpu(gpu, oracle, voc, 5, 0, one, lu)
    _gpu(gpu, oracle, voc, 5, 2, one, lu)


# --------------------------------------------------------------------------- 7. sizes
SIZES = [1, 2, 15, 16, 17, 1023, 1024, 1025, 2047, 2049, 8191, 8192]


@functools.lru_cache(maxsize=None)
def _size_case():
    return synth.vocabulary(10, 3), _rnd(7, 8193)


def test_sizes_cpu(oracle):
    voc, d = _size_case()
    descent = vu.plain_descend(voc, d, 1)
    for n in SIZES + [3]:
        for scoring in (0, 1):
            _cpu(oracle, voc, scoring, 0, d[:n], 1, descent[:n])
    # at least one L2 case tells the fused square-accumulate from the unfused
    # one (the square root hides most differences of the last bit)
    raw = [vu.plain_bow(descent[:n], 0)[1] for n in SIZES]
    assert any(vu.l2_norm(v) != vu.l2_norm(v, fused=False) for v in raw)


@pytest.mark.gpu
@pytest.mark.parametrize("scoring", [0, 1])
def test_sizes_gpu(gpu, oracle, scoring):
    voc, d = _size_case()
    gv = gpu.Vocabulary.from_records(voc, scoring, 0)
    for n in SIZES:
        _gpu(gpu, oracle, voc, scoring, 0, d[:n], 1, batch=n in (1, 1024, 1025, 8192), gv=gv)


@pytest.mark.gpu
def test_sizes_beyond_the_sort_gpu(gpu, oracle):
    import torch
    voc, d = _size_case()
    gv = gpu.Vocabulary.from_records(voc)
    with pytest.raises(gpu.OrbxError) as e:
        gv.transform(d[:8193], 1)
    assert e.value.code == gpu.ERR_UNSUPPORTED
    _gpu(gpu, oracle, voc, 0, 0, d[:100], 1, gv=gv)
    with pytest.raises(gpu.OrbxError) as e:
        gv.transform_batch(torch.from_numpy(d[:8193][None].copy()).cuda(),
                           torch.tensor([8193], dtype=torch.int32).cuda(), 1)
    assert e.value.code == gpu.ERR_UNSUPPORTED
    gv.check()
    _gpu(gpu, oracle, voc, 0, 0, d[:100], 1, batch=True, gv=gv)


@pytest.mark.gpu
def test_sizes_staging_reuse_gpu(gpu, oracle):
    """8192, 3, 8192 on one vocabulary: the staging grows once and is reused,
    and the result buffer grows from a small first call"""
    voc, d = _size_case()
    gv = gpu.Vocabulary.from_records(voc)
    for n in (3, 8192, 3, 8192):
        _gpu(gpu, oracle, voc, 0, 0, d[:n], 1, gv=gv)
    gv = gpu.Vocabulary.from_records(voc)
    for n in (8192, 3, 8192):
        _gpu(gpu, oracle, voc, 0, 0, d[8192 - n:8192], 1, gv=gv)


# --------------------------------------------------------------------------- 8. batch
KCAPS = [1500, 1024, 1025]


def _batch_frames(kcap):
    d = _rnd(8, 3 * kcap + 20)
    counts = [0, 1, kcap, 17, kcap - 1, 0]
    frames, at = [], 0
    for c in counts:
        frames.append(d[at:at + c])
        at += c
    return frames


@pytest.mark.parametrize("kcap", KCAPS)
def test_batch_cpu(oracle, kcap):
    voc = synth.vocabulary(10, 3)
    for d in _batch_frames(kcap):
        _cpu(oracle, voc, 0, 0, d, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("kcap", KCAPS)
def test_batch_gpu(gpu, oracle, kcap):
    voc = synth.vocabulary(10, 3)
    frames = _batch_frames(kcap)
    for scoring in (0, 1):
        gv = gpu.Vocabulary.from_records(voc, scoring, 0)
        ov = oracle.Vocabulary(voc, scoring, 0)
        got = _batch(gpu, gv, frames, kcap, 1)
        for g, d in zip(got, frames):
            vu.same(g, ov.transform(d, 1))
    (bw, _), fv = got[0]
    assert len(bw) == 0 and fv["off"].tolist() == [0]


# --------------------------------------------------------------------------- 9. latched NodeId error
@functools.lru_cache(maxsize=None)
def _latch_case():
    """the wide-root vocabulary at levelsup 0 (NodeId level 2): copies of
    level-2 leaves are fine, a copy of an appended level-1 leaf is kept
    (weight > 0) and never reaches level 2"""
    voc, _, _ = _wide_root()
    n = len(voc["parent"])
    deep = voc["desc"][np.flatnonzero(voc["parent"] > 0)]
    pick = np.random.default_rng(10).choice(len(deep), 90, replace=False)
    frames = [deep[pick[:30]], deep[pick[30:60]], deep[pick[60:]]]
    bad = [f.copy() for f in frames]
    bad[1][11] = voc["desc"][n - 7]
    return voc, frames, bad


def test_latched_nodeid_error_cpu(oracle):
    voc, frames, bad = _latch_case()
    assert voc["weight"][len(voc["parent"]) - 7] > 0
    for f in range(3):
        assert _cpu(oracle, voc, 0, 0, frames[f], 0)[0] is not None
        assert (_cpu(oracle, voc, 0, 0, bad[f], 0)[0] is None) == (f == 1)


@pytest.mark.gpu
def test_latched_nodeid_error_gpu(gpu, oracle):
    import torch
    voc, frames, bad = _latch_case()
    gv = gpu.Vocabulary.from_records(voc)
    desc = torch.from_numpy(np.stack(bad)).cuda()
    counts = torch.tensor([30, 30, 30], dtype=torch.int32).cuda()
    gv.transform_batch(desc, counts, 0)
    with pytest.raises(gpu.OrbxError) as e:
        gv.check()
    assert e.value.code == gpu.ERR_ARG
    gv.check()  # reported once: the latch is cleared
    ov = oracle.Vocabulary(voc)
    for g, d in zip(_batch(gpu, gv, frames, 30, 0), frames):
        vu.same(g, ov.transform(d, 0))


# --------------------------------------------------------------------------- text loader
LOADER = [(v, crlf) for v in ("clean", "nofinal", "blank", "cut", "wrap", "expweight")
          for crlf in (False, True)]


@functools.lru_cache(maxsize=None)
def _loader_lines():
    voc = synth.vocabulary(10, 4, seed=11)
    lines = ["%d %d 0 0" % (voc["k"], voc["L"])]
    for p, l, d, w in zip(voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"]):
        lines.append("%d %d %s %s" % (p, l, " ".join(str(int(x)) for x in d), repr(float(w))))
    return voc, lines


def _loader_variant(path, variant, crlf):
    """writes the file -> the records both loaders must read from it.  For
    'nofinal', 'wrap' and 'expweight' (and CRLF) that is what the reference's
    operator>> reads; for 'blank' and 'cut' it is the project's documented
    rule (vocabulary loader): blank lines are skipped, where the
    reference makes each a phantom child of the root and shifts the later
    node ids, and a failed extraction reads as 0, where the reference leaves
    the remaining descriptor bytes uninitialised."""
    voc, lines = _loader_lines()
    voc, lines = vu._copy(voc), list(lines)
    n = len(voc["parent"])
    final = True
    if variant == "nofinal":
        final = False
    elif variant == "blank":
        lines[n // 2:n // 2] = ["", ""]
    elif variant == "cut":  # 20 numbers: parent, isLeaf, 18 bytes; the rest reads as 0
        lines[-1] = " ".join(lines[-1].split()[:20])
        voc["desc"][n - 1, 18:] = 0
        voc["weight"][n - 1] = 0.0
    elif variant == "wrap":  # FORB::fromString: (unsigned char)n
        for rec in (0, 3, 9, n - 2):
            t = lines[1 + rec].split()
            t[2], t[3], t[4] = "256", "511", "-1"
            lines[1 + rec] = " ".join(t)
            voc["desc"][rec, :3] = [0, 255, 255]
    elif variant == "expweight":
        leaves = np.flatnonzero(voc["is_leaf"] > 0)
        for rec in leaves[:200]:
            t = lines[1 + rec].split()
            t[34] = "%.17e" % voc["weight"][rec]  # 17 digits: the same double
            lines[1 + rec] = " ".join(t)
        t = lines[1 + leaves[200]].split()
        t[34] = "1.5e+00"
        lines[1 + leaves[200]] = " ".join(t)
        voc["weight"][leaves[200]] = 1.5
    eol = "\r\n" if crlf else "\n"
    with open(path, "wb") as f:
        f.write((eol.join(lines) + (eol if final else "")).encode())
    return voc


@pytest.mark.parametrize("variant,crlf", LOADER)
def test_text_loader_variants_cpu(oracle, tmp_path, variant, crlf):
    p = tmp_path / "voc.txt"
    want = _loader_variant(p, variant, crlf)
    back = oracle.parse_vocabulary_text(p)
    assert (back["k"], back["L"], back["scoring"], back["weighting"]) == (10, 4, 0, 0)
    for key in ("parent", "is_leaf", "desc"):
        assert np.array_equal(back[key], want[key]), key
    assert np.array_equal(back["weight"].view(np.uint64), want["weight"].view(np.uint64))


@pytest.mark.gpu
@pytest.mark.parametrize("variant,crlf", LOADER)
def test_text_loader_variants_gpu(gpu, oracle, tmp_path, variant, crlf):
    p = tmp_path / "voc.txt"
    _loader_variant(p, variant, crlf)
    back = oracle.parse_vocabulary_text(p)
    gv = gpu.Vocabulary.load_text(p)
    assert gv.info() == dict(k=back["k"], L=back["L"], scoring=back["scoring"],
                             weighting=back["weighting"], nnodes=len(back["parent"]) + 1,
                             nwords=int((back["is_leaf"] > 0).sum()))
    d = _rnd(3, 500)
    vu.same(gv.transform(d, 2), oracle.Vocabulary.load_text(p).transform(d, 2))
