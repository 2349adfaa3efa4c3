"""A second opinion on the oracle's vocabulary transform, and planted
vocabularies for tests/test_vocabulary_edges.py.

plain_transform restates TemplatedVocabulary::transform
(Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1126-1259) and
BowVector::normalize (BowVector.cpp:61-83) in plain Python/numpy: child lists
in record order, np.unpackbits Hamming distances, a dict as the BowVector.  It
shares no code with oracle/orb_oracle.c, so a mistake in the oracle's CSR
tables, sort or summation order shows as a difference between the two.

The builders plant what orbx.synth.vocabulary never produces: children that
are byte copies of each other (ties), more children than the header's k, and
chosen weights.
"""
import math
from fractions import Fraction

import numpy as np


class UnsetNodeId(Exception):
    """the reference would read the NodeId of a feature that never reached
    level L - levelsup (a kept feature that ends in a shallower leaf)"""


def _tables(voc):
    parent = np.asarray(voc["parent"], np.int64)
    n = len(parent) + 1
    children = [[] for _ in range(n)]
    for rec, pid in enumerate(parent):  # m_nodes[pid].children.push_back(nid), :1401
        children[int(pid)].append(rec + 1)
    desc = np.asarray(voc["desc"], np.uint8).reshape(-1, 32)
    bits = np.zeros((n, 256), np.uint8)
    if n > 1:
        bits[1:] = np.unpackbits(desc, axis=1)
    word = np.zeros(n, np.int64)  # Node(): word_id(0)
    weight = np.zeros(n, np.float64)
    nwords = 0
    for rec, leaf in enumerate(voc["is_leaf"]):  # :1412-1418: words in record order
        weight[rec + 1] = voc["weight"][rec]
        if leaf > 0:
            word[rec + 1] = nwords
            nwords += 1
    return children, bits, word, weight, nwords


def plain_descend(voc, desc, levelsup):
    """transform(feature, word_id, weight, nid, levelsup) (:1217-1259) per
    descriptor -> list of dict(word, weight, nid (None: unset), path
    [(child index chosen, tie at the minimum)] per level)."""
    children, bits, word, weight, nwords = _tables(voc)
    if nwords == 0:
        return None  # empty(): transform returns before any descent (:1134)
    nid_level = int(voc["L"]) - levelsup
    d = np.asarray(desc, np.uint8).reshape(-1, 32)
    fbits = np.unpackbits(d, axis=1) if len(d) else np.zeros((0, 256), np.uint8)
    cbits = {}  # node -> its children's descriptors as bit rows
    out = []
    for fb in fbits:
        nid = 0 if nid_level <= 0 else None
        node, level, path = 0, 0, []
        while True:
            level += 1
            ch = children[node]
            if node not in cbits:
                cbits[node] = bits[ch]
            dist = np.count_nonzero(cbits[node] ^ fb, axis=1).tolist()
            best, pick = dist[0], 0
            for j in range(1, len(ch)):
                if dist[j] < best:  # strict: the first minimum stays
                    best, pick = dist[j], j
            path.append((pick, dist.count(best) > 1))
            node = ch[pick]
            if level == nid_level:
                nid = node
            if not children[node]:  # isLeaf(): children.empty()
                break
        out.append(dict(word=int(word[node]), weight=float(weight[node]), nid=nid, path=path))
    return out


def plain_bow(descent, weighting):
    """the BowVector before :1164-1170 and normalize, and the FeatureVector
    -> (sorted words, their values, {node: [features]})"""
    bow, fv = {}, {}
    tf = weighting in (0, 1)  # TF_IDF, TF: addWeight; IDF, BINARY: addIfNotExist
    for i, r in enumerate(descent or []):
        if not r["weight"] > 0:  # stopped (also NaN)
            continue
        if r["nid"] is None:
            raise UnsetNodeId(i)
        if r["word"] not in bow:
            bow[r["word"]] = r["weight"]
        elif tf:
            bow[r["word"]] += r["weight"]
        fv.setdefault(r["nid"], []).append(i)
    words = sorted(bow)
    return words, [bow[w] for w in words], fv


def l2_norm(vals, fused=True):
    """BowVector::normalize's L2 sum in ascending word order; fused: each
    square-accumulate rounded once (a fused multiply-add, as -march=native
    compiles it), else the product and the sum rounded separately"""
    norm = 0.0
    for v in vals:
        norm = float(Fraction(v) * Fraction(v) + Fraction(norm)) if fused else norm + v * v
    return math.sqrt(norm)


def plain_assemble(descent, scoring, weighting):
    """transform(features, BowVector, FeatureVector, levelsup) (:1126-1194) on
    the per-feature results -> (words u32, values f64, {node: [features]})."""
    words, vals, fv = plain_bow(descent, weighting)
    if scoring == 5:  # DotProductScoring: mustNormalize false
        if weighting in (0, 1) and vals:  # :1164-1170
            nd = float(len(vals))
            vals = [v / nd for v in vals]
    else:
        if scoring == 1:
            norm = l2_norm(vals)
        else:  # L1, also for chi-square, KL and Bhattacharyya (ScoringObject.h:74-89)
            norm = 0.0
            for v in vals:
                norm += abs(v)
        if norm > 0.0:
            vals = [v / norm for v in vals]
    return np.array(words, np.uint32), np.array(vals, np.float64), fv


def plain_transform(voc, scoring, weighting, desc, levelsup):
    """-> (words, values, {node: [features]}, paths); raises UnsetNodeId where
    the reference would read an unset NodeId."""
    descent = plain_descend(voc, desc, levelsup)
    words, vals, fv = plain_assemble(descent, scoring, weighting)
    return words, vals, fv, [r["path"] for r in descent or []]


def as_arrays(words, vals, fv):
    """the oracle's output form: ((words, values), dict(node_id, off, feat))"""
    nodes = sorted(fv)
    off = np.zeros(len(nodes) + 1, np.uint32)
    off[1:] = np.cumsum([len(fv[n]) for n in nodes])
    feat = np.array([i for n in nodes for i in fv[n]], np.uint32)
    return (words, vals), dict(node_id=np.array(nodes, np.uint32), off=off, feat=feat)


def same(a, b):
    """tests/test_vocabulary.py _same: ids exact, values bit for bit"""
    (abw, abv), afv = a
    (bbw, bbv), bfv = b
    assert np.array_equal(abw, bbw)
    assert np.array_equal(abv.view(np.uint64), bbv.view(np.uint64))
    for key in ("node_id", "off", "feat"):
        assert np.array_equal(afv[key], bfv[key]), key


# --------------------------------------------------------------------------- builders
def _copy(voc):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in voc.items()}


def children_of(voc, node):
    """record indices (node id - 1) of a node's children, in record order"""
    return np.flatnonzero(np.asarray(voc["parent"]) == node)


def with_twin_children(voc, node, pairs):
    """child b of `node` becomes a byte copy of child a, for (a, b) in pairs"""
    v = _copy(voc)
    ch = children_of(v, node)
    for a, b in pairs:
        v["desc"][ch[b]] = v["desc"][ch[a]]
    return v


def with_extra_root_children(voc, n, rng):
    """n leaf records appended under the root (random descriptors, weights in
    (0.1, 8)); the header's k is left alone"""
    v = _copy(voc)
    v["parent"] = np.concatenate([v["parent"], np.zeros(n, np.int32)])
    v["is_leaf"] = np.concatenate([v["is_leaf"], np.ones(n, np.int32)])
    v["desc"] = np.concatenate([v["desc"], rng.integers(0, 256, (n, 32), dtype=np.uint8)])
    v["weight"] = np.concatenate([v["weight"], rng.uniform(0.1, 8.0, n)])
    return v


def with_weights(voc, idx, values):
    v = _copy(voc)
    v["weight"][np.asarray(idx)] = values
    return v
