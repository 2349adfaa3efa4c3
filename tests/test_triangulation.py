"""The CPU restatement of ORBmatcher::SearchForTriangulation
(tests/cpp/triangulation_ref.c) against known answers: CheckDistEpipolarLine
worked by hand in exact rational arithmetic (one rounding per operation, in
the order the reference's object performs them), and the search on
containers of a handful of features.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

import triangulation_util as T


# --------------------------------------------------------------------------- exact arithmetic
def _round(fr, mant, emin):
    """fr (a Fraction) rounded to nearest-even in a binary format with `mant`
    significand bits and least exponent emin (of the last place)"""
    if fr == 0:
        return Fraction(0)
    s = -1 if fr < 0 else 1
    v = abs(fr)
    e = v.numerator.bit_length() - v.denominator.bit_length()
    if Fraction(2) ** e > v:
        e -= 1
    assert Fraction(2) ** e <= v < Fraction(2) ** (e + 1)
    q = max(e - (mant - 1), emin)
    m = v / Fraction(2) ** q
    lo = m.numerator // m.denominator
    rem = m - lo
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and lo % 2 == 1):
        lo += 1
    return s * lo * Fraction(2) ** q


def r32(fr):
    return _round(fr, 24, -149)


def r64(fr):
    return _round(fr, 53, -1074)


def f(x):
    return Fraction(float(np.float32(x)))


def hand_epipolar(x1, y1, x2, y2, F12, s2, fused=True, float_compare=False):
    """CheckDistEpipolarLine (ORBmatcher.cc:71-85) by hand.  fused: the
    reference object's form (one product of each pair fused into the add);
    else source order, every operation rounded."""
    F = [[f(v) for v in row] for row in np.asarray(F12, np.float32).reshape(3, 3)]
    x1, y1, x2, y2, s2 = f(x1), f(y1), f(x2), f(y2), f(s2)
    if fused:
        a = r32(r32(x1 * F[0][0] + r32(y1 * F[1][0])) + F[2][0])
        b = r32(r32(x1 * F[0][1] + r32(y1 * F[1][1])) + F[2][1])
        c = r32(r32(y1 * F[1][2] + r32(x1 * F[0][2])) + F[2][2])
        den = r32(a * a + r32(b * b))
        num = r32(r32(b * y2 + r32(a * x2)) + c)
    else:
        a = r32(r32(r32(x1 * F[0][0]) + r32(y1 * F[1][0])) + F[2][0])
        b = r32(r32(r32(x1 * F[0][1]) + r32(y1 * F[1][1])) + F[2][1])
        c = r32(r32(r32(x1 * F[0][2]) + r32(y1 * F[1][2])) + F[2][2])
        num = r32(r32(r32(a * x2) + r32(b * y2)) + c)
        den = r32(r32(a * a) + r32(b * b))
    if den == 0:
        return False
    dsqr = r32(r32(num * num) / den)
    thr = r64(Fraction(3.84) * s2)
    if float_compare:
        return dsqr < r32(thr)
    return dsqr < thr


def _random_vector(rng):
    R2 = T._rot(rng.uniform(-0.03, 0.03), rng.uniform(-0.08, 0.08), rng.uniform(-0.05, 0.05))
    t2 = np.array([rng.uniform(0.3, 1.0), rng.uniform(-0.1, 0.1), rng.uniform(-0.1, 0.1)])
    F = T.fundamental(np.eye(3), np.zeros(3), R2, t2)
    x1, y1 = np.float32(rng.uniform(0, 640)), np.float32(rng.uniform(0, 480))
    x2, y2 = np.float32(rng.uniform(0, 640)), np.float32(rng.uniform(0, 480))
    s2 = T.level_sigma2()[rng.randint(0, 8)]
    return x1, y1, x2, y2, F, s2


def test_epipolar_fused_form_decides_where_source_order_differs():
    """A vector on which the object's fused form and the source-order form
    disagree, found by a bounded seeded search; the restatement gives the
    fused decision, and both agree with the hand computation."""
    rng = np.random.RandomState(20260)
    found = None
    for _ in range(40):
        x1, y1, x2, y2, F, s2 = _random_vector(rng)
        p = T.boundary_point(float(x1), float(y1), float(x2), float(y2), F, float(s2), span=200)
        if p is not None:
            found = (x1, y1, np.float32(p[0]), np.float32(p[1]), F, s2)
            break
    assert found is not None, "no vector separates the two forms in 40 draws"
    x1, y1, x2, y2, F, s2 = found
    fused, written = hand_epipolar(x1, y1, x2, y2, F, s2), hand_epipolar(x1, y1, x2, y2, F, s2, fused=False)
    assert fused != written
    assert T.epipolar(x1, y1, x2, y2, F, s2) == fused
    assert T.epipolar(x1, y1, x2, y2, F, s2, written=True) == written


def test_epipolar_matches_hand_computation_on_random_vectors():
    rng = np.random.RandomState(7)
    seen = set()
    for i in range(120):
        x1, y1, x2, y2, F, s2 = _random_vector(rng)
        if i % 2:  # onto the line, then off it by about the threshold
            Fd = F.astype(np.float64)
            a = x1 * Fd[0, 0] + y1 * Fd[1, 0] + Fd[2, 0]
            b = x1 * Fd[0, 1] + y1 * Fd[1, 1] + Fd[2, 1]
            c = x1 * Fd[0, 2] + y1 * Fd[1, 2] + Fd[2, 2]
            d = (a * x2 + b * y2 + c) / math.hypot(a, b) - rng.uniform(0.5, 1.5) * math.sqrt(3.84 * s2)
            x2, y2 = np.float32(x2 - d * a / math.hypot(a, b)), np.float32(y2 - d * b / math.hypot(a, b))
        want = hand_epipolar(x1, y1, x2, y2, F, s2)
        assert T.epipolar(x1, y1, x2, y2, F, s2) == want
        seen.add(want)
    assert seen == {True, False}


def test_epipolar_zero_denominator_is_false():
    F = np.zeros((3, 3), np.float32)
    F[2, 2] = 1.0  # a = b = 0: den == 0 (:79-81)
    assert hand_epipolar(10, 20, 30, 40, F, 1.0) is False
    assert T.epipolar(10, 20, 30, 40, F, 1.0) is False
    # a den that underflows to zero as well
    F[2, 0] = 1e-30
    assert hand_epipolar(0, 0, 0, 0, F, 1.0) is False
    assert T.epipolar(0, 0, 0, 0, F, 1.0) is False
    # and the same point passes once den is representable (num == c == 0 here)
    F[2, 0], F[2, 2] = 1.0, 0.0
    assert T.epipolar(0, 0, 0, 0, F, 1.0) is True


@pytest.mark.parametrize("pos", range(9))
def test_epipolar_nan_in_f12_is_false(pos):
    """NaN reaches den or num: `den == 0` is false, the final compare too."""
    F = T.fundamental(np.eye(3), np.zeros(3), T._rot(0.01, 0.05, 0.02), np.array([0.7, 0.05, -0.03])).reshape(9)
    F[pos] = np.nan
    for x2, y2 in ((100.0, 100.0), (320.0, 240.0), (0.0, 0.0)):
        assert T.epipolar(300.0, 200.0, x2, y2, F, 50.0) is False


def test_epipolar_threshold_is_compared_in_double():
    """dsqr == (float)(3.84 * s2) with the double product above it: the
    reference's double compare accepts, a float compare would not."""
    F = np.zeros((3, 3), np.float32)
    F[2, 0] = 1.0  # a = 1, b = 0, c = 0: num = x2, den = 1, dsqr = x2 * x2
    found = None
    for k in range(65, 256):
        q = Fraction(k, 64)  # q * q is exact in float
        s0 = np.float32(float(q * q) / 3.84)
        for step in range(-3, 4):
            s2 = T._step(s0, step)
            thr = r64(Fraction(3.84) * f(s2))
            if r32(thr) == q * q and thr > q * q:
                found = (np.float32(float(q)), s2)
                break
        if found:
            break
    assert found is not None
    x2, s2 = found
    assert hand_epipolar(5.0, 6.0, x2, 7.0, F, s2) is True
    assert hand_epipolar(5.0, 6.0, x2, 7.0, F, s2, float_compare=True) is False
    assert T.epipolar(5.0, 6.0, x2, 7.0, F, s2) is True


def test_descriptor_distance():
    rng = np.random.RandomState(3)
    for _ in range(50):
        a, b = rng.randint(0, 256, 32).astype(np.uint8), rng.randint(0, 256, 32).astype(np.uint8)
        want = int(np.unpackbits(a ^ b).sum())
        assert T.ref_lib().tri_descriptor_distance(T._ptr(a), T._ptr(b)) == want


# --------------------------------------------------------------------------- containers
# F12 with a = 0, b = 1, c = 0: the epipolar line of every kp1 is y = 0 in
# image 2 and dsqr = y2 * y2; with sigma2 = 1, y2 = 0 passes and y2 = 10 fails
F_Y0 = np.array([[0, 0, 0], [0, 0, 0], [0, 1, 0]], np.float32)
S2_ONE = np.ones(8, np.float32)


def fam(f_, extra=0):
    """descriptor of family f_ (32 private bits: families are 64 apart) with
    `extra` more bits set at the far end"""
    d = np.zeros(32, np.uint8)
    d[4 * f_:4 * f_ + 4] = 0xFF
    bits = np.zeros(256, np.uint8)
    bits[256 - extra:] = 1 if extra else 0
    return d | np.packbits(bits)


def frame(feats, lists, has_mp=None):
    """feats: list of (desc, y, angle); lists: {node: [feature indices]}"""
    n = len(feats)
    keys = np.zeros(n, T.KEYPOINT_DTYPE)
    desc = np.zeros((n, 32), np.uint8)
    for i, (d, y, ang) in enumerate(feats):
        desc[i] = d
        keys[i]["x"], keys[i]["y"], keys[i]["angle"] = 7.0 + i, y, ang
    nid, off, feat = T._flatten(n, lists, None)
    mp = np.zeros(n, np.uint8)
    for i in has_mp or []:
        mp[i] = 1
    return dict(keys=keys, desc=desc, has_mp=mp, node_id=nid, off=off, feat=feat, level_sigma2=S2_ONE)


def search(kf1, kf2, **kw):
    m, nm, st = T.ref_search(kf1, kf2, F_Y0, **kw)
    assert nm == int((m >= 0).sum())
    return m.tolist(), nm


def test_tie_at_equal_distance_later_candidate_wins():
    kf1 = frame([(fam(0), 0, 0)], {1: [0]})
    kf2 = frame([(fam(0, 5), 0, 0), (fam(0, 5), 0, 0), (fam(0, 6), 0, 0)], {1: [0, 1, 2]})
    assert search(kf1, kf2, check_ori=False) == ([1], 1)
    # list order, not index order
    kf2 = frame([(fam(0, 5), 0, 0), (fam(0, 5), 0, 0), (fam(0, 6), 0, 0)], {1: [1, 2, 0]})
    assert search(kf1, kf2, check_ori=False) == ([0], 1)
    # a later equal candidate that fails the epipolar test does not replace it
    kf2 = frame([(fam(0, 5), 0, 0), (fam(0, 5), 10, 0)], {1: [0, 1]})
    assert search(kf1, kf2, check_ori=False) == ([0], 1)


def test_distance_50_accepted_51_not():
    kf1 = frame([(fam(0), 0, 0)], {1: [0]})
    assert search(kf1, frame([(fam(0, 50), 0, 0)], {1: [0]}), check_ori=False) == ([0], 1)
    assert search(kf1, frame([(fam(0, 51), 0, 0)], {1: [0]}), check_ori=False) == ([-1], 0)


def test_has_mp_skips_on_each_side():
    kf2 = frame([(fam(0, 1), 0, 0), (fam(0, 9), 0, 0)], {1: [0, 1]})
    assert search(frame([(fam(0), 0, 0)], {1: [0]}), kf2, check_ori=False) == ([0], 1)
    assert search(frame([(fam(0), 0, 0)], {1: [0]}, has_mp=[0]), kf2, check_ori=False) == ([-1], 0)
    kf2 = frame([(fam(0, 1), 0, 0), (fam(0, 9), 0, 0)], {1: [0, 1]}, has_mp=[0])
    assert search(frame([(fam(0), 0, 0)], {1: [0]}), kf2, check_ori=False) == ([1], 1)


def test_lower_bound_skips_non_common_nodes_on_each_side():
    feats = [(fam(i), 0, 0) for i in range(4)]
    a = frame(feats, {1: [0], 2: [1], 3: [2], 10: [3]})
    b = frame(feats, {5: [0], 6: [1], 10: [3], 11: [2]})
    assert search(a, b, check_ori=False) == ([-1, -1, -1, 3], 1)
    assert search(b, a, check_ori=False) == ([-1, -1, -1, 3], 1)
    # the same features under common nodes all match
    assert search(a, a, check_ori=False) == ([0, 1, 2, 3], 4)


def _ang2(bin_):
    """a kp2 angle that puts a kp1 of angle 0 into rotation bin `bin_`"""
    return (360.0 - 30.0 * bin_) % 360.0


def test_superseded_acceptance_in_dropped_bin_resets_the_row():
    """Row 0 first accepts a candidate whose rotation falls in bin 4, then a
    closer one in bin 1.  Bins 1, 2, 3 hold 3, 2, 2 events and are kept, bin 4
    (1 event) is dropped: row 0 is reset although its final bin is kept."""
    kf1 = frame([(fam(i), 0, 0) for i in range(4)], {9: [0, 1, 2, 3]})
    c = [(fam(0, 8), 0, _ang2(4)), (fam(0, 2), 0, _ang2(1)),
         (fam(1, 3), 0, _ang2(2)), (fam(1, 3), 0, _ang2(2)),
         (fam(2, 3), 0, _ang2(3)), (fam(2, 3), 0, _ang2(3)),
         (fam(3, 3), 0, _ang2(1)), (fam(3, 3), 0, _ang2(1))]
    kf2 = frame(c, {9: list(range(8))})
    assert search(kf1, kf2) == ([-2, 3, 5, 7], 3)
    assert search(kf1, kf2, check_ori=False) == ([1, 3, 5, 7], 4)
    # without the superseded candidate the row stays
    kf2 = frame(c, {9: list(range(1, 8))})
    assert search(kf1, kf2) == ([1, 3, 5, 7], 4)


@pytest.mark.parametrize("top,second_kept", [(11, False), (10, True)])
def test_three_maxima_first_cutoff(top, second_kept):
    """topValues[1] < 0.1f * topValues[0] drops the second and third bins
    (:496-498): 1 < 1.1 with 11 events, not with 10."""
    kf1 = frame([(fam(0), 0, 0), (fam(1), 0, 0)], {4: [0, 1]})
    c = [(fam(0, 3), 0, _ang2(1))] * top + [(fam(1, 3), 0, _ang2(2))]
    kf2 = frame(c, {4: list(range(top + 1))})
    assert search(kf1, kf2) == ([top - 1, top if second_kept else -2], 2 if second_kept else 1)


@pytest.mark.parametrize("top,third_kept", [(11, False), (10, True)])
def test_three_maxima_second_cutoff(top, third_kept):
    """topValues[2] < 0.1f * topValues[0] drops the third bin only (:499-500)."""
    kf1 = frame([(fam(0), 0, 0), (fam(1), 0, 0), (fam(2), 0, 0)], {4: [0, 1, 2]})
    c = [(fam(0, 3), 0, _ang2(1))] * top + [(fam(1, 3), 0, _ang2(2))] * 2 + [(fam(2, 3), 0, _ang2(3))]
    kf2 = frame(c, {4: list(range(top + 3))})
    assert search(kf1, kf2) == ([top - 1, top + 1, top + 2 if third_kept else -2], 3 if third_kept else 2)


def test_three_maxima_function():
    z = [0] * 30
    assert T.three_maxima(z) == [-1, -1, -1]
    s = list(z); s[3], s[5], s[12], s[7] = 4, 9, 4, 2
    assert T.three_maxima(s) == [5, 3, 12]  # equal values keep bin order
    s = list(z); s[2], s[8] = 11, 1
    assert T.three_maxima(s) == [2, -1, -1]
    s = list(z); s[2], s[8], s[9] = 11, 2, 1
    assert T.three_maxima(s) == [2, 8, -1]
    s = list(z); s[2], s[8], s[9] = 10, 2, 1
    assert T.three_maxima(s) == [2, 8, 9]


def test_only_stereo_gives_empty():
    """`!bOnlyStereo && CheckDistEpipolarLine(..)` (:417) accepts nothing."""
    kf1 = frame([(fam(i), 0, 0) for i in range(3)], {2: [0, 1, 2]})
    assert search(kf1, kf1) == ([0, 1, 2], 3)
    assert search(kf1, kf1, only_stereo=True) == ([-1, -1, -1], 0)


def test_planted_case_is_not_vacuous():
    """The generator the GPU tests use: matches, rotation resets, rows with
    several acceptances, and a real share of epipolar passes and failures."""
    kf1, kf2s, Fs = T.make_case(1, {3: 1, 7: 63, 8: 64, 20: 65, 21: 40}, [{3: 1, 7: 2, 8: 63, 20: 64, 21: 65}])
    m, nm, st = T.ref_search(kf1, kf2s[0], Fs[0])
    assert nm > 0 and (m == -2).any() and st["multi"] > 0
    assert 0.005 * st["evals"] < st["accepted"] < 0.5 * st["evals"]
    assert set(kf2s[0]["keys"]["octave"].tolist()) == set(range(8))


def test_epipolar_reproduces_reference_object_decisions():
    """tests/golden/epipolar_reference.npz: 413 (x1, y1, x2, y2, F12[9],
    sigma2) vectors and the decisions the reference's own compiled
    CheckDistEpipolarLine returned for them (random and near-threshold
    vectors, 40 on which the source-order form decides the other way, F12
    scaled until den is subnormal, den == 0, NaN in every F12 position, the
    double-compare case).  The restatement and the hand computation reproduce
    every one; the source-order form does not."""
    import os
    g = np.load(os.path.join(T.ROOT, "tests", "golden", "epipolar_reference.npz"))
    V, dec = g["vectors"], g["decision"].astype(bool)
    assert V.shape == (413, 14) and dec.shape == (413,) and 0 < dec.sum() < len(dec)
    mine = np.array([T.epipolar(v[0], v[1], v[2], v[3], v[4:13], v[13]) for v in V])
    assert np.array_equal(mine, dec), np.flatnonzero(mine != dec).tolist()
    written = np.array([T.epipolar(v[0], v[1], v[2], v[3], v[4:13], v[13], written=True) for v in V])
    assert (written != dec).sum() >= 30
    finite = np.isfinite(V).all(axis=1)
    assert (~finite).sum() == 9 and not dec[~finite].any()
    hand = np.array([hand_epipolar(v[0], v[1], v[2], v[3], v[4:13], v[13]) for v in V[finite]])
    assert np.array_equal(hand, dec[finite])
