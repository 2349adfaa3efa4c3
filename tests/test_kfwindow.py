"""The CPU restatement of the search ORBmatcher::Fuse / SearchBySim3 share
(tests/cpp/kfwindow_ref.c) pinned on a hand-built keyframe with a known answer
per query, and against a grid-free numpy walk on random input.  No GPU."""
import numpy as np
import pytest

import kfwindow_util as K

INT_MAX = K.INT_MAX


def D(k):
    """a descriptor at Hamming distance k from the all-zero one"""
    d = np.zeros(32, np.uint8)
    for b in range(k):
        d[b >> 3] |= np.uint8(1 << (b & 7))
    return d


# index: (x, y, octave, distance to the zero descriptor).  640 x 480, 10 px
# cells: feature x lies in column round(x / 10)
FEATS = [
    (100.0, 100.0, 0, 10),   # 0
    (103.0, 100.0, 0, 5),    # 1  exactly 3 px from (100, 100)
    (207.5, 200.0, 0, 7),    # 2  column 21
    (1.0, 50.0, 0, 9),       # 3  left edge
    (634.0, 50.0, 0, 11),    # 4  column 63
    (646.0, 50.0, 0, 1),     # 5  column 65: outside the grid
    (300.0, 300.0, 1, 3),    # 6
    (301.0, 300.0, 0, 20),   # 7
    (406.0, 400.0, 0, 8),    # 8  column 41
    (404.0, 400.0, 0, 8),    # 9  column 40: visited before 8
    (320.0, 2.0, 2, 12),     # 10 top edge
    (320.0, 474.0, 2, 13),   # 11 bottom edge (row 47)
]


@pytest.fixture(scope="module")
def kf():
    keys = K.make_keys([f[0] for f in FEATS], [f[1] for f in FEATS], [f[2] for f in FEATS])
    return K.frame_dict(keys, np.array([D(f[3]) for f in FEATS]))


def _one(kf, x, y, r, level):
    q = np.zeros(1, K.KF_QUERY_DTYPE)
    q[0] = (x, y, r, level, 0)
    bi, bd, st = K.ref_search(kf, q, np.zeros((1, 32), np.uint8))
    return int(bi[0]), int(bd[0]), {k: int(v[0]) for k, v in st.items()}


def test_cells_are_filled_in_index_order(kf):
    c = K.ref_cells(kf)
    assert c[0].tolist() == [10, 10, 0] and c[1].tolist() == [10, 10, 1]
    assert c[2].tolist() == [21, 20, 0]
    assert c[5].tolist() == [-1, -1, -1]  # column 65
    assert c[8].tolist() == [41, 40, 0] and c[9].tolist() == [40, 40, 0]
    assert c[6].tolist() == [30, 30, 0] and c[7].tolist() == [30, 30, 1]


def test_feature_exactly_r_away_is_excluded(kf):
    bi, bd, st = _one(kf, 100.0, 100.0, 3.0, 0)
    assert (bi, bd) == (0, 10) and st["visited"] == 2 and st["boxed"] == 1
    # a hair wider and the closer descriptor is in
    assert _one(kf, 100.0, 100.0, 3.5, 0)[:2] == (1, 5)
    # strict on the y side too
    assert _one(kf, 100.0, 103.0, 3.0, 0)[:2] == (-1, INT_MAX)


def test_query_on_a_cell_edge(kf):
    # x - r = 210 and x + r = 216: floor(21.0..) = 21, ceil(21.6) = 22
    bi, bd, st = _one(kf, 213.0, 200.0, 3.0, 0)
    assert (bi, bd) == (-1, INT_MAX) and st["visited"] == 1 and st["boxed"] == 0
    # x - r = 207: column 20 upwards, feature 2 (column 21) 2.5 px away
    assert _one(kf, 210.0, 200.0, 3.0, 0)[:2] == (2, 7)
    # x + r = 200 exactly: ceil(20.0..) reaches column 21 only through rounding
    # up of 200 * 0.1f; feature 2 is 10.5 px away either way
    assert _one(kf, 197.0, 200.0, 3.0, 0)[:2] == (-1, INT_MAX)


def test_windows_that_leave_the_image(kf):
    # the four early returns: nothing is visited
    for x, y in ((-20.0, 50.0), (700.0, 50.0), (320.0, -20.0), (320.0, 520.0)):
        bi, bd, st = _one(kf, x, y, 3.0, 0)
        assert (bi, bd) == (-1, INT_MAX) and st["visited"] == 0
    # partly outside: the clamps
    assert _one(kf, -2.0, 50.0, 3.6, 1)[:2] == (3, 9)     # 3 px from feature 3
    assert _one(kf, -2.0, 50.0, 3.0, 0)[:2] == (-1, INT_MAX)
    assert _one(kf, 636.5, 50.0, 3.0, 0)[:2] == (4, 11)
    assert _one(kf, 320.0, -0.5, 3.0, 2)[:2] == (10, 12)
    assert _one(kf, 320.0, 476.5, 3.0, 2)[:2] == (11, 13)
    # far outside int's range: converts as the reference's x86 object does
    assert _one(kf, 1e30, 50.0, 3.0, 0)[:2] == (-1, INT_MAX)
    assert _one(kf, 100.0, 100.0, 1e30, 0)[:2] == (-1, INT_MAX)


def test_feature_outside_the_grid_is_never_found(kf):
    # feature 5 is 2 px away with the best descriptor, but in no cell
    bi, bd, st = _one(kf, 644.0, 50.0, 3.0, 0)
    assert (bi, bd) == (-1, INT_MAX) and st["boxed"] == 0
    assert _one(kf, 640.0, 50.0, 11.0, -1)[:2] == (4, 11)


def test_octave_gate(kf):
    assert _one(kf, 300.0, 300.0, 3.0, 0)[:2] == (7, 20)   # level 0: octave 0 only
    assert _one(kf, 300.0, 300.0, 3.0, 1)[:2] == (6, 3)    # octaves 0 and 1
    assert _one(kf, 300.0, 300.0, 3.0, 2)[:2] == (6, 3)    # octaves 1 and 2
    assert _one(kf, 300.0, 300.0, 3.0, -1)[:2] == (6, 3)   # no gate
    bi, bd, st = _one(kf, 300.0, 300.0, 3.0, -1)
    assert st["gated"] == 2
    # a window whose every feature fails the gate
    bi, bd, st = _one(kf, 300.0, 300.0, 3.0, 5)
    assert (bi, bd) == (-1, INT_MAX) and st["boxed"] == 2 and st["gated"] == 0


def test_tie_goes_to_the_first_visited_not_the_lowest_index(kf):
    bi, bd, st = _one(kf, 405.0, 400.0, 3.0, 0)
    assert (bi, bd) == (9, 8)
    assert st["at_best"] == 2 and st["lower_loser"] == 1
    # inside one cell the lower index is first
    d = K.frame_dict(K.make_keys([100.0, 101.0], [100.0, 100.0], [0, 0]), np.array([D(4), D(4)]))
    assert _one(d, 100.5, 100.0, 3.0, 0)[:2] == (0, 4)


def test_descriptor_pool_rows(kf):
    q = np.zeros(3, K.KF_QUERY_DTYPE)
    q[0] = (100.0, 100.0, 3.5, 0, 2)
    q[1] = (100.0, 100.0, 3.5, 0, 0)
    q[2] = (100.0, 100.0, 3.5, 0, 2)
    pool = np.array([D(0), D(200), D(10)])
    bi, bd, _ = K.ref_search(kf, q, pool)
    assert bi.tolist() == [0, 1, 0] and bd.tolist() == [0, 5, 0]


@pytest.mark.parametrize("seed", [1, 2])
def test_visiting_order_against_numpy(seed):
    rng = np.random.RandomState(seed)
    kf = K.make_frame(rng, 400)
    q, qd = K.make_queries(rng, kf, 500)
    bi, bd, st = K.ref_search(kf, q, qd)
    K.assert_not_vacuous(kf, bi, bd, st)
    wi, wd = K.brute_force(kf, q, qd)
    assert np.array_equal(bi, wi) and np.array_equal(bd, wd)


def test_empty_shapes():
    kf = K.frame_dict(np.zeros(0, K.KEYPOINT_DTYPE), np.zeros((0, 32), np.uint8))
    q = np.zeros(2, K.KF_QUERY_DTYPE)
    q["radius"] = 3.0
    bi, bd, _ = K.ref_search(kf, q, np.zeros((1, 32), np.uint8))
    assert bi.tolist() == [-1, -1] and bd.tolist() == [INT_MAX, INT_MAX]
    bi, bd, _ = K.ref_search(kf, q[:0], np.zeros((1, 32), np.uint8))
    assert len(bi) == 0 and len(bd) == 0
