"""The planted projection-matcher cases on the CPU (tests/projection_util.py):
the path model (a restatement of k_grid_build / k_proj_cand / k_proj_resolve)
equals the oracle (a restatement of the reference loop) in every match entry
and in nmatches, every case reaches the path it names (asserted on the model's
stats), and the cases with an answer that can be worked out by hand assert it
literally.  tests/test_projection_gpu_edges.py runs the same cases on the GPU."""
import os
import re

import numpy as np
import pytest

import projection_util as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb-slam-system_amd", "csrc")


def test_constants_mirror_the_kernel(oracle):
    hdr = open(os.path.join(CSRC, "proj_internal.h")).read()
    val = lambda name: int(re.search(r"#define %s (\d+)" % name, hdr).group(1))
    assert (val("PJ_T"), val("PJ_MAXN"), val("PG_COLS"), val("PG_ROWS")) == (P.PJ_T, P.PJ_MAXN, P.COLS, P.ROWS)
    assert re.search(r"#define PG_CELLS \(PG_COLS \* PG_ROWS\)", hdr)
    # one definition: neither translation unit re-declares them
    kern = open(os.path.join(CSRC, "kernels_proj.hip")).read()
    api = open(os.path.join(CSRC, "api_proj.hip")).read()
    for txt in (kern, api):
        assert '#include "proj_internal.h"' in txt
        assert not re.search(r"#define (PJ_T|PJ_MAXN|PG_COLS|PG_ROWS|PG_CELLS)\b", txt)
        assert not re.search(r"struct (ProjFrame|ProjProblem) *\{", txt)
    # k_grid_build: one block of GRID_BLOCK threads, strided by the same number
    assert int(re.search(r"__launch_bounds__\((\d+)\) void k_grid_build", kern).group(1)) == P.GRID_BLOCK
    assert re.search(r"k_grid_build, dim3\(\(unsigned\)nprob\), dim3\(%d\)" % P.GRID_BLOCK, api)
    assert set(re.findall(r"\+= (\d+)\)", kern[kern.index("k_grid_build"):kern.index("area_cells")])) == {str(P.GRID_BLOCK)}
    # the sort key holds a cell and an index, the candidate key a distance and a rank, in 16 bits each
    assert P.COLS * P.ROWS <= 1 << 16 and P.PJ_MAXN <= 1 << 16 and P.PJ_T < 64
    assert P.PROJ_QUERY_DTYPE == oracle.PROJ_QUERY_DTYPE and P.KEYPOINT_DTYPE == oracle.KEYPOINT_DTYPE


@pytest.mark.parametrize("geom", sorted(P.GEOMETRIES))
def test_grid_steps_are_found_not_assumed(geom):
    """step_to_product brackets each half-cell threshold by one float32 step,
    and the model's cells agree with oracle-independent double arithmetic"""
    g = P.geometry(geom)
    for axis, last in ((0, P.COLS), (1, P.ROWS)):
        for t in (-0.5, 0.5, last - 1.5, last - 0.5):
            below, at = P.step_to_product(g, axis, t)
            assert np.nextafter(below, np.float32(np.inf)) == at
            assert P.grid_product(g, below, axis) < np.float32(t) <= P.grid_product(g, at, axis)
            # halves round away from zero: the cell changes across t = k + 0.5 > 0
            # and, for t = -0.5, only where the product leaves -0.5 itself
            lo, hi = int(P.c_roundf(P.grid_product(g, below, axis))), int(P.c_roundf(P.grid_product(g, at, axis)))
            if t > 0:
                assert (lo, hi) == (int(t - 0.5), int(t + 0.5))
            else:
                assert lo == -1 and hi in (-1, 0)


def test_rotation_bins_in_float32():
    bins = P.expected_rot_bins()
    assert bins == [P.rot_bin(qa, ka) for qa, ka in P.ROT_EDGES]
    # rot = 0, 15 (0.5 -> 1), 45 (1.5 -> 2), 345 (11.5 -> 12), and the wraps: -15 -> 345, -315 -> 45, -1e-6 -> 360.0f
    assert [bins[i] for i in (0, 1, 2, 4, 6, 7, 8)] == [0, 1, 2, 12, 12, 2, 12]
    assert np.float32(np.float32(0.0) - np.float32(1e-6)) + np.float32(360.0) == np.float32(360.0)
    assert all(0 <= b <= 12 for b in bins)


def test_three_maxima_cutoffs():
    h = np.zeros(30, int)
    h[[0, 4, 9]] = 11, 1, 1
    assert P.three_maxima(h) == (0, -1, -1)  # 1 < 0.1f * 11
    h[0] = 10
    assert P.three_maxima(h) == (0, 4, 9)    # 1 < 0.1f * 10 = 1.0f is false
    assert P.three_maxima(np.zeros(30, int)) == (-1, -1, -1)


@pytest.mark.parametrize("name", P.CASE_NAMES)
def test_model_equals_oracle(oracle, name):
    c = P.case(name)
    m, nm, st = P.assert_reaches_its_path(name)
    rm, rn = oracle.search_by_projection(*c.args)
    assert rn == int((rm >= 0).sum())
    assert nm == rn, (nm, rn)
    assert np.array_equal(m, rm), np.nonzero(m != rm)[0][:10]
    for feat, qi in c.expect.items():
        assert rm[feat] == qi, (feat, int(rm[feat]), qi)


def test_mode1_ignores_check_ori_and_th_dist(oracle):
    a, b = P.case("rot-h11-m1-ori"), P.case("rot-h11-m1-noori")
    assert a.check_ori and not b.check_ori and np.array_equal(a.q, b.q) and np.array_equal(a.qd, b.qd)
    ra, rb = oracle.search_by_projection(*a.args), oracle.search_by_projection(*b.args)
    assert ra[1] == rb[1] == 13 and np.array_equal(ra[0], rb[0])
    a, b = P.case("thr-m1-ratio0.5-th50"), P.case("thr-m1-ratio0.5-th200")
    ra, rb = oracle.search_by_projection(*a.args), oracle.search_by_projection(*b.args)
    assert ra[1] == rb[1] and np.array_equal(ra[0], rb[0])


def test_every_path_is_reached_somewhere():
    """over all cases: each early return, complete and incomplete lists, all
    three rescan outcomes, an equality in the ratio test, features outside"""
    tot = {}
    for name in P.CASE_NAMES:
        st = P.model_of(name)[2]
        for k in P.EARLY + ("empty", "list", "rescan_match", "rescan_reject", "rescan_none", "exact_T",
                            "exact_T1", "ratio_equal", "outside"):
            tot[k] = tot.get(k, 0) + st[k]
    assert all(v > 0 for v in tot.values()), tot
