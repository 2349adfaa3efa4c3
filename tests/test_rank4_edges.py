"""k_distinctive and k_undistort (csrc/kernels_misc.hip): planted edge cases.

MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:222-271): group
sizes at the 64-lane chunk boundaries, medians of 0 and 256 (both ends of the
kernel's binary search), ties whose first minimum sits in an earlier chunk
than an equal later one, empty groups first, last and adjacent.
Frame::UndistortKeyPoints (src/Frame.cc:384-414): 4, 5, 8, 12 and 14
coefficients, keypoints outside the image, at the principal point and at the
corners, sizes around the 256-thread block, the k1 == 0 copy, in place.

Each has a numpy reference written here (float64, unpackbits); the CPU part
proves it equal to the oracle and that every planted case is what it claims,
the GPU part is bit-exact against both.
"""
import ctypes
import functools

import numpy as np
import pytest

EUROC_K = np.array([[458.654, 0, 367.215], [0, 457.296, 248.375], [0, 0, 1]], np.float32)
EUROC_D = np.array([-0.28340811, 0.07395907, 0.00019359, 1.76187114e-05], np.float32)
TUM1_K = np.array([[517.306408, 0, 318.643040], [0, 516.469215, 255.313989], [0, 0, 1]], np.float32)
TUM1_D = np.array([0.262383, -0.953104, -0.005358, 0.002628, 1.163314], np.float32)

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"),
                           ("response", "<f4"), ("octave", "<i4"), ("class_id", "<i4")])


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# --------------------------------------------------------------------------- distinctive
def np_medians(g):
    """row i: the N/2-th smallest of its N Hamming distances, d_ii = 0 included"""
    bits = np.unpackbits(np.asarray(g, np.uint8).reshape(-1, 32), axis=1)
    ham = (bits[:, None, :] != bits[None, :, :]).sum(2)
    return np.sort(ham, axis=1)[:, len(bits) // 2]


def np_distinctive(g):
    return int(np.argmin(np_medians(g))) if len(g) else -1  # argmin: the first minimum


def _near(rng, centre, n, frac):
    """n copies of centre, each bit flipped with probability frac"""
    flips = np.packbits(rng.uniform(size=(n, 256)) < frac, axis=1)
    return centre[None] ^ flips


SWEEP_N = [1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 200]


@functools.lru_cache(maxsize=None)
def _sweep_groups():
    rng = np.random.default_rng(41)
    return [_near(rng, rng.integers(0, 256, 32, dtype=np.uint8), n, 0.05) for n in SWEEP_N]


def _spread(rng, centre_rows, n=130):
    """n rows 40 % of the bits away from a centre (about 102 from it, about
    123 from each other), the rows of centre_rows the centre itself: those
    have the smallest median"""
    c = rng.integers(0, 256, 32, dtype=np.uint8)
    g = _near(rng, c, n, 0.4)
    g[list(centre_rows)] = c
    return g


@functools.lru_cache(maxsize=None)
def _planted_groups():
    """-> {name: (group, expected row)}"""
    rng = np.random.default_rng(42)
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    return {
        "identical": (np.repeat(a[None], 70, 0), 0),
        "complement": (np.stack([a, ~a]), 0),
        "two-complements": (np.stack([a, ~a, ~a]), 1),
        "last-row": (_spread(rng, [129]), 129),
        "tie-3-70": (_spread(rng, [3, 70]), 3),
        "tie-70-128": (_spread(rng, [70, 128]), 70),
    }


def test_distinctive_numpy_reference_is_the_oracle(oracle):
    for g in _sweep_groups() + [g for g, _ in _planted_groups().values()]:
        assert np_distinctive(g) == oracle.distinctive_descriptor(g), len(g)
    e = np.zeros((0, 32), np.uint8)
    assert np_distinctive(e) == oracle.distinctive_descriptor(e) == -1


def test_distinctive_planted_groups_are_what_they_claim(oracle):
    p = _planted_groups()
    for name, (g, want) in p.items():
        assert np_distinctive(g) == want == oracle.distinctive_descriptor(g), name
    assert np_medians(p["identical"][0]).tolist() == [0] * 70
    assert np_medians(p["complement"][0]).tolist() == [256, 256]  # the binary search's upper end
    assert np_medians(p["two-complements"][0]).tolist() == [256, 0, 0]
    med = np_medians(p["last-row"][0])
    assert (med == med.min()).sum() == 1 and med.argmin() == 129  # third 64-lane chunk, alone
    med = np_medians(p["tie-3-70"][0])
    assert np.flatnonzero(med == med.min()).tolist() == [3, 70]   # first and second chunk
    med = np_medians(p["tie-70-128"][0])
    assert np.flatnonzero(med == med.min()).tolist() == [70, 128]  # second and third chunk


@functools.lru_cache(maxsize=None)
def _group_lists():
    """group counts 1, 3, 4, 5 (the kernel takes four map points per block)
    and 1001, empty groups first, last and adjacent"""
    rng = np.random.default_rng(43)
    e = np.zeros((0, 32), np.uint8)
    sweep = _sweep_groups()
    planted = [g for g, _ in _planted_groups().values()]

    def small():
        n = int(rng.integers(0, 9))
        return _near(rng, rng.integers(0, 256, 32, dtype=np.uint8), n, 0.05)

    many = [e, e] + [small() for _ in range(996)] + [e, e, e]
    many[500] = many[501] = e
    return [[sweep[4]], [e], [e, sweep[5], e], [e, e, sweep[6], planted[3]],
            [sweep[0], e, e, sweep[3], e], sweep + planted, many]


def test_distinctive_group_lists_cpu(oracle):
    lists = _group_lists()
    assert [len(l) for l in lists] == [1, 1, 3, 4, 5, len(SWEEP_N) + 6, 1001]
    assert max(len(g) for l in lists for g in l) <= 200
    for l in lists:
        assert [np_distinctive(g) for g in l] == [oracle.distinctive_descriptor(g) for g in l]


@pytest.mark.gpu
def test_distinctive_edges_gpu(gpu, oracle):
    for l in _group_lists():
        best = gpu.compute_distinctive_descriptors(l)
        want = np.array([np_distinctive(g) for g in l], np.int32)
        assert np.array_equal(best, want)
        assert np.array_equal(best, np.array([oracle.distinctive_descriptor(g) for g in l], np.int32))
    want = [w for _, w in _planted_groups().values()]
    assert gpu.compute_distinctive_descriptors([g for g, _ in _planted_groups().values()]).tolist() == want


@pytest.mark.gpu
def test_distinctive_group_too_large_is_an_argument_error(gpu):
    """more than 2^20 rows in a group: refused from `off` alone, before any read of desc"""
    for off in ([0, (1 << 20) + 1], [0, 5, 5 + (1 << 20) + 1], [0, 5, 3]):
        off = np.array(off, np.int32)
        desc = np.zeros((1, 32), np.uint8)
        best = np.full(len(off) - 1, 77, np.int32)
        rc = gpu.lib().orbm_compute_distinctive_descriptors(_ptr(desc), _ptr(off), len(off) - 1, 0,
                                                            _ptr(best))
        assert rc == gpu.ERR_ARG
        assert best.tolist() == [77] * (len(off) - 1)


# --------------------------------------------------------------------------- undistort
def np_undistort(kps, K, dist):
    """oo_undistort_keypoints operation by operation, in numpy float64"""
    out = kps.copy()
    D = np.asarray(dist, np.float32).reshape(-1)
    if len(D) == 0 or D[0] == 0:
        return out
    k = np.zeros(14, np.float64)
    k[:len(D)] = D.astype(np.float64)
    K = np.asarray(K, np.float32).reshape(3, 3)
    fx, fy, cx, cy = (np.float64(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    ifx, ify = 1. / fx, 1. / fy
    x = (kps["x"].astype(np.float64) - cx) * ifx
    y = (kps["y"].astype(np.float64) - cy) * ify
    x0, y0 = x, y
    for _ in range(5):
        r2 = x * x + y * y
        icdist = (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2) / (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2)
        dx = 2 * k[2] * x * y + k[3] * (r2 + 2 * x * x) + k[8] * r2 + k[9] * r2 * r2
        dy = k[2] * (r2 + 2 * y * y) + 2 * k[3] * x * y + k[10] * r2 + k[11] * r2 * r2
        x = (x0 - dx) * icdist
        y = (y0 - dy) * icdist
    xx = fx * x + 0. * y + cx
    yy = 0. * x + fy * y + cy
    ww = 1. / (0. * x + 0. * y + 1.)
    out["x"] = (xx * ww).astype(np.float32)
    out["y"] = (yy * ww).astype(np.float32)
    return out


D8 = np.concatenate([TUM1_D, np.array([0.01, 0.02, -0.01], np.float32)])
D12 = np.concatenate([D8, np.array([1e-3, -2e-3, 5e-4, 1e-4], np.float32)])
D14 = np.concatenate([D12, np.zeros(2, np.float32)])
COEFFS = {"euroc4": (EUROC_K, EUROC_D, 752, 480), "tum5": (TUM1_K, TUM1_D, 640, 480),
          "k8": (TUM1_K, D8, 640, 480), "s12": (TUM1_K, D12, 640, 480),
          "zero-tilt14": (TUM1_K, D14, 640, 480)}
UNDIST_N = [1, 255, 256, 257, 1000]


SPECIAL = 7  # _keypoints(SPECIAL, ...): the planted points alone, a call of their own


def _keypoints(n, K, w, h, seed=50):
    """exactly n keypoints up to 200 px outside the image, every other field
    random; from n = 7 on the last seven are three at the principal point and
    the four image corners (the last row of the last block is a planted one)"""
    rng = np.random.default_rng(seed + n)
    kp = np.zeros(n, KEYPOINT_DTYPE)
    kp["x"] = rng.uniform(-200, w + 200, n)
    kp["y"] = rng.uniform(-200, h + 200, n)
    if n >= SPECIAL:
        kp["x"][n - 7:n - 4], kp["y"][n - 7:n - 4] = K[0, 2], K[1, 2]
        kp["x"][n - 4:] = [0, w - 1, 0, w - 1]
        kp["y"][n - 4:] = [0, 0, h - 1, h - 1]
    kp["size"] = rng.uniform(10, 100, n)
    kp["angle"] = rng.uniform(0, 360, n)
    kp["response"] = rng.uniform(0, 255, n)
    kp["octave"] = rng.integers(0, 8, n)
    kp["class_id"] = rng.integers(-1, 1 << 30, n)
    return kp


def test_undistort_keypoint_counts():
    """the kernel sees exactly the listed sizes: one row, one below, at and
    one above its 256-thread block, and several blocks with a tail"""
    for n in UNDIST_N + [SPECIAL]:
        kp = _keypoints(n, TUM1_K, 640, 480)
        assert len(kp) == n
        if n >= SPECIAL:
            assert kp["x"][n - 7:n - 4].tolist() == [TUM1_K[0, 2]] * 3
            assert (kp["x"][-1], kp["y"][-1]) == (639, 479) and (kp["x"][-4], kp["y"][-4]) == (0, 0)
    assert UNDIST_N == [1, 255, 256, 257, 1000]


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("name", list(COEFFS))
def test_undistort_numpy_reference_is_the_oracle(oracle, name):
    K, D, w, h = COEFFS[name]
    for n in UNDIST_N + [SPECIAL]:
        kp = _keypoints(n, K, w, h)
        r = oracle.undistort_keypoints(kp, K, D)
        assert np.isfinite(r["x"]).all() and np.isfinite(r["y"]).all()
        assert np.array_equal(_bytes(r), _bytes(np_undistort(kp, K, D)))
        for f in ("size", "angle", "response", "octave", "class_id"):
            assert np.array_equal(_bytes(r[f]), _bytes(kp[f]))
        assert not np.array_equal(r["x"], kp["x"])
        if name == "zero-tilt14":
            assert np.array_equal(_bytes(r), _bytes(oracle.undistort_keypoints(kp, K, D12)))
    # every further coefficient set changes the result
    kp = _keypoints(1000, TUM1_K, 640, 480)
    res = [oracle.undistort_keypoints(kp, TUM1_K, D) for D in (TUM1_D, D8, D12)]
    assert not np.array_equal(res[0]["x"], res[1]["x"]) and not np.array_equal(res[1]["x"], res[2]["x"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(COEFFS))
def test_undistort_edges_gpu(gpu, oracle, name):
    K, D, w, h = COEFFS[name]
    for n in UNDIST_N + [SPECIAL]:
        kp = _keypoints(n, K, w, h)
        assert len(kp) == n
        g = gpu.undistort_keypoints(kp, K, D)
        assert np.array_equal(_bytes(g), _bytes(oracle.undistort_keypoints(kp, K, D)))
        assert np.array_equal(_bytes(g), _bytes(np_undistort(kp, K, D)))
        if name == "zero-tilt14":
            assert np.array_equal(_bytes(g), _bytes(gpu.undistort_keypoints(kp, K, D12)))


@pytest.mark.parametrize("k1", [0.0, -0.0])
def test_undistort_k1_zero_copies_cpu(oracle, k1):
    kp = _keypoints(300, TUM1_K, 640, 480)
    D = D12.copy()
    D[0] = k1
    assert np.array_equal(_bytes(oracle.undistort_keypoints(kp, TUM1_K, D)), _bytes(kp))
    assert np.array_equal(_bytes(np_undistort(kp, TUM1_K, D)), _bytes(kp))


@pytest.mark.gpu
@pytest.mark.parametrize("k1", [0.0, -0.0])
def test_undistort_k1_zero_copies_gpu(gpu, k1):
    kp = _keypoints(300, TUM1_K, 640, 480)
    D = D12.copy()
    D[0] = k1
    assert np.signbit(D[0]) == np.signbit(np.float32(k1))
    assert np.array_equal(_bytes(gpu.undistort_keypoints(kp, TUM1_K, D)), _bytes(kp))


@pytest.mark.parametrize("tilt", [(0.01, 0.0), (0.0, -0.02), (np.nan, 0.0)])
def test_undistort_tilt_is_refused_by_the_oracle_too(oracle, tilt):
    kp = _keypoints(300, TUM1_K, 640, 480)
    D = D14.copy()
    D[12:] = tilt
    with pytest.raises(oracle.OracleError) as e:
        oracle.undistort_keypoints(kp, TUM1_K, D)
    assert e.value.code == oracle.OO_ERR_UNSUPPORTED
    if tilt[1] == 0.0:
        with pytest.raises(oracle.OracleError):
            oracle.undistort_keypoints(kp, TUM1_K, D[:13])
    D[0] = 0  # Frame::UndistortKeyPoints copies before OpenCV is reached
    assert np.array_equal(_bytes(oracle.undistort_keypoints(kp, TUM1_K, D)), _bytes(kp))


def _raw_undistort(gpu, kp, out, K, D):
    K9 = np.ascontiguousarray(K, np.float32).reshape(9)
    D = np.ascontiguousarray(D, np.float32)
    return gpu.lib().orbx_undistort_keypoints(_ptr(kp), len(kp), _ptr(K9), _ptr(D), len(D), 0,
                                              _ptr(out))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["euroc4", "s12"])
def test_undistort_in_place_gpu(gpu, oracle, name):
    K, D, w, h = COEFFS[name]
    kp = _keypoints(1000, K, w, h)
    want = gpu.undistort_keypoints(kp, K, D)
    assert np.array_equal(_bytes(want), _bytes(oracle.undistort_keypoints(kp, K, D)))
    buf = kp.copy()
    assert _raw_undistort(gpu, buf, buf, K, D) == gpu.OK
    assert np.array_equal(_bytes(buf), _bytes(want))
    D0 = np.array(D)
    D0[0] = 0  # the copy rule in place
    buf = kp.copy()
    assert _raw_undistort(gpu, buf, buf, K, D0) == gpu.OK
    assert np.array_equal(_bytes(buf), _bytes(kp))


@pytest.mark.gpu
@pytest.mark.parametrize("tilt", [(0.01, 0.0), (0.0, -0.02), (0.01, 0.02), (np.nan, 0.0)])
def test_undistort_tilt_is_unsupported_gpu(gpu, oracle, tilt):
    """OpenCV applies the inverse tilt matrix when tauX or tauY is non-zero;
    the kernel has no tilt model, so such a call is refused instead of
    answered without the tilt -- and leaves the next call intact"""
    kp = _keypoints(300, TUM1_K, 640, 480)
    D = D14.copy()
    D[12:] = tilt
    out = np.zeros_like(kp)
    assert _raw_undistort(gpu, kp, out, TUM1_K, D) == gpu.ERR_UNSUPPORTED
    assert not _bytes(out).any()
    with pytest.raises(gpu.OrbxError) as e:
        gpu.undistort_keypoints(kp, TUM1_K, D)
    assert e.value.code == gpu.ERR_UNSUPPORTED
    if tilt[1] == 0.0:  # 13 coefficients: tauX alone
        assert _raw_undistort(gpu, kp, out, TUM1_K, D[:13]) == gpu.ERR_UNSUPPORTED
    g = gpu.undistort_keypoints(kp, TUM1_K, D14)
    assert np.array_equal(_bytes(g), _bytes(oracle.undistort_keypoints(kp, TUM1_K, D14)))
    # Frame::UndistortKeyPoints copies on k1 == 0 before OpenCV is reached
    D[0] = 0
    assert np.array_equal(_bytes(gpu.undistort_keypoints(kp, TUM1_K, D)), _bytes(kp))
