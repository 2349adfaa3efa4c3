"""The reference-shaped C++ surface (cpp/orbslam2_compat.hpp: ORB_SLAM2::
ORBextractor / ORBmatcher / ORBVocabulary, DBoW2 vectors, Frame's stereo
search) compiled against liborbx.so and driven like the reference's call
sites; outputs checked against the oracle."""
import os
import subprocess

import numpy as np
import pytest

import native
from orbx import synth


def _build_stereo():
    return native.program("stereo_main.cpp")


def test_cpp_stereo_adapter_compiles():
    assert os.path.exists(_build_stereo())


@pytest.mark.gpu
def test_cpp_stereo_adapter_matches_oracle(gpu, oracle, tmp_path):
    exe = _build_stereo()
    W, H, nf, fx, bf = 1241, 376, 2000, 718.856, 386.1448
    L, R = synth.stereo_pair(W, H, 60)
    (tmp_path / "l.raw").write_bytes(L.tobytes())
    (tmp_path / "r.raw").write_bytes(R.tobytes())
    out = tmp_path / "out.bin"
    subprocess.check_call([exe, str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), str(W),
                           str(H), str(nf), repr(fx), repr(bf), str(out)])
    raw = out.read_bytes()
    nl, nr, n = np.frombuffer(raw[:12], np.int32).tolist()
    ur = np.frombuffer(raw[12:12 + 4 * nl], np.float32)
    dep = np.frombuffer(raw[12 + 4 * nl:12 + 8 * nl], np.float32)
    el, er = oracle.Extractor(nf, 1.2, 8, 20, 7), oracle.Extractor(nf, 1.2, 8, 20, 7)
    kl, dl = el.extract(L)
    kr, dr = er.extract(R)
    assert (nl, nr) == (len(kl), len(kr))
    t = el.tables()
    mb = np.float32(np.float32(bf) / np.float32(fx))
    ur0, dep0, n0 = oracle.compute_stereo_matches(kl, dl, kr, dr, t["scale"], t["inv_scale"],
                                                  [el.level(l) for l in range(8)],
                                                  [er.level(l) for l in range(8)], mb, np.float32(bf))
    assert n == n0
    assert np.array_equal(ur.view(np.uint32), ur0.view(np.uint32))
    assert np.array_equal(dep.view(np.uint32), dep0.view(np.uint32))


def _build_vocab():
    return native.program("vocab_main.cpp")


def test_cpp_vocab_adapter_compiles():
    assert os.path.exists(_build_vocab())


@pytest.mark.gpu
def test_cpp_vocab_adapter_matches_oracle(gpu, oracle, tmp_path):
    exe = _build_vocab()
    W, H = 1241, 376
    voc = synth.vocabulary(10, 5, seed=3)
    synth.write_vocabulary_text(tmp_path / "voc.txt", voc)
    a, b = synth.frame(W, H, 61), synth.frame(W, H, 62)
    (tmp_path / "a.raw").write_bytes(a.tobytes())
    (tmp_path / "b.raw").write_bytes(b.tobytes())
    out = tmp_path / "out.bin"
    subprocess.check_call([exe, str(tmp_path / "voc.txt"), str(tmp_path / "a.raw"),
                           str(tmp_path / "b.raw"), str(W), str(H), str(out)])
    raw = out.read_bytes()
    n1, nb, nf, nm = np.frombuffer(raw[:16], np.int32).tolist()
    off = 16
    bw = np.frombuffer(raw[off:off + 4 * nb], np.uint32); off += 4 * nb
    bv = np.frombuffer(raw[off:off + 8 * nb], np.float64); off += 8 * nb
    fn = np.frombuffer(raw[off:off + 4 * nf], np.uint32); off += 4 * nf
    fo = np.frombuffer(raw[off:off + 4 * (nf + 1)], np.uint32); off += 4 * (nf + 1)
    ff = np.frombuffer(raw[off:off + 4 * int(fo[-1])], np.uint32); off += 4 * int(fo[-1])
    m12 = np.frombuffer(raw[off:off + 4 * n1], np.int32)
    ex = oracle.Extractor(2000, 1.2, 8, 20, 7)
    k1, d1 = ex.extract(a)
    k2, d2 = ex.extract(b)
    ov = oracle.Vocabulary.load_text(tmp_path / "voc.txt")
    (rbw, rbv), rfv1 = ov.transform(d1, 4)
    _, rfv2 = ov.transform(d2, 4)
    assert np.array_equal(bw, rbw) and np.array_equal(bv.view(np.uint64), rbv.view(np.uint64))
    assert np.array_equal(fn, rfv1["node_id"]) and np.array_equal(fo, rfv1["off"])
    assert np.array_equal(ff, rfv1["feat"])
    kf1 = dict(desc=d1, angle=k1["angle"], valid=None, **rfv1)
    kf2 = dict(desc=d2, angle=k2["angle"], valid=None, **rfv2)
    rm, rnm = oracle.search_by_bow(kf1, kf2, 0.75, True)
    # vpMatches12 as pointers: matched entries name kf2's MapPoint, the rest
    # (never written, or reset by the rotation check) are null
    assert nm == rnm and np.array_equal(m12, np.where(rm >= 0, rm, -1))


def _build_compat():
    return native.program("compat_main.cpp", extra=("-pthread",))


def test_reference_shaped_call_sites_compile():
    """Frame::ExtractORB / Frame::Frame's stereo threads / LoopClosing's
    SearchByBoW / DescriptorDistance(cv::Mat, cv::Mat) written as in the
    reference compile against cpp/orbslam2_compat.hpp."""
    assert os.path.exists(_build_compat())


def _compat_featvec(n):
    nodes = [4 * j + 3 for j in range(5)]
    feat, off = [], [0]
    for j in range(5):
        feat.extend(i for i in range(n) if i % 5 == j)
        off.append(len(feat))
    return np.array(nodes, np.uint32), np.array(off, np.uint32), np.array(feat, np.uint32)


@pytest.mark.gpu
def test_reference_shaped_concurrent_call_sites(gpu, oracle, tmp_path):
    """Two ORB_SLAM2::ORBextractor instances on the two stereo threads of a
    Frame-shaped constructor, concurrently with SearchByBoW(KF, KF) on a third
    thread, 6 repetitions (each identical to the first, checked in C++), all
    bit-exact against the oracle."""
    exe = _build_compat()
    W, H, nf = 752, 480, 1200
    L, R = synth.stereo_pair(W, H, 70)
    c, d = synth.frame(W, H, 80, "pan"), synth.frame(W, H, 81, "pan")
    paths = []
    for name, im in (("l", L), ("r", R), ("c", c), ("d", d)):
        (tmp_path / (name + ".raw")).write_bytes(np.ascontiguousarray(im).tobytes())
        paths.append(str(tmp_path / (name + ".raw")))
    out = tmp_path / "out.bin"
    subprocess.check_call([exe] + paths + [str(W), str(H), str(nf), "6", str(out)], timeout=120)
    raw = out.read_bytes()
    nl, nr, n1, nm, dist = np.frombuffer(raw[:20], np.int32).tolist()
    off = 20
    kl = np.frombuffer(raw[off:off + 28 * nl], oracle.KEYPOINT_DTYPE); off += 28 * nl
    dl = np.frombuffer(raw[off:off + 32 * nl], np.uint8).reshape(nl, 32); off += 32 * nl
    kr = np.frombuffer(raw[off:off + 28 * nr], oracle.KEYPOINT_DTYPE); off += 28 * nr
    dr = np.frombuffer(raw[off:off + 32 * nr], np.uint8).reshape(nr, 32); off += 32 * nr
    m12 = np.frombuffer(raw[off:off + 4 * n1], np.int32); off += 4 * n1
    sc = np.frombuffer(raw[off:off + 32], np.float32); off += 32
    tw, th = np.frombuffer(raw[off:off + 8], np.int32).tolist(); off += 8
    top = np.frombuffer(raw[off:off + tw * th], np.uint8).reshape(th, tw)
    e = oracle.Extractor(nf, 1.2, 8, 20, 7)
    rkr, rdr = e.extract(R)
    rkl, rdl = e.extract(L)
    assert np.array_equal(top, e.level(7))  # mvImagePyramid after the left frame
    assert np.array_equal(kl.view(np.uint8), rkl.view(np.uint8)) and np.array_equal(dl, rdl)
    assert np.array_equal(kr.view(np.uint8), rkr.view(np.uint8)) and np.array_equal(dr, rdr)
    assert np.array_equal(sc, e.tables()["scale"])
    assert dist == oracle.descriptor_distance(rdl[0], rdr[0])
    kc, dc = e.extract(c)
    kd, dd = e.extract(d)

    def kf(k, dsc):
        n = len(k)
        ids, offs, feat = _compat_featvec(n)
        valid = np.array([(i % 7 != 3) and (i % 11 != 5) for i in range(n)], np.uint8)
        return dict(desc=dsc, angle=k["angle"], valid=valid, node_id=ids, off=offs, feat=feat)
    rm, rnm = oracle.search_by_bow(kf(kc, dc), kf(kd, dd), 0.75, True)
    assert nm == rnm and nm > 0 and np.array_equal(m12, rm)
    # SearchByBoW(KF, Frame): stub by default (checked in C++), then
    # bow_kf_frame=full against the oracle's upstream restatement
    off += tw * th  # past mvImagePyramid[7]
    nkf, nfd = np.frombuffer(raw[off:off + 8], np.int32).tolist(); off += 8
    mf = np.frombuffer(raw[off:off + 4 * nfd], np.int32)
    fr = dict(kf(kd, dd), valid=None)
    rmf, rnkf = oracle.search_by_bow_kf_frame(kf(kc, dc), fr, 0.7, True)
    assert nfd == len(kd) and nkf == rnkf and nkf > 0 and np.array_equal(mf, rmf)
