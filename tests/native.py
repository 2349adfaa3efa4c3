"""The one place that compiles and loads native test code: the CPU restatements
under tests/cpp/ (each compiled once per process, one way, whether it is loaded
with ctypes or linked into a stand-alone program), the stand-alone programs
over liborbx.so, and the host ASan/UBSan runs of the Makefile's build_asan/
programs.  Also the few definitions every *_util module shared by copy.  No
GPU, no orbx import."""
import atexit
import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "orb-slam-system_amd")
CPP = os.path.join(ROOT, "tests", "cpp")
INCLUDE = os.path.join(ROOT, "include")

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"),
                           ("octave", "<i4"), ("class_id", "<i4")])

# A restatement is what every bit-exact GPU test is judged against: each source
# is compiled with REF_BASE_FLAGS plus its row here, nowhere else.
REF_BASE_FLAGS = ("-O2", "-ffp-contract=off", "-Wall")
REF_FLAGS = {
    "bowdb_ref.c": (),
    "initransac_ref.c": ("-fno-strict-aliasing",),
    "initrecon_ref.c": ("-fno-strict-aliasing",),
    "initsearch_ref.c": (),
    "kfbuild_ref.c": (),
    "kfwindow_ref.c": (),
    "match_fold_hash.c": (),  # integer only
    "poseopt_ref.c": (),
    "projbuild_ref.c": (),
    "triangulation_ref.c": ("-mfma",),
}


@functools.lru_cache(maxsize=None)
def _workdir():
    """this process's build directory, outside the tree, removed at exit"""
    d = tempfile.mkdtemp(prefix="orbx_native_")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    return d


def _stem(name):
    return os.path.splitext(name)[0]


@functools.lru_cache(maxsize=None)
def ref_object(name):
    """the object file of tests/cpp/<name>, a source of REF_FLAGS"""
    obj = os.path.join(_workdir(), _stem(name) + ".o")
    subprocess.check_call(["gcc", *REF_BASE_FLAGS, *REF_FLAGS[name], "-fPIC", "-c", os.path.join(CPP, name),
                           "-o", obj])
    return obj


@functools.lru_cache(maxsize=None)
def ref_lib(name):
    """ref_object(name) as a shared object, loaded"""
    so = os.path.join(_workdir(), "lib" + _stem(name) + ".so")
    subprocess.check_call(["gcc", "-shared", "-o", so, ref_object(name), "-lm"])
    return ctypes.CDLL(so)


@functools.lru_cache(maxsize=None)
def program(main_cpp, refs=(), extra=()):
    """the path of the stand-alone program tests/cpp/<main_cpp> over liborbx.so,
    linked with the restatements `refs` (names of REF_FLAGS) and built with the
    further flags `extra`; tuples, so that a second call finds the first"""
    exe = os.path.join(_workdir(), _stem(main_cpp))
    objs = [ref_object(r) for r in refs]
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", *extra, "-I", os.path.join(PKG, "cpp"), "-I", CPP,
                           os.path.join(CPP, main_cpp), *objs, "-o", exe, "-L", PKG, "-lorbx", "-lm",
                           "-Wl,-rpath," + PKG])
    return exe


def run_sanitized(target):
    """make build_asan/<target> and run it on the CPU (the devices are hidden;
    leak checking is off: the HIP runtime keeps its allocations until exit).
    Returns the completed process once it ended clean, for the caller's own
    check of the summary line."""
    subprocess.check_call(["make", "-s", "-j8", "-C", PKG, "build_asan/" + target], timeout=900)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([os.path.join(PKG, "build_asan", target)], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    return r


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def same_bits(a, b):
    """bit-for-bit equality of two float32 arrays, NaNs of any payload equal"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])
