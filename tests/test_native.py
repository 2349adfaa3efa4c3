"""tests/native.py itself: the flags table covers the restatements under
tests/cpp/, and a source or a program is built once per process."""
import glob
import os

import native


def test_every_restatement_has_a_flags_row():
    refs = {os.path.basename(p) for p in glob.glob(os.path.join(native.CPP, "*_ref.c"))}
    assert refs and refs <= set(native.REF_FLAGS)
    for name in native.REF_FLAGS:
        assert os.path.isfile(os.path.join(native.CPP, name)), name


def test_ref_lib_is_built_once():
    lib = native.ref_lib("match_fold_hash.c")
    assert native.ref_lib("match_fold_hash.c") is lib
    assert lib.fold_rounds() > 0


def test_program_is_built_once():
    args = ("poseopt_compat_main.cpp", ("poseopt_ref.c",))
    exe = native.program(*args)
    stamp = os.stat(exe).st_mtime_ns
    assert native.program(*args) == exe and os.stat(exe).st_mtime_ns == stamp
    # linked with the object the loader's shared object is made of
    assert os.stat(native.ref_object("poseopt_ref.c")).st_mtime_ns <= stamp
