"""Host ASan + UBSan runs of the library's host code (SURVEY §5 sanitizer
build): `make sanitize` compiles geometry.cpp and every API translation unit
with -fsanitize=address,undefined on the host side only (-Xarch_host; no GPU
sanitizer) and keeps the objects in build_asan/; each row of PROGRAMS is a
stand-alone program of tests/cpp/ linked over them and run on the CPU (no GPU,
the devices are hidden).  Leak checking is off (the HIP runtime keeps its
allocations until exit)."""
import pytest

import native

# (program, its summary line on a clean run)
PROGRAMS = [
    # geometry planning over a size/parameter sweep plus malformed-argument
    # calls of every entry point
    ("sanitize_main", ", 0 failures"),
    # the drop-in calls' typed arena (csrc/call_arena.h) over two host buffers
    ("arena_main", ", 0 failures"),
    # the handles' resource owners (csrc/owned.h) over malloc'd blocks
    ("owned_main", ", 0 failures"),
    # the device-side projection: PredictScale threshold builder, argument checks
    ("projbuild_main", "projbuild_main: 0 failures"),
    # the keyframe projection: argument checks of orbm_keyframe_project and the
    # orbm_kf_plan_* entry points
    ("kfbuild_main", "kfbuild_main: 0 failures"),
    # the pose optimisation: argument checks of orbm_pose_optimization and the
    # orbm_pose_plan_* entry points
    ("poseopt_main", "poseopt_main: 0 failures"),
    # the initializer RANSAC: every argument check of orbm_initializer_ransac
    ("initransac_main", "initransac_main: 0 failures"),
    # the initializer reconstruction: every argument check of
    # orbm_initializer_reconstruct
    ("initrecon_main", "initrecon_main: 0 failures"),
]


@pytest.mark.parametrize("program,summary", PROGRAMS, ids=[p for p, _ in PROGRAMS])
def test_host_code_clean_under_asan_ubsan(program, summary):
    r = native.run_sanitized(program)
    assert summary in r.stdout
