"""Host ASan + UBSan run of the Sim3 solver's host code (csrc/api_sim3.hip):
tests/cpp/sim3_main.cpp, a stand-alone program linked over the Makefile's
build_asan/ objects, makes every argument check of orbm_sim3_solve with the
devices hidden.  No GPU; nothing is loaded into Python."""
import native


def test_sim3_host_code_clean_under_asan_ubsan():
    r = native.run_sanitized("sim3_main")
    assert "sim3_main: 0 failures" in r.stdout
