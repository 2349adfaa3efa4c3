"""Host ASan + UBSan run of the initializer reconstruction's host code: the
stand-alone tests/cpp/initrecon_main.cpp (every argument check of
orbm_initializer_reconstruct; no GPU, the devices are hidden) over the sanitizer
build of the library's objects that `make sanitize` keeps in build_asan/."""
import os
import subprocess

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orb-slam-system_amd")


def test_initializer_reconstruct_host_code_clean_under_asan_ubsan():
    subprocess.check_call(["make", "-s", "-j8", "-C", PKG, "build_asan/initrecon_main"], timeout=900)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1", HIP_VISIBLE_DEVICES="")
    r = subprocess.run([os.path.join(PKG, "build_asan", "initrecon_main")], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "initrecon_main: 0 failures" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
