"""The choice of tiled kernel as pure host functions (randomfield_amd/csrc/rf_select.h) on the CPU: tests/select_test.cpp walks
fastgen_variant over its whole input space (both dtypes x every served length x emit x noise64 x noise32 x pot x slab: 576 cases) against
literal rule tables, col_halves / halves_fit at the two served lengths and their neighbours, and fastgen_sequence at the smallest grids where
each of its branches exists (every tile exactly once, the kz = 0 tiles by a repairing launch).  Built with AddressSanitizer + UBSan as a
program of its own and run here.  The GPU launchers only turn what these functions return into kernel instantiations."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_selection_under_sanitizers(tmp_path):
    exe = str(tmp_path / "select_test")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "select_test.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert build.returncode == 0, build.stdout.decode(errors="replace")[-4000:]
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-4000:]
    assert "all checks passed" in out and "FAILED" not in out and "runtime error" not in out and "Sanitizer" not in out, out[-4000:]
