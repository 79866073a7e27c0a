"""A call made of timed calls in the interval recorder (randomfield_amd/csrc/rf_timing.h span_begin / span_end / span_abandon, what makes
rf_elapsed_ms cover the whole of rf_particles_paint_interlaced) on the CPU: tests/timing_span_test.cpp walks a span over detailed and
plain calls with a fake runtime whose events carry a counter; built with AddressSanitizer + UBSan as a program of its own and run
here, as tests/test_timing.py runs tests/timing_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_timing_span_under_sanitizers(tmp_path):
    exe = str(tmp_path / "timing_span_test")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "timing_span_test.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert build.returncode == 0, build.stdout.decode(errors="replace")[-4000:]
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-4000:]
    assert "all checks passed" in out and "FAILED" not in out and "runtime error" not in out and "Sanitizer" not in out, out[-4000:]
