"""The owning types behind the plan's buffers, events and streams (randomfield_amd/csrc/rf_owned.h) on the CPU: tests/owned_test.cpp
instantiates them with a fake runtime that counts calls and fails on request, is built with AddressSanitizer + UBSan as a program of
its own and run here.  The failure paths it walks (a failed allocation leaves an empty, retryable buffer; the second of a pair failing
leaves the first intact) are reached in the product only when the device is out of memory, so this is their only test."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owned_types_under_sanitizers(tmp_path):
    exe = str(tmp_path / "owned_test")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "owned_test.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert build.returncode == 0, build.stdout.decode(errors="replace")[-4000:]
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-4000:]
    assert "all checks passed" in out and "FAILED" not in out and "runtime error" not in out and "Sanitizer" not in out, out[-4000:]
