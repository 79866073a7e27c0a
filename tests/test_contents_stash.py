"""The stashed half spectrum in the record of what a plan's device buffers hold (randomfield_amd/csrc/rf_contents.h stash() /
stash_ready()) on the CPU: tests/contents_stash_test.cpp walks every state the other transitions can reach and checks that the stash
is set by its one transition alone, survives every other one and changes nothing else; built with AddressSanitizer + UBSan as a
program of its own and run here, as tests/test_contents.py runs tests/contents_test.cpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stash_in_plan_contents_under_sanitizers(tmp_path):
    exe = str(tmp_path / "contents_stash_test")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "contents_stash_test.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert build.returncode == 0, build.stdout.decode(errors="replace")[-4000:]
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-4000:]
    assert "all checks passed" in out and "FAILED" not in out and "runtime error" not in out and "Sanitizer" not in out, out[-4000:]
