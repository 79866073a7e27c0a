"""Which pipeline a plan runs (randomfield_amd/csrc/rf_route.h) on the CPU: tests/route_test.cpp carries, as literal copies, the
expressions the C-API layer worked that out with before there was a route, walks every combination of the plan's seven facts and compares
on every combination the creators and setters allow; built with AddressSanitizer + UBSan as a program of its own and run here."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plan_route_under_sanitizers(tmp_path):
    exe = str(tmp_path / "route_test")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "route_test.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert build.returncode == 0, build.stdout.decode(errors="replace")[-4000:]
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-4000:]
    assert "all checks passed" in out and "FAILED" not in out and "runtime error" not in out and "Sanitizer" not in out, out[-4000:]
    # 3 rank counts x 3 chunk counts x 2^5 flags = 288 combinations.  Reachable: 2 unpacked (generic or not), 1 generic, 12 tiled plans on one
    # rank (force_slab x direct x 3 chunk counts), 24 on 2 or 4 ranks (replicate x direct x 3 chunk counts each)
    counts = re.search(r"combinations: (\d+) reachable, (\d+) excluded", out)
    assert counts, out[-4000:]
    assert (int(counts.group(1)), int(counts.group(2))) == (39, 249), out[-4000:]
