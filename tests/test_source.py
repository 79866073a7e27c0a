"""Which generator fills an x pass (randomfield_amd/csrc/rf_source.h) on the CPU: tests/source_test.cpp carries, as literal copies, the
expressions the C-API layer worked that out with before there was one decision, walks every combination of the plan's facts and the call's
ask and compares on every combination the entry points can reach; built with AddressSanitizer + UBSan as a program of its own and run here."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_generation_source_under_sanitizers(tmp_path):
    exe = str(tmp_path / "source_test")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "source_test.cpp"), "-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert build.returncode == 0, build.stdout.decode(errors="replace")[-4000:]
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=60,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1"))
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-4000:]
    assert "all checks passed" in out and "FAILED" not in out and "runtime error" not in out and "Sanitizer" not in out, out[-4000:]
    # 2 dtypes x 2 x 2 flags x 5 kinds x 3 deviate states x 2 (k-space given) x 3 modes x 3 asks = 2160 combinations.  Reachable plans: a tiled
    # kind has 2 x 2 x 2 x 3 - 4 (no float32 pairs on complex128) = 20, a generic one 2 x 2 x 2 = 8 (no fast records, no pairs), c2c none that
    # realises.  Calls per plan: a given k-space array 1 (never on a replicated plan); a plain generation 1 / 2 / 3 with no / float32 / float64
    # deviates (NATIVE; + RESIDENT; + EXTERNAL), which is 8 + 8 + 24 = 40 per tiled kind and 4 + 12 = 16 generic; the potential stored, and
    # emitted, 6 each on single and exchanging plans (NATIVE on the 5 plans with the fast path, RESIDENT on the one that holds float32 pairs).
    # single 20 + 40 + 6 + 6 = 72, exchange 72, replicated 40, generic 8 + 16 = 24: 208
    counts = re.search(r"combinations: (\d+) reachable, (\d+) excluded", out)
    assert counts, out[-4000:]
    assert (int(counts.group(1)), int(counts.group(2))) == (208, 1952), out[-4000:]
