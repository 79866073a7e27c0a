"""The host side of the MT19937 replay (randomfield_amd/csrc/rf_replay.h) on the CPU: tests/replay_test.cpp carries, as literal copies,
the geometry, the two jump-tree loops, the digit hop, the rank split, the table widening and the step comparisons that rf_capi_mt.hip held
inside its HIP entry points, and compares the header with them over the ranges its sections list; built with AddressSanitizer + UBSan as a
program of its own and run here.  Its second mode prints the header's geometry and rank split for one grid: they are held against
tests/replay_matrix.py geom() and RANK_SPLITS, the figures the GPU suite's case table is chosen by."""
import os
import re
import subprocess

import pytest

import replay_matrix as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("replay") / "replay_test")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "replay_test.cpp"), "-o", path],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert build.returncode == 0, build.stdout.decode(errors="replace")[-4000:]
    return path


def _run(exe, *args):
    run = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120, env=ENV)
    out = run.stdout.decode(errors="replace")
    assert run.returncode == 0, out[-4000:]
    assert "runtime error" not in out and "Sanitizer" not in out, out[-4000:]
    return out


def test_replay_plan_under_sanitizers(exe):
    out = _run(exe)
    assert "all checks passed" in out and "FAILED" not in out, out[-4000:]
    # geometry: (70 000 + 2 grids) x 6 bps x 2 radices x 2 modes, 6 checks each without a tree, 8 with one (a table one row short is refused);
    # tree: 74 097 segment counts x 5 + 2 per count <= 5000 (9097 of them) + 2; hops: one check per refused (first, stages), 3 per accepted;
    # split: 54 cases + 2 refused, per rank; step: 7 + 7^2 + ... + 7^5 sequences, 4 checks per call, + 8 mode pairs; widening: 22 tables + 2
    sections = dict(re.findall(r"^(\w+): (\d+) checks$", out, re.M))
    assert {k: int(v) for k, v in sections.items()} == {"geometry": 12777904, "tree": 388681, "hops": 567991, "split": 6658, "step": 379100,
                                                        "widening": 62}, out[-4000:]
    total = re.search(r"^(\d+) checks, 0 failed$", out, re.M)
    assert total and int(total.group(1)) == 14120396, out[-4000:]


@pytest.mark.parametrize("case", rm.CASES, ids=[rm.case_id(c) for c in rm.CASES])
def test_geometry_equals_the_case_table(exe, case):
    """replay_geom (what the entry points size the replay by) against replay_matrix.geom (what the GPU suite's cases are chosen by)"""
    shape = case[0]
    g = rm.geom(shape, case[1])
    got = tuple(int(v) for v in _run(exe, "geom", shape[0], shape[1], shape[2], g.bps).split())
    assert got == (g.nseg, g.stages, g.last_nb, g.cap)


@pytest.mark.parametrize("split", rm.RANK_SPLITS, ids=["%dx%dx%d-%dranks" % (s[0] + (s[2],)) for s in rm.RANK_SPLITS])
def test_rank_split_equals_the_case_table(exe, split):
    shape, bps, nranks, seed, first = split
    nseg = int(_run(exe, "geom", shape[0], shape[1], shape[2], bps).split()[0])
    assert nseg == rm.geom(shape, bps).nseg
    assert tuple(int(v) for v in _run(exe, "split", nseg, nranks).split()) == tuple(first)
