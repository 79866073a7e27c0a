"""The kernel phase functions under AddressSanitizer + UBSan on the CPU (GPU sanitizers are not available
on this pool): every supported axis length of the strided passes, the c2r and r2c row passes and both
generation flavours, and the generic mixed-radix blocks, run in a separate process against an instrumented build of the emulator, whose LDS /
global "memory" are exactly-sized heap arrays -- any out-of-bounds index aborts the run."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "randomfield_amd", "csrc")
SO = os.path.join(CSRC, "emu", "librf_emu_asan.so")

DRIVER = r'''
import ctypes, sys, os
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, os.path.join(%(root)r, "tests"))
import emu_util
emu_util.SO = %(so)r
emu_util._lib = ctypes.CDLL(%(so)r)
from oracle import cpu_ref
pw = np.load(os.path.join(%(root)r, "tests", "golden", "default_power.npz"))
rng = np.random.RandomState(0)
for N in (8, 16, 32, 64, 128, 256, 512, 1024, 2048):
    for dt in (np.complex64, np.complex128):
        a = (rng.normal(size=(N, 64)) + 1j * rng.normal(size=(N, 64))).astype(dt)
        assert emu_util.col_fft(a, N, +1, 64, 64, 0, 64) == 0
for M in (8, 16, 32, 64, 128, 256, 512, 1024):
    for dt in (np.float32, np.float64):
        f = rng.normal(size=(8, 8, 2 * M)).astype(dt)
        spec = emu_util.r2c(f)
        back, s1, s2 = emu_util.c2r(spec)
        assert np.max(np.abs(back - f)) < 1e-3
for shape in ((8, 8, 16), (16, 32, 64), (64, 16, 32)):
    nx, ny, nz = shape
    xt, st = cpu_ref.sigma_table(pw["k"], pw["Pk"], nx, ny, nz, 2.5)
    noise = cpu_ref.reference_noise(1, nx * ny * (nz // 2 + 1))
    for dt in (np.complex64, np.complex128):
        emu_util.generate_kspace(nx, ny, nz, 2.5, xt, st, noise=noise, dtype=dt)
        emu_util.realise(nx, ny, nz, 2.5, xt, st, noise=noise, dtype=dt)
        emu_util.realise(nx, ny, nz, 2.5, xt, st, seed=3, dtype=dt)
    emu_util.realise_fast(nx, ny, nz, 2.5, xt, st, seed=3)
# the float32 generation pass of length 1024 on tile pairs (ColPair: parked registers, paired stores) and as two half transforms at 2048
for shape in ((1024, 8, 32), (2048, 8, 16)):
    nx, ny, nz = shape
    xt, st = cpu_ref.sigma_table(pw["k"], pw["Pk"], nx, ny, nz, 2.5)
    emu_util.realise_fast(nx, ny, nz, 2.5, xt, st, seed=5)
for shape in ((4, 6, 8), (40, 60, 80), (10, 14, 22), (2, 2, 2), (26, 34, 46)):        # the generic mixed-radix blocks
    for ct, rt in ((np.complex64, np.float32), (np.complex128, np.float64)):
        nx, ny, nz = shape
        ks = (rng.normal(size=(nx, ny, nz // 2 + 1)) + 1j * rng.normal(size=(nx, ny, nz // 2 + 1))).astype(ct)
        out, s1, s2 = emu_util.generic_c2r(ks)
        assert np.max(np.abs(out - np.fft.irfftn(ks.astype(np.complex128), s=shape, axes=(0, 1, 2)))) < 1e-3
        emu_util.generic_r2c(out)
        emu_util.generic_c2c(ks, True)
# the same blocks on host threads (the kernels' own thread walk, tile-wide LDS images sized to the byte as the launchers size them,
# real barriers): line counts that divide no tile, smooth and prime radices, and the four-step form with a lowered cap
for shape, cap in (((10, 14, 24), 0), ((14, 22, 28), 0), ((12, 10, 24), 8)):
    old = emu_util.lib().emu_set_generic_cap(cap)
    for nth, tile in ((16, 4), (32, 16)):
        for ct, rt in ((np.complex64, np.float32), (np.complex128, np.float64)):
            nx, ny, nz = shape
            ks = (rng.normal(size=(nx, ny, nz // 2 + 1)) + 1j * rng.normal(size=(nx, ny, nz // 2 + 1))).astype(ct)
            a = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(ct)
            with emu_util.generic_threads(nth, tile):
                out, s1, s2 = emu_util.generic_c2r(ks)
                emu_util.generic_r2c(out)
                emu_util.generic_c2c(a, True)
                emu_util.generic_c2c(a, False)
            assert np.max(np.abs(out - np.fft.irfftn(ks.astype(np.complex128), s=shape, axes=(0, 1, 2)))) < 1e-3
    emu_util.lib().emu_set_generic_cap(old)
print("SANITIZED-OK")
'''


def test_emulator_under_asan_ubsan():
    src = os.path.join(CSRC, "emu", "rf_emu.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-shared", "-fPIC", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", SO, src])
    asan = subprocess.check_output(["g++", "-print-file-name=libasan.so"]).decode().strip()
    env = dict(os.environ, LD_PRELOAD=asan, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    p = subprocess.run([sys.executable, "-c", DRIVER % dict(root=ROOT, so=SO)], env=env, capture_output=True,
                       text=True, timeout=900)
    assert p.returncode == 0 and "SANITIZED-OK" in p.stdout, (p.stdout[-2000:], p.stderr[-4000:])


TSAN_PROBE = r"""
#include <thread>
#include <pthread.h>
int main() {
  pthread_barrier_t b; pthread_barrier_init(&b, nullptr, 2);
  int x = 0;
  std::thread t([&] { x = 1; pthread_barrier_wait(&b); });
  pthread_barrier_wait(&b);
  t.join();
  return x == 1 ? 0 : 1;
}
"""

# a program of its own (ThreadSanitizer wants the whole process instrumented: no Python around it): the emulator's source plus a main()
# that runs a threaded generic c2r and checks it against the single-thread run
TSAN_MAIN = r"""
#include "%(src)s"
#include <complex>
int main() {
  const int nx = 10, ny = 14, nz = 24, nzh = nz / 2 + 1;
  std::vector<cplx<float>> K((size_t)nx * ny * nzh);
  unsigned s = 12345u;
  for (auto& v : K) { s = s * 1664525u + 1013904223u; v.x = (float)(s >> 8) / 16777216.0f - 0.5f; s = s * 1664525u + 1013904223u; v.y = (float)(s >> 8) / 16777216.0f - 0.5f; }
  std::vector<float> one((size_t)nx * ny * nz), many(one.size());
  double s1, s2;
  if (emu_generic_c2r(0, nx, ny, nz, K.data(), one.data(), &s1, &s2)) return 2;
  const int tiles[3] = {4, 8, 16};
  for (int t = 0; t < 3; ++t) {
    emu_set_generic_threads(16);
    emu_set_generic_tile(tiles[t]);
    if (emu_generic_c2r(0, nx, ny, nz, K.data(), many.data(), &s1, &s2)) return 3;
    emu_set_generic_threads(1);
    emu_set_generic_tile(3);
    if (memcmp(one.data(), many.data(), one.size() * sizeof(float))) return 4;
  }
  puts("TSAN-OK");
  return 0;
}
"""


def _tsan_works(tmp_path):
    """can this g++ build AND run a threaded program under -fsanitize=thread (the runtime refuses some kernels' address-space layouts)?"""
    src, exe = tmp_path / "probe.cpp", tmp_path / "probe"
    src.write_text(TSAN_PROBE)
    if subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", "-fsanitize=thread", "-o", str(exe), str(src)], capture_output=True).returncode:
        return False
    try:
        return subprocess.run([str(exe)], capture_output=True, timeout=120).returncode == 0
    except (OSError, subprocess.TimeoutExpired):
        return False


def test_threaded_generic_c2r_under_tsan(tmp_path):
    """One threaded generic c2r (16 host threads, tiles 4 / 8 / 16, grid (10, 14, 24)) under ThreadSanitizer: a barrier missing between
    two phases of a block function that touch the same LDS element is a data race it reports.  Skipped only where a probe shows that
    this g++ cannot build or run any threaded program with -fsanitize=thread."""
    if not _tsan_works(tmp_path):
        pytest.skip("g++ -fsanitize=thread does not build or run a threaded probe program here")
    src, exe = tmp_path / "tsan_main.cpp", tmp_path / "tsan_main"
    src.write_text(TSAN_MAIN % dict(src=os.path.join(CSRC, "emu", "rf_emu.cpp")))
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=thread", "-o", str(exe), str(src)])
    p = subprocess.run([str(exe)], env=dict(os.environ, TSAN_OPTIONS="halt_on_error=1"), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "TSAN-OK" in p.stdout, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
