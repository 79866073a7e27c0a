#!/usr/bin/env python3
"""Does a build of the CPU emulator (randomfield_amd/csrc/emu/librf_emu.so) compute what another build computes?

    python tools/emu_parity.py [path/to/librf_emu.so] [--whole-columns] > digests.txt

Prints one line per result -- `shape dtype call [switches]: sha256` of the field and its two moments -- for emu_realise,
emu_realise_fast, emu_c2r, emu_r2c, emu_c2c, emu_c2r_lognormal and emu_row_c2r_xgather over tiny grids chosen so that every branch of
the rules the emulator follows is reached (rf_select.h: whole columns and Col2 halves at ny = 1024 / 2048, split and unsplit generation
passes, tile pairs on and off, the side buffer and the owning lane's repair, the blocked intermediate on and off).  Run it once per
build (the default is the emulator of this tree) and diff the two outputs.  --whole-columns calls emu_set_col_halves(0) first where the
build has it: in-place passes then keep whole columns, as builds before that switch did in emu_c2r / emu_c2c / emu_r2c.
This is a comparison tool, not a test of values."""
import ctypes
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import emu_util  # noqa: E402
from oracle import cpu_ref  # noqa: E402
from randomfield_amd import powertools  # noqa: E402

SPACING = 2.5
# fast generation: unsplit, split with the owning lane's repair, split with the side buffer, tile pairs (one and two pairs per ky row), Col2
# halves unsplit and split, the float64 halves form, y passes of 1024 / 2048
FAST = [(8, 8, 16), (64, 32, 128), (64, 64, 64), (512, 8, 16), (512, 8, 32), (1024, 8, 16), (1024, 8, 32), (1024, 8, 64), (2048, 8, 16),
        (2048, 8, 32), (8, 1024, 32), (8, 2048, 16)]
EXACT = [(8, 8, 16), (64, 32, 128), (64, 64, 64), (512, 8, 32), (8, 1024, 32), (8, 2048, 16), (1024, 8, 16)]
C2C = [(8, 8, 8), (16, 8, 32), (1024, 8, 8), (8, 1024, 8), (2048, 8, 8), (8, 2048, 8)]
XGATHER = [(512, 16, 4, 8, 8), (256, 32, 2, 16, 16), (1024, 8, 4, 8, 4)]
LINES = []


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def record(key, fn):
    try:
        out = fn()
        val = sha(*[np.asarray(o) for o in out]) if isinstance(out, (tuple, list)) else sha(out)
    except AssertionError as exc:
        val = "REFUSED " + " ".join(str(exc).split())
    LINES.append("%s: %s" % (key, val))
    print(LINES[-1], flush=True)


class switches:
    def __init__(self, L, xposed, pairs):
        self.L, self.want = L, (xposed, pairs)

    def __enter__(self):
        self.old = (self.L.emu_set_xposed(self.want[0]), self.L.emu_set_pairs(self.want[1]))

    def __exit__(self, *exc):
        self.L.emu_set_xposed(self.old[0])
        self.L.emu_set_pairs(self.old[1])
        return False


def lognormal(L, ks):
    nx, ny, nzh = ks.shape
    nz = 2 * (nzh - 1)
    growth = np.exp(-0.5 * np.arange(nz) / nz)
    dens = 0.5 + np.arange(nz) / nz
    out = np.zeros((nx, ny, nz), np.float32 if ks.dtype == np.complex64 else np.float64)
    sig, s1, s2 = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    dp = ctypes.POINTER(ctypes.c_double)
    rc = L.emu_c2r_lognormal(int(ks.dtype == np.complex128), nx, ny, nz, ks.ctypes.data_as(ctypes.c_void_p), growth.ctypes.data_as(dp),
                             dens.ctypes.data_as(dp), out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(sig), ctypes.byref(s1), ctypes.byref(s2))
    assert rc == 0, rc
    return out, sig.value, s1.value, s2.value


def xgather(L, M, nx, ny, tc, rb, dtype):
    rng = np.random.RandomState(M + nx)
    X = (rng.normal(size=(nx // rb, M // tc, ny, rb, tc)) + 1j * rng.normal(size=(nx // rb, M // tc, ny, rb, tc))).astype(dtype)
    out = np.zeros((nx, ny, 2 * M), np.float32 if dtype == np.complex64 else np.float64)
    s1, s2 = ctypes.c_double(), ctypes.c_double()
    rc = L.emu_row_c2r_xgather(int(dtype == np.complex128), M, nx, ny, tc, rb, X.ctypes.data_as(ctypes.c_void_p),
                               out.ctypes.data_as(ctypes.c_void_p), ctypes.c_double(0.5), ctypes.byref(s1), ctypes.byref(s2))
    assert rc == 0, rc
    return out, s1.value, s2.value


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if args:
        emu_util.SO = os.path.abspath(args[0])
        emu_util.build = lambda force=False: emu_util.SO
    L = emu_util.lib()
    if "--whole-columns" in sys.argv[1:] and hasattr(L, "emu_set_col_halves"):
        L.emu_set_col_halves(0)
    power = powertools.load_default_power()
    k, Pk = power["k"], power["Pk"]
    for dtype in (np.complex64, np.complex128):
        rt = np.float32 if dtype == np.complex64 else np.float64
        name = np.dtype(dtype).name
        for shape in FAST:
            if dtype == np.complex128 and shape[0] == 2048:
                continue                                  # (no fast generation kernel: float64, nx = 2048)
            xt, st = cpu_ref.sigma_table(k, Pk, *shape, SPACING)
            for xposed, pairs in ((0, 1), (0, 0), (1, 1)):
                with switches(L, xposed, pairs):
                    record("%dx%dx%d %s emu_realise_fast xposed=%d pairs=%d" % (shape + (name, xposed, pairs)),
                           lambda: emu_util.realise_fast(*shape, SPACING, xt, st, seed=7, dtype=rt))
        for shape in EXACT:
            nx, ny, nz = shape
            xt, st = cpu_ref.sigma_table(k, Pk, nx, ny, nz, SPACING)
            rng = np.random.RandomState(nx + ny + nz)
            ks = (rng.normal(size=(nx, ny, nz // 2 + 1)) + 1j * rng.normal(size=(nx, ny, nz // 2 + 1))).astype(dtype)
            cpu_ref.symmetrize_packed(ks)
            field = rng.normal(size=shape).astype(rt)
            for xposed in (0, 1):
                with switches(L, xposed, 1):
                    tag = "%dx%dx%d %s " % (shape + (name,))
                    record(tag + "emu_realise xposed=%d" % xposed, lambda: emu_util.realise(nx, ny, nz, SPACING, xt, st, seed=3, dtype=dtype))
                    record(tag + "emu_c2r xposed=%d" % xposed, lambda: emu_util.c2r(ks))
            record(tag + "emu_r2c", lambda: emu_util.r2c(field))
            record(tag + "emu_c2r_lognormal", lambda: lognormal(L, ks))
        for shape in C2C:
            rng = np.random.RandomState(sum(shape))
            data = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(dtype)
            for inverse in (False, True):
                record("%dx%dx%d %s emu_c2c inverse=%d" % (shape + (name, inverse)), lambda: emu_util.c2c(data, inverse))
        for M, nx, ny, tc, rb in XGATHER:
            record("M=%d nx=%d ny=%d tc=%d rb=%d %s emu_row_c2r_xgather" % (M, nx, ny, tc, rb, name), lambda: xgather(L, M, nx, ny, tc, rb, dtype))
    print("# %d lines, sha256 of all: %s" % (len(LINES), hashlib.sha256("\n".join(LINES).encode()).hexdigest()), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
