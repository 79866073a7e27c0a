#!/usr/bin/env python3
"""Do two builds of the CPU kernel emulator give the same bits for the particle operations?

    python tools/particles_walk_parity.py OLD/librf_emu.so NEW/librf_emu.so

Runs emu_particles_paint (A, dropped), emu_particles_gather (G, dropped; `first`, then an add onto it) and emu_particles_tile_stats of
both libraries over every displacement set of tests/cic_oracle.displacement_sets plus one with a NaN and an inf planted, the shapes
(4,6,8), (16,16,16), (30,14,22), (16,32,64), both real types, form 1 and form 2 with the bricks (8,8,64; halo 2) and (2,2,4; halo 1), and
1, 3 and 16 host threads, and compares the sha256 of every output.  Prints the number of digests compared; exit status 1 on a difference."""
import ctypes
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import cic_oracle  # noqa: E402

SPACING = 2.5
SHAPES = [(4, 6, 8), (16, 16, 16), (30, 14, 22), (16, 32, 64)]
BRICKS = [((8, 8, 64), 2), ((2, 2, 4), 1)]
THREADS = [1, 3, 16]
_dp = ctypes.POINTER(ctypes.c_double)
_up = ctypes.POINTER(ctypes.c_ulonglong)


def load(path):
    lib = ctypes.CDLL(os.path.abspath(path))
    lib.emu_particles_paint.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3 + [_dp] + [ctypes.c_int] * 6 + [_up, _up]
    lib.emu_particles_tile_stats.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3 + [_dp] + [ctypes.c_int] * 4 + [_up]
    lib.emu_particles_gather.argtypes = ([ctypes.c_int] * 4 + [ctypes.c_void_p] * 3 + [_dp] + [ctypes.c_void_p] * 2 + [ctypes.c_double]
                                         + [ctypes.c_int] * 7 + [_up])
    return lib


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def cases():
    for shape in SHAPES:
        sets = cic_oracle.displacement_sets(shape, SPACING)
        bad = sets["rms3"].copy()
        bad[0][tuple(n // 2 for n in shape)] = np.nan
        bad[2][(0, 0, 0)] = np.inf
        sets["nonfinite"] = bad
        for name, s3 in sets.items():
            for dtype in (np.float32, np.float64):
                yield shape, name, dtype, [np.ascontiguousarray(s.astype(dtype)) for s in s3]


def digests(lib):
    out = {}
    inv_h = (ctypes.c_double * 3)(*([1.0 / SPACING] * 3))
    for shape, name, dtype, s3 in cases():
        f64 = int(dtype == np.float64)
        ptrs = [s.ctypes.data for s in s3]
        rng = np.random.RandomState(5)
        W = rng.normal(size=shape).astype(dtype)
        W2 = rng.normal(size=shape).astype(dtype)
        key = (shape, name, np.dtype(dtype).name)
        for brick, halo in BRICKS:
            st = np.zeros(4, np.uint64)
            assert lib.emu_particles_tile_stats(f64, *shape, *ptrs, inv_h, *brick, halo, st.ctypes.data_as(_up)) == 0
            out[key + ("stats", brick)] = sha(st)
        for form, brick, halo in [(1, (1, 1, 1), 1)] + [(2, b, h) for b, h in BRICKS]:
            for nth in THREADS:
                A = np.empty(shape, np.uint64)
                d = ctypes.c_ulonglong(99)
                assert lib.emu_particles_paint(f64, *shape, *ptrs, inv_h, form, *brick, halo, nth, A.ctypes.data_as(_up), ctypes.byref(d)) == 0
                out[key + ("paint", form, brick, nth)] = sha(A, np.uint64(d.value))
                G = np.full(shape, 7, dtype)
                for step, (field, coeff, first) in enumerate([(W, 1.0, 1), (W2, -0.75, 0)]):
                    d = ctypes.c_ulonglong(99)
                    assert lib.emu_particles_gather(f64, *shape, *ptrs, inv_h, field.ctypes.data, G.ctypes.data, coeff, first, form, *brick, halo, nth,
                                                    ctypes.byref(d)) == 0
                    out[key + ("gather", form, brick, nth, step)] = sha(G, np.uint64(d.value))
    return out


def main():
    old, new = digests(load(sys.argv[1])), digests(load(sys.argv[2]))
    assert old.keys() == new.keys()
    differ = [k for k in old if old[k] != new[k]]
    for k in differ[:20]:
        print("DIFFERENT", k)
    print("%d digests compared, %d equal, %d different" % (len(old), len(old) - len(differ), len(differ)))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
