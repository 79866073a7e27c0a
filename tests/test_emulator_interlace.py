"""The interlaced paint on the CPU emulator (csrc/emu emu_particles_paint_shifted: the rf_core.h functions cic_particle_half /
tsc_particle_half that the HALF instantiations of rf_k_particles.hip's paint operations call, under the same two walks on real host
threads; emu_kspace_interlace: interlace_mul / interlace_cell, the cell function of interlace_kernel, over the array) and the ABI
surface.

Oracle: tests/interlace_oracle.py.  Integer weights and float64 steps rounded one by one: every comparison is ==."""
import ctypes
import os

import numpy as np
import pytest

import emu_util
import interlace_oracle as orc
import tsc_oracle as torc

SPACING = 0.5
INV_H = [1.0 / SPACING] * 3
SHAPES = [(4, 6, 8), (10, 12, 70), (16, 16, 16)]          # as tests/test_emulator_tsc.py
REALS = [np.float32, np.float64]
_c_dp = ctypes.POINTER(ctypes.c_double)
_c_up = ctypes.POINTER(ctypes.c_ulonglong)
RUNS = [(1, 1, None, 0), (1, 5, None, 0), (2, 1, (8, 8, 64), 2), (2, 7, (8, 8, 64), 2), (2, 3, (2, 2, 4), 1), (2, 4, (4, 4, 8), 2)]


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else np.dtype(v).name


@pytest.fixture(scope="module")
def lib():
    lib = emu_util.lib()
    lib.emu_particles_paint_shifted.argtypes = [ctypes.c_int] * 6 + [ctypes.c_void_p] * 3 + [_c_dp] + [ctypes.c_int] * 6 + [_c_up, _c_up]
    lib.emu_particles_paint_shifted.restype = ctypes.c_int
    lib.emu_kspace_interlace.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 5
    lib.emu_kspace_interlace.restype = ctypes.c_int
    return lib


def emu_paint(lib, s3, form, brick=None, halo=2, nth=1, scheme=2, half=1, rc_want=0):
    s3 = [np.ascontiguousarray(s) for s in s3]
    nx, ny, nz = s3[0].shape
    brick = brick or (8, 8, 64)
    A = np.full((nx, ny, nz), 7, np.uint64)
    dropped = ctypes.c_ulonglong(99)
    h = np.asarray(INV_H, np.float64)
    rc = lib.emu_particles_paint_shifted(int(s3[0].dtype == np.float64), scheme, half, nx, ny, nz, *[s.ctypes.data for s in s3], h.ctypes.data_as(_c_dp),
                                         form, brick[0], brick[1], brick[2], max(halo, 1), nth, A.ctypes.data_as(_c_up), ctypes.byref(dropped))
    assert rc == rc_want
    return A, int(dropped.value)


def emu_combine(lib, S, K, tables):
    K = np.ascontiguousarray(K).copy()
    S = np.ascontiguousarray(S)
    nx, ny, nzh = K.shape
    tabs = [None if t is None else np.ascontiguousarray(t, np.complex128) for t in (tables or [None] * 3)]
    rc = lib.emu_kspace_interlace(int(K.dtype == np.complex128), nx, ny, 2 * (nzh - 1), S.ctypes.data, K.ctypes.data,
                                  *[None if t is None else t.ctypes.data for t in tabs])
    assert rc == 0
    return K


def sets_of(shape, rt):
    sets = dict(torc.displacement_sets(shape, SPACING))
    sets.update(torc.extra_sets(shape, SPACING))
    bad = sets["rms0.6"].copy()
    bad[1][1, 2, 3] = np.nan
    bad[2][tuple(n - 1 for n in shape)] = np.inf
    sets["non-finite"] = bad
    return {name: s.astype(rt) for name, s in sets.items()}


@pytest.mark.parametrize("scheme", [2, 3], ids=["cic", "tsc"])
@pytest.mark.parametrize("rt", REALS, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_shifted_paint_both_walks_equal_the_oracle(lib, shape, rt, scheme):
    n = int(np.prod(shape))
    for name, s in sets_of(shape, rt).items():
        want, wdrop = orc.paint(s, INV_H, scheme)
        assert wdrop == (2 if name == "non-finite" else 0) and orc.total(want) == (n - wdrop) * orc.ONE
        for form, nth, brick, halo in RUNS:
            A, dropped = emu_paint(lib, s, form, brick, halo, nth, scheme)
            assert dropped == wdrop and np.array_equal(A, want), (name, form, nth, brick)
        if name in ("rms3", "huge"):
            plain, pdrop = emu_paint(lib, s, 2, nth=3, scheme=scheme, half=0)
            assert pdrop == wdrop and np.array_equal(plain, orc.unshifted(s, INV_H, scheme)[0]) and not np.array_equal(plain, want)


def test_half_cell_argument(lib):
    s = sets_of((4, 6, 8), np.float32)["rms3"]
    for bad in (2, -1):
        emu_paint(lib, s, 1, half=bad, rc_want=-1)
    emu_paint(lib, s, 1, scheme=4, rc_want=-1)


@pytest.mark.parametrize("ctype", [np.complex64, np.complex128], ids=_ids)
@pytest.mark.parametrize("shape", [(4, 6, 8), (16, 16, 16), (10, 12, 70)], ids=_ids)
def test_combine_equals_the_oracle(lib, shape, ctype):
    rng = np.random.RandomState(sum(shape))
    kshape = (shape[0], shape[1], shape[2] // 2 + 1)
    S = (rng.normal(size=kshape) + 1j * rng.normal(size=kshape)).astype(ctype)       # no Hermitian symmetry: every cell on its own
    K = (rng.normal(size=kshape) + 1j * rng.normal(size=kshape)).astype(ctype)
    random_tabs = [rng.normal(size=n) + 1j * rng.normal(size=n) for n in kshape]
    for tabs in (None, orc.phases(shape), random_tabs, [None, random_tabs[1], None]):
        out = emu_combine(lib, S, K, tabs)
        assert out.dtype == ctype and np.array_equal(out, orc.combine(S, K, tabs))
    assert not np.array_equal(emu_combine(lib, S, K, None), emu_combine(lib, S, K, orc.phases(shape)))


def test_abi_reports_the_interlaced_paint():
    from randomfield_amd import _hip
    assert (_hip.ABI_MAJOR, _hip.ABI_MINOR) == (5, 5) and _hip.abi_version() == (5, 5)
    assert _hip.FEATURES["particles_interlace"] == 1 << 21
    lib = _hip.load()
    assert lib.rf_abi_features() & (1 << 21)
    assert "particles_interlace" in _hip.abi_features()
    for name in ("rf_particles_paint_shifted", "rf_kspace_stash", "rf_kspace_interlace", "rf_particles_paint_interlaced"):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    header = open(os.path.join(emu_util.ROOT, "include", "randomfield_hip.h")).read()
    assert "RF_FEATURE_PARTICLES_INTERLACE = 1 << 21" in header
    assert "int rf_particles_paint_shifted(rf_plan* plan, const double* inv_h, int scheme, int half_cell, unsigned long long* dropped);" in header
    assert "int rf_kspace_stash(rf_plan* plan);" in header
    assert "int rf_kspace_interlace(rf_plan* plan, const double* px, const double* py, const double* pz);" in header
    assert "#define RF_ABI_MAJOR 5" in header and "#define RF_ABI_MINOR 5" in header
