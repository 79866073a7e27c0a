"""Generic grids with the generation inside the first FFT pass (csrc/rf_generic.h generic_c2r_from_seq, GenericGenSource), on the CPU
emulator: the fused sequence must give the field and the moments of generation + generic_c2r_seq bit for bit -- the same gen_cell
values in the same LDS positions through the same stages -- for every thread walk the kernels and the emulator have.  Plus the ABI
surface of the option (flag 64, feature bit 13), which needs no GPU either."""
import ctypes
import os
import re

import numpy as np
import pytest

import emu_util
from conftest import golden
from oracle import cpu_ref

SPACING = 2.5
SHAPES = [(4, 6, 8), (40, 60, 80), (10, 14, 22),
          (26, 34, 46),                 # 2 13, 2 17, 23: axes that are not smooth (two LDS buffers, natural order)
          (30, 14, 22)]                 # Lx = 14 * 12 = 168 lines: a ragged last block at tile 16
WALKS = [(1, 3), (16, 4), (16, 8), (16, 16)]        # (host threads, lines per block): the walk by index, then the kernels' own walk

_c_dp = ctypes.POINTER(ctypes.c_double)
_GEN = [ctypes.c_int] * 4 + [_c_dp] * 5 + [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, _c_dp]


@pytest.fixture(scope="module")
def lib():
    lib = emu_util.lib()
    lib.emu_generic_realise.argtypes = _GEN + [ctypes.c_void_p, _c_dp, _c_dp]
    lib.emu_generic_realise.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module")
def dpower():
    d = golden("default_power.npz")
    return d["k"], d["Pk"]


def fused(lib, shape, xt, st, seed, noise, dtype):
    nx, ny, nz = shape
    args, keep = emu_util._gen_args(nx, ny, nz, SPACING, xt, st, seed, noise)
    out = np.empty(shape, np.float32 if dtype == np.complex64 else np.float64)
    s1, s2 = ctypes.c_double(), ctypes.c_double()
    rc = lib.emu_generic_realise(int(dtype == np.complex128), nx, ny, nz, *args, out.ctypes.data_as(ctypes.c_void_p),
                                 ctypes.byref(s1), ctypes.byref(s2))
    assert rc == 0, rc
    return out, s1.value, s2.value


def unfused(shape, xt, st, seed, noise, dtype):
    nx, ny, nz = shape
    ks = emu_util.generate_kspace(nx, ny, nz, SPACING, xt, st, seed=seed, noise=noise, dtype=dtype)
    return emu_util.generic_c2r(ks)


@pytest.fixture(scope="module")
def cases(dpower):
    """Per shape: the power table and one set of reference deviates, made once."""
    k, Pk = dpower
    out = {}
    for shape in SHAPES:
        nx, ny, nz = shape
        xt, st = cpu_ref.sigma_table(k, Pk, nx, ny, nz, SPACING)
        out[shape] = (xt, st, cpu_ref.reference_noise(7, nx * ny * (nz // 2 + 1)))
    return out


@pytest.mark.parametrize("external", [False, True], ids=["native", "external"])
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128], ids=["c64", "c128"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_fused_equals_generate_then_c2r_bit_for_bit(lib, cases, shape, dtype, external):
    xt, st, noise = cases[shape]
    noise = noise if external else None
    seed = 0 if external else 4242
    for nth, tile in WALKS:
        with emu_util.generic_threads(nth, tile):
            want, w1, w2 = unfused(shape, xt, st, seed, noise, dtype)
            got, g1, g2 = fused(lib, shape, xt, st, seed, noise, dtype)
        assert float(np.std(want)) > 0
        assert np.array_equal(got, want), "threads %d tile %d" % (nth, tile)
        assert (g1, g2) == (w1, w2), "threads %d tile %d" % (nth, tile)


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128], ids=["c64", "c128"])
def test_split_x_axis_takes_the_unfused_fallback(lib, cases, dtype):
    """An x axis in the four-step form is not fused: the sequence generates into its scratch array and runs the unfused passes."""
    shape = (40, 60, 80)
    xt, st, noise = cases[shape]
    old = lib.emu_set_generic_cap(16)              # 40 = 8 x 5, 60 = 10 x 6: x and y split; 40 = nz / 2 too
    try:
        for nth, tile in ((1, 3), (16, 4)):
            with emu_util.generic_threads(nth, tile):
                for seed, nz_ in ((99, None), (0, noise)):
                    want, w1, w2 = unfused(shape, xt, st, seed, nz_, dtype)
                    got, g1, g2 = fused(lib, shape, xt, st, seed, nz_, dtype)
                    assert np.array_equal(got, want) and (g1, g2) == (w1, w2)
    finally:
        lib.emu_set_generic_cap(old)
    # (the cap did bite: the four-step form rounds differently from the whole-line form, and computes the same field)
    plain = unfused(shape, xt, st, 0, noise, dtype)[0]
    tol = 6e-6 if dtype == np.complex64 else 6e-14        # each form within 3e-6 / 3e-14 * std of the exact transform (test_emulator.py)
    assert not np.array_equal(want, plain) and np.max(np.abs(want - plain)) <= tol * float(np.std(plain))


def _header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "randomfield_hip.h")) as f:
        return f.read()


def test_abi_names_the_flag_and_the_feature():
    from randomfield_amd import _hip
    assert _hip.FEATURES["generic_fused"] == 1 << 13
    h = _header()
    assert re.search(r"RF_FLAG_FUSED_GENERIC_GENERATION\s*=\s*64\b", h)
    assert re.search(r"RF_FEATURE_GENERIC_FUSED\s*=\s*1\s*<<\s*13\b", h)
    assert (_hip.ABI_MAJOR, _hip.ABI_MINOR) >= (5, 4)


def test_library_reports_the_feature():
    from randomfield_amd import _hip
    lib = _hip.load()
    assert lib.rf_abi_features() & (1 << 13)
    assert "generic_fused" in _hip.abi_features()
