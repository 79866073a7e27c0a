"""The table, inputs, references and bounds of tests/axis_matrix.py through the CPU emulator's r2c, c2r and c2c: the phase functions of
every tiled axis length, one axis long at a time, in both dtypes.  The counterpart of tests/test_gpu_axis_matrix.py -- a case that
passes here and fails there is a fault of the GPU build or launch; one that fails in both is phase-function logic."""
import numpy as np
import pytest

import axis_matrix as am
import emu_util


@pytest.mark.parametrize("axis,n", am.CASES, ids=am.case_id)
def test_r2c_c2r_c2c_one_long_axis(axis, n):
    for shape, dtype in am.plans(axis, n, packed=True):
        field = am.real_field(shape, dtype, n)
        spec = emu_util.r2c(field)
        bound = am.check("r2c", spec, am.rfftn(field), dtype, shape)
        am.check_hermitian(spec, bound, shape)
        for what, ks in zip(("c2r", "c2r raw"), am.half_spectra(shape, dtype, n)):
            ref = am.irfftn(ks, shape)
            out, s1, s2 = emu_util.c2r(ks)
            am.check(what, out, ref, dtype, shape)
            mean = s1 / out.size
            am.check_moments(what, mean, np.sqrt(max(s2 / out.size - mean * mean, 0.0)), ref, dtype, shape)
    for shape, dtype in am.plans(axis, n, packed=False):
        a = am.complex_array(shape, dtype, n)
        am.check("c2c forward", emu_util.c2c(a, inverse=False), am.fftn(a), dtype, shape)
        am.check("c2c inverse", emu_util.c2c(a, inverse=True), am.ifftn(a), dtype, shape)


def test_the_table_covers_every_length_and_the_guards_bite():
    """every tiled length on every axis; a companion moved out of its regime, or out of the tiled kernels, fails at the guard"""
    assert {n for a, n in am.CASES if a == "x"} == {n for a, n in am.CASES if a == "y"} == {8 << i for i in range(9)}
    assert {n for a, n in am.CASES if a == "z" and am.packed_shapes(a, n)} == {16 << i for i in range(8)}
    assert {n for a, n in am.CASES if a == "z" and am.c2c_shapes(a, n)} == {8 << i for i in range(9)}
    for packed in (True, False):
        for dtype in am.DTYPES:
            n = 256 if dtype == am.C64 else 128
            assert am.TILE_COLS[dtype][n] == 16
            with pytest.raises(AssertionError):        # short companion as wide as the 16-column tile
                am.guard("y", n, ((8, n, 32 if packed else 16), (8, n, 128)), dtype, packed)
            with pytest.raises(AssertionError):        # long companion narrower than the tile
                am.guard("y", 64, ((8, 64, 16 if packed else 8), (8, 64, 16 if packed else 8)), dtype, packed)
            with pytest.raises(AssertionError):        # not a tiled shape
                am.guard("x", 64, ((64, 8, 16), (64, 12, 128)), dtype, packed)
