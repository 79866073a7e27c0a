"""The table, inputs, references and bound of tests/generic_matrix.py through the CPU emulator's generic path: the block functions of
csrc/rf_generic.h at every radix sequence and four-step split, in the form the library runs for each row (and, where the emulator's
prefer-split switch gives another form -- the one-line form of a strided axis that the library splits by preference -- in that form
too).  The counterpart of tests/test_gpu_generic_matrix.py: a case that passes here and fails there is a fault of the GPU build or
launch; one that fails in both is the arithmetic.

Every row runs with 3 lines per block (the walk by index, line counts that divide nothing) and with 1 (a thread stays on its line: the
kernels' own walk); rows of up to 120 points also on host threads with real barriers.  Rows with a dot-product stage longer than
generic_matrix.BIG_RADIX run the library's form at 3 lines per block only: one such stage is seconds of CPU time."""
import ctypes

import numpy as np
import pytest

import emu_util
import generic_matrix as gm
from conftest import golden
from oracle import cpu_ref

THREADED = ((16, 4), (32, 16))           # (host threads, lines per block): GenericWalk::fixed, as in every kernel launch
SPACING = 0.5

# the lengths the table was designed with: a row taken out of generic_matrix fails here (or at a coverage guard)
MIN_STRIDED = {2 << i for i in range(13)} | {
    6, 10, 12, 18, 20, 24, 30, 40, 50, 60, 96, 100, 120, 360, 1000, 1536, 4374, 5000, 6000, 6144, 6250, 7776,
    14, 22, 26, 28, 34, 42, 56, 70, 98, 154, 254, 442, 2038, 2310, 3408, 3410, 4078, 6816, 6818, 7168, 8186,
    8194, 9898, 16384, 4098, 16382}
MIN_ZROW = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 21, 25, 27, 35, 49, 64, 105, 125, 243, 1019, 2048, 2187, 3125, 4093, 4096, 8194, 4098}


class Emulator:
    @staticmethod
    def c2r(shape, dtype, ks):
        out, s1, s2 = emu_util.generic_c2r(ks)
        mean = s1 / out.size
        return out, mean, float(np.sqrt(max(s2 / out.size - mean * mean, 0.0)))

    @staticmethod
    def r2c(shape, dtype, field):
        return emu_util.generic_r2c(field)

    @staticmethod
    def c2c(shape, dtype, a, inverse):
        return emu_util.generic_c2c(a, inverse)


def _tile(tile):
    class _Tile:
        def __enter__(self):
            self.old = emu_util.lib().emu_set_generic_tile(tile)

        def __exit__(self, *exc):
            emu_util.lib().emu_set_generic_tile(self.old)
            return False
    return _Tile()


def _other_form_differs(role, n, dtype):
    for packed in gm.plans_of(role):
        lib_form = gm.forms(role, n, dtype, packed)
        with emu_util.generic_prefer_split(False):
            if gm.forms(role, n, dtype, packed) != lib_form:
                return True
    return False


@pytest.fixture(scope="module")
def dpower():
    d = golden("default_power.npz")
    return d["k"], d["Pk"]


def _fused_equals_unfused(n, dtype, dpower):
    """x rows: the generation inside the x pass loads the same cells into the same generic_pos positions (bit for bit)"""
    lib = emu_util.lib()
    _c_dp = ctypes.POINTER(ctypes.c_double)
    lib.emu_generic_realise.argtypes = [ctypes.c_int] * 4 + [_c_dp] * 5 + [ctypes.c_int, ctypes.c_int, ctypes.c_uint64, _c_dp] + [ctypes.c_void_p, _c_dp, _c_dp]
    lib.emu_generic_realise.restype = ctypes.c_int
    nx, ny, nz = shape = gm.shape_of("x", n)
    xt, st = cpu_ref.sigma_table(*dpower, nx, ny, nz, SPACING)
    seed = 31337
    ks = emu_util.generate_kspace(nx, ny, nz, SPACING, xt, st, seed=seed, dtype=dtype)
    want, w1, w2 = emu_util.generic_c2r(ks)
    args, keep = emu_util._gen_args(nx, ny, nz, SPACING, xt, st, seed, None)
    got = np.empty(shape, gm.real_of(dtype))
    s1, s2 = ctypes.c_double(), ctypes.c_double()
    assert lib.emu_generic_realise(int(dtype == gm.C128), nx, ny, nz, *args, got.ctypes.data_as(ctypes.c_void_p), ctypes.byref(s1), ctypes.byref(s2)) == 0
    assert float(np.std(want)) > 0
    assert np.array_equal(got, want) and (s1.value, s2.value) == (w1, w2), ("fused generation", n, gm.dtype_name(dtype))


@pytest.mark.parametrize("role,n", gm.CASES, ids=gm.case_id)
def test_generic_transforms_at_every_radix_sequence(role, n, dpower):
    for dtype in gm.dtypes_of(role, n):
        big = max(gm.rmax_of(gm.forms(role, n, dtype, packed)) for packed in gm.plans_of(role)) > gm.BIG_RADIX
        one = gm.run_row(role, n, dtype, Emulator, " tile 3")                          # the library's form
        if big:
            continue
        with _tile(1):
            got = gm.run_row(role, n, dtype, Emulator, " tile 1")
        for key in one:
            assert np.array_equal(got[key], one[key]), (key, "tile 1 against tile 3")      # the same butterflies on the same values
        if role == "x":
            _fused_equals_unfused(n, dtype, dpower)
        if n <= 120:
            for nth, tile in THREADED:
                with emu_util.generic_threads(nth, tile):
                    got = gm.run_row(role, n, dtype, Emulator, " %d threads tile %d" % (nth, tile))
                for key in one:
                    assert np.array_equal(got[key], one[key]), (key, nth, tile)
        if _other_form_differs(role, n, dtype):
            with emu_util.generic_prefer_split(False):                                   # the one-line form of a line the library splits
                for tile in (3, 1):
                    with _tile(tile):
                        gm.run_row(role, n, dtype, Emulator, " one line, tile %d" % tile)
                if role == "x":
                    _fused_equals_unfused(n, dtype, dpower)


def test_the_table_reaches_every_stage_form_and_the_guards_bite():
    assert MIN_STRIDED <= set(gm.STRIDED) and MIN_ZROW <= set(gm.ZROW_M)
    assert len(set(gm.CASES)) == len(gm.CASES) == 3 * len(gm.STRIDED) + len(gm.ZROW_M)
    gm.guard_coverage()
    # rows whose removal a coverage guard notices by itself: the only ones of their kind
    for gone in ([("zrow", 1)],                                        # M = 1
                 [("zrow", m) for m in (3, 9, 15, 21, 27, 105, 243, 2187)],      # radix 3 first: odd lines only
                 [(r, 224) for r in ("x", "y", "zc2c")],               # 4 8 7: a radix 8 behind the first stage of a two-buffer line
                 [("zc2c", 3410)], [("zc2c", 6816)],                   # one side of a stage-table boundary
                 [(r, n) for r in ("x", "y") for n in (8186, 16382, 2038, 4078)]):      # n2 = 2 by preference (and forced, in complex128)
        with pytest.raises(AssertionError):
            gm.guard_coverage([c for c in gm.CASES if c not in gone])
    # the switch: at its default the emulator decides as the library (x = 4096 runs 64 x 64, 8186 runs 4093 x 2); 0 is one line
    f = emu_util.generic_axis_form(gm.C64, 4096, True)
    assert (f["n1"], f["n2"]) == (64, 64) and all(l["radices"] == (4, 4, 4) for l in f["lines"])
    f = emu_util.generic_axis_form(gm.C64, 8186, True)
    assert (f["n1"], f["n2"]) == (4093, 2)
    assert emu_util.generic_axis_form(gm.C64, 4096, False)["n1"] == 0          # contiguous axes never split by preference
    with emu_util.generic_prefer_split(False):
        f = emu_util.generic_axis_form(gm.C64, 4096, True)
        assert f["n1"] == 0 and f["lines"][0]["radices"] == (4,) * 6
        assert emu_util.generic_axis_form(gm.C64, 8194, True)["n1"] == 241     # beyond the cap: split whatever the switch says
    # the thresholds of the preference follow from generic_strided_tile's LDS formula: the first strided lengths that split
    for dtype, smooth, rough in ((gm.C64, 3894, 2272), (gm.C128, 1994, 1136)):
        cap = 8192 if dtype == gm.C64 else 4096
        first = {True: None, False: None}
        for n in range(2, cap + 1, 2):
            f = emu_util.generic_axis_form(dtype, n, True)
            with emu_util.generic_prefer_split(False):
                s = emu_util.generic_axis_form(dtype, n, True)["lines"][0]["smooth"]
            if f["n1"] and first[s] is None:
                first[s] = n
        assert first[True] > smooth and first[False] > rough, first
        with emu_util.generic_prefer_split(False):
            below = [n for n in range(2, smooth + 1, 2) if emu_util.generic_axis_form(dtype, n, True)["lines"][0]["smooth"]]
        assert not any(emu_util.generic_axis_form(dtype, n, True)["n1"] for n in below + list(range(2, rough + 1, 2)))


def test_the_library_accepts_what_the_emulator_reports():
    """rf_shape_supported_dtype (host code of the library: rf_capi.hip generic_dims) and the emulator's export call the same
    generic_axis_form: every packed shape of the table is a generic shape (2) in the dtypes it lists, and 16382 is refused in complex128"""
    from randomfield_amd import _hip
    lib = _hip.load()
    for role, n in gm.CASES:
        shape = gm.shape_of(role, n)
        for dtype in gm.DTYPES:
            served = emu_util.generic_shape_form(dtype, shape, True) is not None
            if True in gm.plans_of(role):
                assert served == (dtype in gm.dtypes_of(role, n)), (shape, gm.dtype_name(dtype))
            code = _hip.RF_F64 if dtype == gm.C128 else _hip.RF_F32
            assert lib.rf_shape_supported_dtype(*shape, code) == (2 if served else 0), (shape, gm.dtype_name(dtype))


def test_print_the_worst_figures():
    """(after the table: the worst measured / bound per transform, dtype and role, for CHANGES.md)"""
    for line in gm.worst_lines():
        print(line)
