"""The triangular-shaped cloud on the CPU emulator (csrc/emu emu_particles_paint_ex / _gather_ex / _tile_stats_ex: the rf_core.h
functions tsc_particle / tsc_scatter_global / tsc_scatter_tiled / tsc_gather_global / tsc_gather_tiled that rf_k_particles.hip calls,
under the same two walks as cloud in cell, on real host threads with barriers, the tiled form over a tile array it really stages)
and the ABI surface.

Oracle: tests/tsc_oracle.py.  Integer weights and float64 steps rounded one by one: every comparison is ==."""
import ctypes
import os

import numpy as np
import pytest

import cic_oracle as corc
import emu_util
import tsc_oracle as orc

SPACING = 0.5
INV_H = [1.0 / SPACING] * 3
SHAPES = [(4, 6, 8), (10, 12, 70), (16, 16, 16)]          # smaller than the tile (slots alias); partial bricks, two in z; whole bricks in x, y
REALS = [np.float32, np.float64]
COEFF = 0.3
TSC, CIC = 3, 2
_c_dp = ctypes.POINTER(ctypes.c_double)
_c_up = ctypes.POINTER(ctypes.c_ulonglong)
# (form, threads, brick, halo): the global walk; the library's geometry; small bricks with halo 1 and halo 2
RUNS = [(1, 1, None, 0), (1, 5, None, 0), (2, 1, (8, 8, 64), 2), (2, 7, (8, 8, 64), 2), (2, 3, (2, 2, 4), 1), (2, 4, (4, 4, 8), 2)]


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else np.dtype(v).name


@pytest.fixture(scope="module")
def lib():
    lib = emu_util.lib()
    lib.emu_particles_paint_ex.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3 + [_c_dp] + [ctypes.c_int] * 6 + [_c_up, _c_up]
    lib.emu_particles_paint_ex.restype = ctypes.c_int
    lib.emu_particles_gather_ex.argtypes = ([ctypes.c_int] * 5 + [ctypes.c_void_p] * 3 + [_c_dp] + [ctypes.c_void_p] * 2 + [ctypes.c_double]
                                            + [ctypes.c_int] * 7 + [_c_up])
    lib.emu_particles_gather_ex.restype = ctypes.c_int
    lib.emu_particles_tile_stats_ex.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3 + [_c_dp] + [ctypes.c_int] * 4 + [_c_up]
    lib.emu_particles_tile_stats_ex.restype = ctypes.c_int
    return lib


def _arrays(s3):
    s3 = [np.ascontiguousarray(s) for s in s3]
    return s3, [s.ctypes.data for s in s3], int(s3[0].dtype == np.float64)


def emu_paint(lib, s3, form, brick=None, halo=2, nth=1, scheme=TSC, rc_want=0):
    s3, ptrs, f64 = _arrays(s3)
    nx, ny, nz = s3[0].shape
    brick = brick or (8, 8, 64)
    A = np.full((nx, ny, nz), 7, np.uint64)
    dropped = ctypes.c_ulonglong(99)
    h = np.asarray(INV_H, np.float64)
    rc = lib.emu_particles_paint_ex(f64, scheme, nx, ny, nz, *ptrs, h.ctypes.data_as(_c_dp), form, brick[0], brick[1], brick[2], max(halo, 1), nth,
                                    A.ctypes.data_as(_c_up), ctypes.byref(dropped))
    assert rc == rc_want
    return A, int(dropped.value)


def emu_gather(lib, s3, W, form, brick=None, halo=2, nth=1, coeff=1.0, first=True, G=None, scheme=TSC, rc_want=0):
    s3, ptrs, f64 = _arrays(s3)
    W = np.ascontiguousarray(W)
    nx, ny, nz = W.shape
    brick = brick or (8, 8, 64)
    G = np.full(W.shape, 777, W.dtype) if G is None else np.ascontiguousarray(G).copy()
    dropped = ctypes.c_ulonglong(99)
    h = np.asarray(INV_H, np.float64)
    rc = lib.emu_particles_gather_ex(f64, scheme, nx, ny, nz, *ptrs, h.ctypes.data_as(_c_dp), W.ctypes.data, G.ctypes.data, coeff, 1 if first else 0,
                                     form, brick[0], brick[1], brick[2], max(halo, 1), nth, ctypes.byref(dropped))
    assert rc == rc_want
    return G, int(dropped.value)


def emu_tile_stats(lib, s3, brick, halo, scheme=TSC):
    s3, ptrs, f64 = _arrays(s3)
    nx, ny, nz = s3[0].shape
    out4 = (ctypes.c_ulonglong * 4)()
    h = np.asarray(INV_H, np.float64)
    assert lib.emu_particles_tile_stats_ex(f64, scheme, nx, ny, nz, *ptrs, h.ctypes.data_as(_c_dp), brick[0], brick[1], brick[2], halo, out4) == 0
    return [int(v) for v in out4]


_CASES = {}


def case_of(shape, rt):
    """the displacement sets rounded to the real type with one NaN / inf set added, a field, a random G and the oracle's results (once)"""
    key = (shape, np.dtype(rt).name)
    if key not in _CASES:
        rng = np.random.RandomState(sum(shape))
        W = rng.normal(size=shape).astype(rt)
        G0 = rng.normal(size=shape).astype(rt)
        sets = dict(orc.displacement_sets(shape, SPACING))
        sets.update(orc.extra_sets(shape, SPACING))
        bad = sets["rms0.6"].copy()
        bad[1][1, 2, 3] = np.nan
        bad[2][tuple(n - 1 for n in shape)] = np.inf
        sets["non-finite"] = bad
        out = {}
        for name, s in sets.items():
            s = s.astype(rt)
            out[name] = (s, orc.paint(s, INV_H), orc.gather(s, INV_H, W), orc.gather(s, INV_H, W, COEFF, False, G0))
        _CASES[key] = (W, G0, out)
    return _CASES[key]


@pytest.mark.parametrize("rt", REALS, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_paint_both_walks_equal_the_oracle(lib, shape, rt):
    _, _, sets = case_of(shape, rt)
    n = int(np.prod(shape))
    for name, (s, (want, wdrop), _, _) in sets.items():
        assert wdrop == (2 if name == "non-finite" else 0) and orc.total(want) == (n - wdrop) * orc.ONE
        for form, nth, brick, halo in RUNS:
            A, dropped = emu_paint(lib, s, form, brick, halo, nth)
            assert dropped == wdrop and np.array_equal(A, want), (name, form, nth, brick)
    for name in ("zero", "plus3", "minus2.5"):
        assert np.all(sets[name][1][0] == np.uint64(orc.ONE)), name


@pytest.mark.parametrize("rt", REALS, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_gather_both_walks_equal_the_oracle(lib, shape, rt):
    W, G0, sets = case_of(shape, rt)
    for name, (s, _, (want, wdrop), (want_add, _)) in sets.items():
        for form, nth, brick, halo in RUNS:
            G, dropped = emu_gather(lib, s, W, form, brick, halo, nth)
            assert dropped == wdrop and G.dtype == rt and np.array_equal(G, want), (name, form, nth, brick)
            G, dropped = emu_gather(lib, s, W, form, brick, halo, nth, coeff=COEFF, first=False, G=G0)
            assert dropped == wdrop and np.array_equal(G, want_add), (name, form, nth, brick)
    # three whole cells: the same weights (1/8, 3/4, 1/8 per axis, the middle of a cell) on the field rolled by three
    assert np.array_equal(sets["plus3"][2][0], orc.gather(sets["zero"][0], INV_H, np.roll(W, (-3, -3, -3), (0, 1, 2)))[0])


@pytest.mark.parametrize("shape", [(4, 6, 8), (10, 12, 70)], ids=_ids)
def test_adjoint_of_the_paint_exactly(lib, shape):
    rng = np.random.RandomState(5)
    W = rng.randint(-15, 16, size=shape).astype(np.float64)
    for name in ("rms0.6", "rms3", "half", "one"):
        s = case_of(shape, np.float64)[2][name][0]
        lhs, rhs = orc.adjoint_sums(s, INV_H, W)
        assert lhs == rhs, name
        for form, nth in ((1, 3), (2, 3)):
            G, _ = emu_gather(lib, s, W, form, nth=nth)
            scaled = G * 2.0 ** 48
            assert np.all(scaled == np.floor(scaled)) and sum(int(v) for v in scaled.ravel()) == rhs, (name, form)


def test_tile_rule_and_stats(lib):
    """the tiled walk's own count of the particles that leave their tile equals the rule -h <= l + c_lo <= b + h - 3 restated by the
    oracle; every particle with |u| < 1.5 stays under halo 2"""
    shape = (16, 32, 128)
    sets = dict(orc.displacement_sets(shape, SPACING))
    sets.update(orc.extra_sets(shape, SPACING))
    for brick, halo in (((8, 8, 64), 2), ((4, 4, 8), 2), ((2, 2, 4), 1)):
        for name in ("uniform", "rms0.6", "rms3", "rms7", "huge"):
            s = sets[name].astype(np.float32)
            stay = orc.stays_in_tile(s, INV_H, brick, halo)
            fallback, fallback_adds, flushed, dropped = emu_tile_stats(lib, s, brick, halo)
            assert fallback == stay.size - np.count_nonzero(stay) and dropped == 0, (name, brick)
            assert fallback_adds <= 27 * fallback and flushed > 0
            if halo == 2:
                near = np.all(np.abs(s.astype(np.float64) * INV_H[0]) < 1.5, axis=0)
                assert np.all(stay[near]), (name, brick)
    assert emu_tile_stats(lib, sets["uniform"].astype(np.float32), (8, 8, 64), 2)[0] == 0
    st = orc.stays_in_tile(sets["rms7"], INV_H, (8, 8, 64), 2)
    assert np.count_nonzero(st) < st.size // 2                                       # most particles of the wide set leave the tile
    # cloud in cell through the same entry point is the old entry point
    s = sets["rms3"].astype(np.float32)
    old = (ctypes.c_ulonglong * 4)()
    h = np.asarray(INV_H, np.float64)
    _, ptrs, f64 = _arrays(s)
    lib.emu_particles_tile_stats.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3 + [_c_dp] + [ctypes.c_int] * 4 + [_c_up]
    assert lib.emu_particles_tile_stats(f64, *shape, *ptrs, h.ctypes.data_as(_c_dp), 8, 8, 64, 2, old) == 0
    assert emu_tile_stats(lib, s, (8, 8, 64), 2, scheme=CIC) == [int(v) for v in old]


def test_scheme_argument(lib):
    shape = (4, 6, 8)
    W, G0, sets = case_of(shape, np.float32)
    s = sets["rms3"][0]
    for form in (1, 2):
        A, _ = emu_paint(lib, s, form, scheme=CIC, nth=2)
        assert np.array_equal(A, corc.paint(s, INV_H)[0])
    for bad in (1, 4, 0):
        emu_paint(lib, s, 1, scheme=bad, rc_want=-1)
        emu_gather(lib, s, W, 1, scheme=bad, rc_want=-1)


def test_non_finite_field_values_reach_zero_weights(lib):
    """a NaN reaches every particle whose 27 cells contain it -- zero weights are not skipped: in the second set Wp = 0 (tau = 100 < 363)
    and the particles one cell below the NaN see it through that weight alone"""
    shape = (4, 6, 8)
    W = np.ones(shape, np.float64)
    W[1, 2, 4] = np.nan
    for s in (np.zeros((3,) + shape), np.full((3,) + shape, (-0.5 + 100 / 65536.0) * SPACING)):
        want, _ = orc.gather(s, INV_H, W)
        for form in (1, 2):
            G, _ = emu_gather(lib, s, W, form, nth=2)
            assert np.array_equal(G, want, equal_nan=True)
            assert np.count_nonzero(np.isnan(G)) == 27
    near = np.zeros(shape, bool)
    near[0:3, 1:4, 3:6] = True                                                       # zero displacement: the cells around (1, 2, 4)
    assert np.array_equal(np.isnan(orc.gather(np.zeros((3,) + shape), INV_H, W)[0]), near)


def test_abi_reports_the_scheme():
    from randomfield_amd import _hip
    assert (_hip.ABI_MAJOR, _hip.ABI_MINOR) == (5, 5) and _hip.abi_version() == (5, 5)
    assert _hip.FEATURES["particles_tsc"] == 1 << 20
    lib = _hip.load()
    assert lib.rf_abi_features() & (1 << 20)
    assert "particles_tsc" in _hip.abi_features()
    for name in ("rf_particles_paint_ex", "rf_particles_gather_ex"):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    header = open(os.path.join(emu_util.ROOT, "include", "randomfield_hip.h")).read()
    assert "RF_FEATURE_PARTICLES_TSC = 1 << 20" in header
    assert "enum { RF_ASSIGN_CIC = 2, RF_ASSIGN_TSC = 3 };" in header
    assert "int rf_particles_paint_ex(rf_plan* plan, const double* inv_h, int scheme, unsigned long long* dropped);" in header
    assert ("int rf_particles_gather_ex(rf_plan* plan, const double* inv_h, int scheme, int slot, double coeff, int first, "
            "unsigned long long* dropped);") in header
    assert "#define RF_ABI_MAJOR 5" in header and "#define RF_ABI_MINOR 5" in header
