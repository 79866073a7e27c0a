"""Particles on the CPU: the cloud-in-cell paint and the displacement buffer's fma step through the emulator (csrc/emu: the rf_core.h
functions cic_axis ... particles_axpy that rf_k_particles.hip calls, on real host threads with atomic adds), the numpy backend of
Generator.particle_displacements / paint_particles / particle_positions, and the ABI surface.

Oracle: tests/cic_oracle.py.  The accumulator grid is integer, so every comparison of it is np.array_equal.  The accumulate step: the
coefficient is exactly representable, so `first` is one rounding of coeff * W (eps/2 |coeff W|) and a further add is at most
two (a product and a sum without fma; one with it): 2 eps (|Q| + |coeff W|)."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import cic_oracle as orc
import emu_util

SPACING = 0.5            # a power of two: whole and half cells are exact in float32
INV_H = [1.0 / SPACING] * 3
SHAPES = [(4, 6, 8), (6, 4, 12), (16, 16, 16), (30, 14, 22)]
REALS = [np.float32, np.float64]
_c_dp = ctypes.POINTER(ctypes.c_double)
_c_up = ctypes.POINTER(ctypes.c_ulonglong)


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else np.dtype(v).name


@pytest.fixture(scope="module")
def lib():
    lib = emu_util.lib()
    lib.emu_particles_paint.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3 + [_c_dp] + [ctypes.c_int] * 6 + [_c_up, _c_up]
    lib.emu_particles_paint.restype = ctypes.c_int
    lib.emu_particles_accumulate.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong]
    lib.emu_particles_accumulate.restype = ctypes.c_int
    lib.emu_particles_delta.argtypes = [ctypes.c_int, _c_up, ctypes.c_void_p, ctypes.c_longlong]
    lib.emu_particles_delta.restype = ctypes.c_int
    lib.emu_particles_tile_stats.argtypes = [ctypes.c_int] * 4 + [ctypes.c_void_p] * 3 + [_c_dp] + [ctypes.c_int] * 4 + [_c_up]
    lib.emu_particles_tile_stats.restype = ctypes.c_int
    return lib


def emu_paint(lib, s3, form, brick=(8, 8, 64), halo=2, nth=1, inv_h=INV_H):
    s3 = [np.ascontiguousarray(s) for s in s3]
    nx, ny, nz = s3[0].shape
    A = np.full((nx, ny, nz), 12345, np.uint64)            # (the call clears it)
    dropped = ctypes.c_ulonglong(99)
    h = np.asarray(inv_h, np.float64)
    rc = lib.emu_particles_paint(int(s3[0].dtype == np.float64), nx, ny, nz, s3[0].ctypes.data, s3[1].ctypes.data, s3[2].ctypes.data,
                                 h.ctypes.data_as(_c_dp), form, brick[0], brick[1], brick[2], halo, nth, A.ctypes.data_as(_c_up),
                                 ctypes.byref(dropped))
    assert rc == 0
    return A, int(dropped.value)


_SETS = {}


def sets_of(shape, rt):
    """the displacement sets rounded to the real type, with the oracle's grid of each (computed once)"""
    key = (shape, np.dtype(rt).name)
    if key not in _SETS:
        out = {}
        for name, s in orc.displacement_sets(shape, SPACING).items():
            s = s.astype(rt)
            out[name] = (s, orc.paint(s, INV_H))
        _SETS[key] = out
    return _SETS[key]


@pytest.mark.parametrize("rt", REALS, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_both_forms_and_thread_counts_equal_the_oracle(lib, shape, rt):
    n = int(np.prod(shape))
    for name, (s, (want, wdrop)) in sets_of(shape, rt).items():
        assert wdrop == 0 and orc.total(want) == n * orc.ONE
        for form, nth in ((1, 1), (1, 5), (2, 1), (2, 7)):
            A, dropped = emu_paint(lib, s, form, nth=nth)
            assert dropped == 0, (name, form, nth)
            assert np.array_equal(A, want), (name, form, nth)
        # a small brick: several bricks, partial ones at the edge, halos of 1 and 2
        for halo in (1, 2):
            for nth in (1, 4):
                A, dropped = emu_paint(lib, s, 2, brick=(3, 2, 4), halo=halo, nth=nth)
                assert dropped == 0 and np.array_equal(A, want), (name, halo, nth)
    zero = sets_of(shape, rt)["zero"][1][0]
    assert np.all(zero == np.uint64(orc.ONE))
    for name in ("plus3", "minus2.5"):
        assert np.all(sets_of(shape, rt)[name][1][0] == np.uint64(orc.ONE)), name


@pytest.mark.parametrize("rt", REALS, ids=_ids)
def test_one_particle_against_hand_computed_weights(lib, rt):
    shape = (4, 6, 8)
    s = sets_of(shape, rt)["one"][0]
    q = tuple(n - 1 for n in shape)
    cells = orc.one_particle(shape, q, [s[a][q] for a in range(3)], INV_H)
    assert len(cells) == 8 and sum(cells.values()) == orc.ONE
    want = np.full(shape, orc.ONE, np.uint64)
    want[q] = 0
    for cell, w in cells.items():
        want[cell] += np.uint64(w)
    for form in (1, 2):
        A, dropped = emu_paint(lib, s, form, brick=(2, 2, 4), halo=1, nth=3)
        assert dropped == 0 and np.array_equal(A, want)
    # 0.3 cells along x from the last cell: weights 0.7 / 0.3 in units of 2^-16, floor((0.3 rounded) * 65536) = 19660
    u = float(s[0][q]) * INV_H[0]
    assert int(np.floor(u * 65536)) == 19660
    assert sum(w for (jx, jy, jz), w in cells.items() if jx == 0) == 19660 << 32


@pytest.mark.parametrize("rt", REALS, ids=_ids)
def test_non_finite_displacements_are_dropped_and_counted(lib, rt):
    shape = (6, 4, 12)
    s = sets_of(shape, rt)["rms3"][0].copy()
    s[1][2, 3, 5] = np.nan
    s[2][5, 0, 11] = np.inf
    omit = np.zeros(shape, bool)
    omit[2, 3, 5] = omit[5, 0, 11] = True
    clean = sets_of(shape, rt)["rms3"][0]
    want, _ = orc.paint(clean, INV_H, omit=omit)
    assert orc.total(want) == (int(np.prod(shape)) - 2) * orc.ONE
    assert orc.paint(s, INV_H)[1] == 2 and np.array_equal(orc.paint(s, INV_H)[0], want)
    for form, nth in ((1, 1), (1, 3), (2, 1), (2, 6)):
        A, dropped = emu_paint(lib, s, form, brick=(4, 4, 8), halo=2, nth=nth)
        assert dropped == 2 and np.array_equal(A, want)


def test_huge_displacements_stay_inside_the_grid(lib):
    """the mod is formed in float64 before the conversion to integer: any finite displacement gives an index in range"""
    shape = (4, 6, 8)
    s = np.zeros((3,) + shape, np.float64)
    s[0][1, 2, 3] = 1e300
    s[1][1, 2, 3] = -3e18
    s[2][1, 2, 3] = 2.0 ** 40 + 0.25
    s[2][0, 0, 0] = -1e-300                      # floor = -1 and u + 1 rounds to 1: t = 65536, all the weight on the cell itself
    want, wdrop = orc.paint(s, INV_H)
    assert wdrop == 0 and orc.total(want) == int(np.prod(shape)) * orc.ONE
    for form in (1, 2):
        A, dropped = emu_paint(lib, s, form, brick=(2, 3, 4), halo=1, nth=2)
        assert dropped == 0 and np.array_equal(A, want)
    big = np.full((3,) + shape, 1e308)           # the product overflows float64: dropped, as a non-finite displacement is
    A, dropped = emu_paint(lib, big, 1)
    assert dropped == int(np.prod(shape)) and not A.any() and orc.paint(big, INV_H)[1] == dropped


def test_tile_stats_follow_the_tile_rule(lib):
    """a particle at local index l of its brick stays in the tile iff -h <= l + floor(u) <= b + h - 2 on every axis -- the whole tile, not
    a window of +-h around the particle; counted here from that sentence alone"""
    shape, brick, halo = (6, 4, 12), (3, 2, 4), 2
    s = sets_of(shape, np.float64)["rms3"][0]
    stay = np.ones(shape, bool)
    for a in range(3):
        l = (np.arange(shape[a]) % brick[a]).reshape([-1 if b == a else 1 for b in range(3)])
        lo = l + np.floor(s[a] * INV_H[a])
        stay &= (lo >= -halo) & (lo <= brick[a] + halo - 2)
    assert 0 < np.count_nonzero(stay) < stay.size
    out = (ctypes.c_ulonglong * 4)()
    h = np.asarray(INV_H, np.float64)
    s3 = [np.ascontiguousarray(c) for c in s]
    assert lib.emu_particles_tile_stats(1, *shape, s3[0].ctypes.data, s3[1].ctypes.data, s3[2].ctypes.data, h.ctypes.data_as(_c_dp), *brick, halo,
                                        out) == 0
    assert out[0] == stay.size - np.count_nonzero(stay) and out[0] <= out[1] <= 8 * out[0] and out[3] == 0
    assert 0 < out[2] <= 8 * np.count_nonzero(stay)
    # more than the window of +-halo: some particle moves further than the halo and still stays
    moved = np.zeros(shape, bool)
    for a in range(3):
        c = np.floor(s[a] * INV_H[a])
        moved |= (c < -halo) | (c > halo - 1)
    assert np.any(stay & moved)


@pytest.mark.parametrize("rt", REALS, ids=_ids)
def test_delta_is_rounded_once(lib, rt):
    shape = (6, 4, 12)
    A = sets_of(shape, rt)["rms3"][1][0].copy()
    A[0, 0, 0] = np.uint64(2 ** 64 - 1)           # beyond 2^53: the conversion to float64 rounds
    A[0, 0, 1] = np.uint64(orc.ONE + 1)
    W = np.empty(shape, rt)
    assert lib.emu_particles_delta(int(rt == np.float64), A.ctypes.data_as(_c_up), W.ctypes.data, A.size) == 0
    assert np.array_equal(W, orc.delta(A, rt))
    from randomfield_amd import particles
    assert np.array_equal(particles.counts_to_delta(A, rt), orc.delta(A, rt))


@pytest.mark.parametrize("rt", REALS, ids=_ids)
@pytest.mark.parametrize("n", [1, 7, 4096], ids=str)
def test_accumulate_step_bounds(lib, rt, n):
    rng = np.random.RandomState(n)
    W1, W2 = rng.normal(size=n).astype(rt), rng.normal(size=n).astype(rt)
    eps = np.finfo(rt).eps
    Q = np.full(n, 7.0, rt)                       # (first: what Q held does not matter)
    c1, c2 = 0.75, 0.25
    assert lib.emu_particles_accumulate(int(rt == np.float64), 1, c1, W1.ctypes.data, Q.ctypes.data, n) == 0
    want1 = c1 * W1.astype(np.float64)
    assert np.all(np.abs(Q - want1) <= 0.5 * eps * np.abs(want1))
    Q1 = Q.copy()
    assert lib.emu_particles_accumulate(int(rt == np.float64), 0, c2, W2.ctypes.data, Q.ctypes.data, n) == 0
    add = c2 * W2.astype(np.float64)
    assert np.all(np.abs(Q - (Q1.astype(np.float64) + add)) <= 2 * eps * (np.abs(Q1) + np.abs(add)))
    c3 = 0.3                                      # not representable in float32: the coefficient is rounded to the real type once
    assert lib.emu_particles_accumulate(int(rt == np.float64), 1, c3, W1.ctypes.data, Q.ctypes.data, n) == 0
    assert np.array_equal(Q, rt(c3) * W1)


# ---- the numpy backend of the Generator --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.complex64, np.complex128], ids=_ids)
def test_numpy_backend_against_the_oracle(dtype):
    from randomfield_amd import Generator
    shape = (16, 16, 16)
    rt = np.float32 if dtype == np.complex64 else np.float64
    eps = np.finfo(rt).eps
    gen = Generator(*shape, SPACING, backend="numpy", dtype=dtype)
    gen.generate_delta_field(seed=11, save_potential=True)
    with pytest.raises(RuntimeError, match="No particle displacements"):
        gen.paint_particles()
    psi1 = [gen.calculate_displacement_field(a, order=1).astype(np.float64) for a in range(3)]
    psi2 = [gen.calculate_displacement_field(a, order=2).astype(np.float64) for a in range(3)]
    D1 = 0.5
    for order in (1, 2):
        s = gen.particle_displacements(order=order, D1=D1)
        assert s.shape == (3,) + shape and s.dtype == rt
        for a in range(3):
            want = D1 * psi1[a] + (D1 * D1 * psi2[a] if order == 2 else 0.0)
            bound = 2 * eps * (np.abs(D1 * psi1[a]) + np.abs(D1 * D1 * psi2[a]))
            assert np.all(np.abs(s[a] - want) <= bound)
    assert gen.particle_displacements(order=2, D1=D1, download=False) is None
    assert gen.paint_particles(download=False) is None
    assert gen.particle_displacements(order=2, D1=D1) is not gen.particle_displacements(order=2, D1=D1)     # new arrays
    with pytest.raises(ValueError, match="order"):
        gen.particle_displacements(order=3)
    A, wdrop = orc.paint(s, INV_H)
    got = gen.paint_particles()
    assert got.dtype == rt and np.array_equal(got, orc.delta(A, rt)) and gen.particles_dropped == 0 == wdrop
    assert np.array_equal(gen.particle_positions(), orc.positions(s, SPACING))
    pos = gen.particle_positions()
    assert pos.dtype == np.float64 and np.all((pos >= 0) & (pos < shape[0] * SPACING))
    # the painted field is the current field
    p_current = gen.measure_power_spectrum()
    p_given = gen.measure_power_spectrum(field=got.copy())
    for name in ("k", "Pk", "nmodes"):
        assert np.array_equal(p_current[name], p_given[name], equal_nan=True)
    # a caller's own displacements, one of them non-finite
    own = orc.displacement_sets(shape, SPACING)["rms3"].astype(rt)
    own[0][3, 4, 5] = np.nan
    gen.set_particle_displacements(own)
    A, wdrop = orc.paint(own, INV_H)
    assert np.array_equal(gen.paint_particles(), orc.delta(A, rt)) and gen.particles_dropped == 1 == wdrop
    with pytest.raises(ValueError, match="shape"):
        gen.set_particle_displacements(own[:2])
    # the potential and the displacement calls still work
    assert np.array_equal(gen.calculate_displacement_field(0, order=1).astype(np.float64), psi1[0])
    # a new field drops the displacements of the old one
    gen.generate_delta_field(seed=12, save_potential=True)
    with pytest.raises(RuntimeError, match="No particle displacements"):
        gen.paint_particles()
    with pytest.raises(RuntimeError, match="No particle displacements"):
        gen.particle_positions()


def test_abi_reports_particles():
    import os
    from randomfield_amd import _hip
    assert (_hip.ABI_MAJOR, _hip.ABI_MINOR) == (5, 5) and _hip.abi_version() == (5, 5)
    assert _hip.FEATURES["particles"] == 1 << 17
    lib = _hip.load()
    assert lib.rf_version() == (5 << 16) | 5
    assert lib.rf_abi_features() & (1 << 17)
    assert "particles" in _hip.abi_features()
    for name in ("particles_accumulate", "particles_upload", "particles_download", "particles_paint", "particles_download_counts",
                 "set_paint_form"):
        assert hasattr(_hip.DevicePlan, name)
    for name in ("rf_particles_accumulate", "rf_particles_upload", "rf_particles_download", "rf_particles_paint"):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    for name in ("rf_particles_download_counts", "rf_particles_set_paint_form", "rf_particles_paint_geometry"):
        assert hasattr(lib, name) and name in _hip.DIAG_SIGNATURES
    header = open(os.path.join(emu_util.ROOT, "include", "randomfield_hip.h")).read()
    assert "RF_FEATURE_PARTICLES = 1 << 17" in header
    assert "#define RF_ABI_MAJOR 5" in header and "#define RF_ABI_MINOR 5" in header
    nm = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
    names = [line.split()[-1] for line in nm.splitlines() if line.strip()]
    assert names and all(re.match(r"rf_[a-z0-9_]+$", n) for n in names), [n for n in names if not n.startswith("rf_")][:5]
