"""The cloud-in-cell gather on the CPU: the emulator (csrc/emu emu_particles_gather: the rf_core.h functions cic_gather_global /
cic_gather_tiled / cic_gather_value / cic_gather_out that rf_k_particles.hip calls, on real host threads, the tiled form over a tile
array it really stages), the numpy backend (randomfield_amd/particles.py gather, Generator.interpolate_at_particles / shift_particles)
and the ABI surface.

Oracle: tests/gather_oracle.py, float64 numpy over tests/cic_oracle.py's per-axis terms.  The definition fixes every rounding, so every
comparison of gathered values is np.array_equal.  The adjoint identity is checked in Python integers."""
import ctypes
import os

import numpy as np
import pytest

import cic_oracle as orc
import emu_util
import gather_oracle as gorc

SPACING = 0.5            # a power of two: whole and half cells are exact in float32
INV_H = [1.0 / SPACING] * 3
# (4,6,8) and (8,8,16): the tile of the kernels' brick (8, 8, 64) + halo 2 is larger than the grid on every axis
SHAPES = [(4, 6, 8), (8, 8, 16), (16, 16, 16), (30, 14, 22), (16, 32, 64)]
REALS = [np.float32, np.float64]
COEFF = 0.3              # not a power of two, not representable: the coefficient stays float64
_c_dp = ctypes.POINTER(ctypes.c_double)
_c_up = ctypes.POINTER(ctypes.c_ulonglong)
# (form, threads, brick, halo): the kernels' geometry and a small brick with several, partial bricks
RUNS = [(1, 1, None, 0), (1, 5, None, 0), (2, 1, (8, 8, 64), 2), (2, 7, (8, 8, 64), 2), (2, 1, (3, 2, 4), 1), (2, 4, (3, 2, 4), 2)]


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else np.dtype(v).name


@pytest.fixture(scope="module")
def lib():
    lib = emu_util.lib()
    lib.emu_particles_gather.argtypes = ([ctypes.c_int] * 4 + [ctypes.c_void_p] * 3 + [_c_dp] + [ctypes.c_void_p] * 2 + [ctypes.c_double]
                                         + [ctypes.c_int] * 7 + [_c_up])
    lib.emu_particles_gather.restype = ctypes.c_int
    return lib


def emu_gather(lib, s3, W, form, brick=None, halo=2, nth=1, coeff=1.0, first=True, G=None, inv_h=INV_H):
    s3 = [np.ascontiguousarray(s) for s in s3]
    W = np.ascontiguousarray(W)
    nx, ny, nz = W.shape
    brick = brick or (8, 8, 64)
    G = np.full(W.shape, 777, W.dtype) if G is None else np.ascontiguousarray(G).copy()
    dropped = ctypes.c_ulonglong(99)
    h = np.asarray(inv_h, np.float64)
    rc = lib.emu_particles_gather(int(W.dtype == np.float64), nx, ny, nz, s3[0].ctypes.data, s3[1].ctypes.data, s3[2].ctypes.data,
                                  h.ctypes.data_as(_c_dp), W.ctypes.data, G.ctypes.data, coeff, 1 if first else 0, form, brick[0], brick[1],
                                  brick[2], max(halo, 1), nth, ctypes.byref(dropped))
    assert rc == 0
    return G, int(dropped.value)


_CASES = {}


def case_of(shape, rt):
    """the displacement sets rounded to the real type, a field of normal deviates, a random G, and the oracle's results (computed once)"""
    key = (shape, np.dtype(rt).name)
    if key not in _CASES:
        rng = np.random.RandomState(sum(shape))
        W = rng.normal(size=shape).astype(rt)
        G0 = rng.normal(size=shape).astype(rt)
        sets = {}
        for name, s in orc.displacement_sets(shape, SPACING).items():
            s = s.astype(rt)
            sets[name] = (s, gorc.gather(s, INV_H, W), gorc.gather(s, INV_H, W, COEFF, False, G0))
        _CASES[key] = (W, G0, sets)
    return _CASES[key]


@pytest.mark.parametrize("rt", REALS, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_both_forms_and_thread_counts_equal_the_oracle(lib, shape, rt):
    W, G0, sets = case_of(shape, rt)
    for name, (s, (want, wdrop), (want_add, _)) in sets.items():
        assert wdrop == 0
        for form, nth, brick, halo in RUNS:
            G, dropped = emu_gather(lib, s, W, form, brick, halo, nth)
            assert dropped == 0 and G.dtype == rt and np.array_equal(G, want), (name, form, nth, brick)
            G, dropped = emu_gather(lib, s, W, form, brick, halo, nth, coeff=COEFF, first=False, G=G0)
            assert dropped == 0 and np.array_equal(G, want_add), (name, form, nth, brick)
    assert np.array_equal(sets["zero"][1][0], W)                                     # every particle sits on its own cell
    assert np.array_equal(sets["plus3"][1][0], np.roll(W, (-3, -3, -3), (0, 1, 2)))  # three whole cells: the field rolled by three


@pytest.mark.parametrize("rt", REALS, ids=_ids)
@pytest.mark.parametrize("shape", [(4, 6, 8), (16, 16, 16), (30, 14, 22)], ids=_ids)
def test_adjoint_of_the_paint_exactly(lib, shape, rt):
    """integer field in [-15, 15]: every product and sum of the gather is exact, and sum_q g 2^48 == sum_cells A W in integers"""
    rng = np.random.RandomState(5)
    W = rng.randint(-15, 16, size=shape).astype(rt)
    for name, s in orc.displacement_sets(shape, SPACING).items():
        s = s.astype(rt)
        lhs, rhs = gorc.adjoint_sums(s, INV_H, W)
        assert lhs == rhs, name
        for form, nth in ((1, 3), (2, 3)):
            # (float64 copies of the same displacements and field: g itself comes back, not rounded to float32)
            G, _ = emu_gather(lib, s.astype(np.float64), W.astype(np.float64), form, nth=nth)
            scaled = G * 2.0 ** 48
            assert np.all(scaled == np.floor(scaled)) and sum(int(v) for v in scaled.ravel()) == rhs, (name, form)


@pytest.mark.parametrize("rt", REALS, ids=_ids)
def test_constant_and_linear_fields(lib, rt):
    shape = (16, 16, 16)
    sets = orc.displacement_sets(shape, SPACING)
    s = sets["rms3"].astype(rt)
    const = np.full(shape, 2.75, rt)
    ix, iy, iz = np.meshgrid(*[np.arange(n, dtype=np.float64) for n in shape], indexing="ij")
    lin = (3 * ix - 2 * iy + iz).astype(rt)
    terms = [orc.axis_terms(s[a], INV_H[a], a) for a in range(3)]
    inside = np.ones(shape, bool)
    want = np.zeros(shape, np.float64)
    for a, c in enumerate((3.0, -2.0, 1.0)):
        _, (j0, j1), (w0, w1) = terms[a]
        inside &= np.broadcast_to(j1 == j0 + 1, shape)                               # the two cells do not straddle the wrap
        want = want + c * (np.broadcast_to(j0, shape) + np.broadcast_to(w1, shape).astype(np.float64) / 65536.0)
    assert 0 < np.count_nonzero(inside) < inside.size
    for form, nth in ((1, 2), (2, 2)):
        G, _ = emu_gather(lib, s, const, form, nth=nth)
        assert np.array_equal(G, const), form                                        # the weights sum to 2^48: a constant returns itself
        G, _ = emu_gather(lib, s, lin, form, nth=nth)
        # small integers times 16-bit weights: every step exact, the defining property of CIC holds to the last bit
        assert np.array_equal(G[inside].astype(np.float64), want[inside].astype(rt).astype(np.float64)), form


@pytest.mark.parametrize("rt", REALS, ids=_ids)
def test_forms_agree_when_particles_leave_the_tile(lib, rt):
    shape = (16, 32, 64)
    W, G0, sets = case_of(shape, rt)
    s = sets["rms3"][0]
    stay = np.ones(shape, bool)
    for a, (b, halo) in enumerate(((8, 2), (8, 2), (64, 2))):
        l = (np.arange(shape[a]) % b).reshape([-1 if c == a else 1 for c in range(3)])
        lo = l + np.floor(s[a].astype(np.float64) * INV_H[a])
        stay &= (lo >= -halo) & (lo <= b + halo - 2)
    assert 0 < np.count_nonzero(stay) < stay.size                                    # both branches of the tiled form run
    G1, _ = emu_gather(lib, s, W, 1)
    G2, _ = emu_gather(lib, s, W, 2, nth=3)
    assert np.array_equal(G1, G2)


@pytest.mark.parametrize("rt", REALS, ids=_ids)
def test_non_finite_displacements_gather_zero_and_are_counted(lib, rt):
    shape = (8, 8, 16)
    W, G0, sets = case_of(shape, rt)
    s = sets["rms3"][0].copy()
    s[1][2, 3, 5] = np.nan
    s[2][7, 0, 15] = np.inf
    bad = np.zeros(shape, bool)
    bad[2, 3, 5] = bad[7, 0, 15] = True
    want, wdrop = gorc.gather(s, INV_H, W)
    want_add, _ = gorc.gather(s, INV_H, W, COEFF, False, G0)
    assert wdrop == 2 and not want[bad].any() and np.array_equal(want_add[bad], G0[bad])
    assert np.array_equal(want[~bad], sets["rms3"][1][0][~bad])
    for form, nth, brick, halo in RUNS:
        G, dropped = emu_gather(lib, s, W, form, brick, halo, nth)
        assert dropped == 2 and np.array_equal(G, want), (form, nth, brick)
        G, dropped = emu_gather(lib, s, W, form, brick, halo, nth, coeff=COEFF, first=False, G=G0)
        assert dropped == 2 and np.array_equal(G, want_add), (form, nth, brick)


def test_non_finite_field_values_reach_zero_weights(lib):
    """zero weights are not skipped: a particle exactly on a cell has weight 0 on its seven other cells and still sees their NaN"""
    shape = (4, 6, 8)
    W = np.ones(shape, np.float64)
    W[1, 2, 4] = np.nan
    s = np.zeros((3,) + shape, np.float64)
    want, _ = gorc.gather(s, INV_H, W)
    near = np.zeros(shape, bool)
    near[0:2, 1:3, 3:5] = True                                                       # the particles whose j0 / j1 include (1, 2, 4)
    assert np.array_equal(np.isnan(want), near)
    for form in (1, 2):
        G, _ = emu_gather(lib, s, W, form, nth=2)
        assert np.array_equal(G, want, equal_nan=True)


def test_huge_displacements_stay_inside_the_grid(lib):
    shape = (4, 6, 8)
    rng = np.random.RandomState(2)
    W = rng.normal(size=shape)
    s = np.zeros((3,) + shape, np.float64)
    s[0][1, 2, 3] = 1e300
    s[1][1, 2, 3] = -3e18
    s[2][1, 2, 3] = 2.0 ** 40 + 0.25
    s[2][0, 0, 0] = -1e-300
    want, wdrop = gorc.gather(s, INV_H, W)
    assert wdrop == 0 and np.all(np.isfinite(want))
    for form, nth, brick, halo in RUNS:
        G, dropped = emu_gather(lib, s, W, form, brick, halo, nth)
        assert dropped == 0 and np.array_equal(G, want), (form, brick)
    big = np.full((3,) + shape, 1e308)               # the product overflows float64: dropped, as a non-finite displacement is
    G, dropped = emu_gather(lib, big, W, 1)
    assert dropped == W.size and not G.any() and gorc.gather(big, INV_H, W)[1] == dropped


# ---- the numpy backend -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rt", REALS, ids=_ids)
def test_numpy_gather_against_the_oracle(rt):
    from randomfield_amd import particles
    shape = (30, 14, 22)
    W, G0, sets = case_of(shape, rt)
    for name, (s, (want, wdrop), (want_add, _)) in sets.items():
        out, dropped = particles.gather(s, INV_H, W)
        assert out.dtype == rt and dropped == wdrop and np.array_equal(out, want), name
        out, dropped = particles.gather(s, INV_H, W, COEFF, False, G0.copy())
        assert np.array_equal(out, want_add), name
    s = sets["rms3"][0].copy()
    s[0][3, 4, 5] = np.nan
    want, wdrop = gorc.gather(s, INV_H, W)
    out, dropped = particles.gather(s, INV_H, W)
    assert dropped == 1 == wdrop and np.array_equal(out, want)
    want_add, _ = gorc.gather(s, INV_H, W, COEFF, False, G0)
    assert np.array_equal(particles.gather(s, INV_H, W, COEFF, False, G0.copy())[0], want_add)


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128], ids=_ids)
def test_numpy_generator_interpolates_and_shifts(dtype):
    from randomfield_amd import Generator
    shape = (16, 16, 16)
    rt = np.float32 if dtype == np.complex64 else np.float64
    eps = np.finfo(rt).eps
    gen = Generator(*shape, SPACING, backend="numpy", dtype=dtype)
    field = gen.generate_delta_field(seed=11, save_potential=True).copy()
    with pytest.raises(RuntimeError, match="No particle displacements"):
        gen.interpolate_at_particles()
    s = orc.displacement_sets(shape, SPACING)["rms3"].astype(rt)
    s[0][3, 4, 5] = np.nan
    gen.set_particle_displacements(s)
    with pytest.raises(RuntimeError, match="No gathered values"):
        gen.shift_particles(0)
    got = gen.interpolate_at_particles()
    want, wdrop = gorc.gather(s, INV_H, field)
    assert got.dtype == rt and np.array_equal(got, want) and gen.particles_dropped == 1 == wdrop
    assert np.array_equal(gen.plan_c2r.data_out, field)                              # the field is left as it is
    other = np.random.RandomState(4).normal(size=shape).astype(rt)
    got2 = gen.interpolate_at_particles(other, slot=2, coeff=COEFF)
    assert got2 is not got and np.array_equal(got2, gorc.gather(s, INV_H, other, COEFF)[0])
    assert np.array_equal(gen.plan_c2r.data_out, other)                              # a given array becomes the current field
    got3 = gen.interpolate_at_particles(field, slot=2, coeff=-1.5, first=False)
    assert np.array_equal(got3, gorc.gather(s, INV_H, field, -1.5, False, got2)[0])
    assert gen.interpolate_at_particles(slot=1, download=False) is None
    with pytest.raises(ValueError, match="slot"):
        gen.interpolate_at_particles(slot=3)
    # the shift: Q_axis + coeff G_slot within two roundings; the other components stay
    clean = np.nan_to_num(s)
    gen.set_particle_displacements(clean)
    g1 = gen.interpolate_at_particles(field, slot=1)
    gen.shift_particles(1, coeff=0.25)
    moved = gen._download_particles()
    add = 0.25 * g1.astype(np.float64)
    assert np.all(np.abs(moved[1] - (clean[1].astype(np.float64) + add)) <= 2 * eps * (np.abs(clean[1]) + np.abs(add)))
    assert np.array_equal(moved[0], clean[0]) and np.array_equal(moved[2], clean[2])
    gen.shift_particles(0, slot=1, coeff=0.25)
    assert np.all(np.abs(gen._download_particles()[0] - (clean[0].astype(np.float64) + add)) <= 2 * eps * (np.abs(clean[0]) + np.abs(add)))
    with pytest.raises(ValueError, match="axis"):
        gen.shift_particles(3)
    # a new field drops the gathered values with the displacements
    gen.generate_delta_field(seed=12, save_potential=True)
    with pytest.raises(RuntimeError, match="No particle displacements"):
        gen.interpolate_at_particles()
    gen.set_particle_displacements(clean)
    with pytest.raises(RuntimeError, match="No gathered values"):
        gen.shift_particles(0)


def test_abi_reports_the_gather():
    from randomfield_amd import _hip
    assert (_hip.ABI_MAJOR, _hip.ABI_MINOR) == (5, 5) and _hip.abi_version() == (5, 5)
    assert _hip.FEATURES["particles_gather"] == 1 << 19
    lib = _hip.load()
    assert lib.rf_abi_features() & (1 << 19)
    assert "particles_gather" in _hip.abi_features()
    for name in ("particles_gather", "particles_gather_download", "particles_shift", "set_gather_form"):
        assert hasattr(_hip.DevicePlan, name)
    for name in ("rf_particles_gather", "rf_particles_gather_download", "rf_particles_shift"):
        assert hasattr(lib, name) and name in _hip.SIGNATURES
    assert hasattr(lib, "rf_particles_set_gather_form") and "rf_particles_set_gather_form" in _hip.DIAG_SIGNATURES
    header = open(os.path.join(emu_util.ROOT, "include", "randomfield_hip.h")).read()
    assert "RF_FEATURE_PARTICLES_GATHER = 1 << 19" in header
    assert "#define RF_ABI_MAJOR 5" in header and "#define RF_ABI_MINOR 5" in header
