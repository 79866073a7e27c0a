"""The interlaced paint on the host: the numpy definition of the half-cell shifted paint (randomfield_amd/particles.py), the default
phase tables and the combine (randomfield_amd/powertools.py), and the numpy backend of Generator.paint_particles(interlaced=True)
with measure_power_spectrum / measure_power_multipoles(source='kspace').

Oracle: tests/interlace_oracle.py.  Integer weights and float64 steps rounded one by one: the comparisons of counts and of the
combine are ==."""
import numpy as np
import pytest

import interlace_oracle as orc
from randomfield_amd import Generator, particles, powertools

SPACING = 0.5
INV_H = [1.0 / SPACING] * 3
SHAPE = (16, 16, 16)
ORDERS = {"cic": 2, "tsc": 3}


@pytest.mark.parametrize("rt", [np.float32, np.float64], ids=lambda t: np.dtype(t).name)
@pytest.mark.parametrize("scheme", ["cic", "tsc"])
def test_half_cell_is_the_paint_of_the_moved_particles(scheme, rt):
    """on the 2^-16-cell lattice s + h/2 is exact in both real types: the shifted paint is the paint of the particles moved by hand"""
    s = orc.lattice_displacements(SHAPE, SPACING, seed=3).astype(rt)
    moved = (s.astype(np.float64) + 0.5 * SPACING).astype(rt)
    assert np.array_equal(moved.astype(np.float64), s.astype(np.float64) + 0.5 * SPACING)
    A, dropped = particles.paint_counts(s, INV_H, ORDERS[scheme], half_cell=True)
    want, wdrop = particles.paint_counts(moved, INV_H, ORDERS[scheme])
    assert dropped == wdrop == 0 and A.dtype == np.uint64 and np.array_equal(A, want)
    assert orc.total(A) == s[0].size * orc.ONE
    assert np.array_equal(A, orc.paint(s, INV_H, ORDERS[scheme])[0])
    plain = particles.paint_counts(s, INV_H, ORDERS[scheme])[0]
    assert np.array_equal(plain, particles.paint_counts(s, INV_H, ORDERS[scheme], half_cell=False)[0]) and not np.array_equal(plain, A)


def _single(shape, q, s):
    """displacements with every particle NaN but the one at lattice cell q"""
    d = np.full((3,) + shape, np.nan)
    d[(slice(None),) + q] = s
    return d


# (name, lattice cell, u in cells along x, what the shifted particle's x terms must be: (j0', t'))
BY_HAND = [
    ("no carry", (3, 2, 1), 0.25, (3, 16384 + 32768)),
    ("carry", (3, 2, 1), 0.75, (4, 16384)),
    ("carry and wrap", (15, 2, 1), 0.75, (0, 16384)),
    ("t = 65536", (3, 2, 1), -(2.0 ** -60), (3, 32768)),
    ("c + 1 == c", (3, 2, 1), 1e30, ((3 + int(1e30 % 16)) % 16, 32768)),
]


@pytest.mark.parametrize("name,q,u,want", BY_HAND, ids=[c[0] for c in BY_HAND])
def test_one_particle_by_hand(name, q, u, want):
    j0, t = want
    s = np.array([u * SPACING, 0.0, 0.0])
    assert s[0] * INV_H[0] == u
    if name == "c + 1 == c":
        assert np.floor(u) + 1.0 == np.floor(u)
    # y and z: u = 0, t = 0 -> t' = 32768 without a carry: half the weight on the particle's own cell, half on the next
    cells = {}
    for (jx, wx) in ((j0, 65536 - t), ((j0 + 1) % 16, t)):
        for (jy, wy) in ((q[1], 32768), (q[1] + 1, 32768)):
            for (jz, wz) in ((q[2], 32768), (q[2] + 1, 32768)):
                if wx * wy * wz:
                    cells[jx, jy, jz] = wx * wy * wz
    assert sum(cells.values()) == orc.ONE
    assert orc.one_particle(SHAPE, q, s, INV_H) == cells
    A, dropped = particles.paint_counts(_single(SHAPE, q, s), INV_H, 2, half_cell=True)
    assert dropped == A.size - 1
    assert {tuple(int(i) for i in c): int(A[tuple(c)]) for c in np.argwhere(A)} == cells
    # the triangular-shaped cloud on the same (t', j0'): the oracle in Python numbers against the numpy definition
    A3, _ = particles.paint_counts(_single(SHAPE, q, s), INV_H, 3, half_cell=True)
    assert {tuple(int(i) for i in c): int(A3[tuple(c)]) for c in np.argwhere(A3)} == orc.one_particle(SHAPE, q, s, INV_H, orc.TSC)


@pytest.mark.parametrize("shape", [(16, 16, 16), (4, 6, 8)], ids=lambda s: "x".join(map(str, s)))
def test_phase_tables(shape):
    tabs = powertools.interlace_phases(shape)
    want = orc.phases(shape)
    assert [len(t) for t in tabs] == [shape[0], shape[1], shape[2] // 2 + 1]
    for a, (p, w) in enumerate(zip(tabs, want)):
        n = shape[a]
        assert p.dtype == np.complex128 and np.array_equal(p, w)
        assert p[0] == 1.0 and p[n // 2] == 0.0
        if a < 2:
            for i in range(1, n):
                assert p[n - i] == np.conj(p[i]), (a, i)
        assert np.allclose(np.abs(np.delete(p, n // 2)), 1.0, rtol=0, atol=1e-15)
        assert p[1].imag > 0          # exp(+i pi m / n)


def _interlaced(s, scheme, tables):
    out = []
    for half in (False, True):
        A, _ = particles.paint_counts(s, INV_H, ORDERS[scheme], half_cell=half)
        out.append(np.fft.rfftn(particles.counts_to_delta(A, np.float64), axes=(0, 1, 2)))
    return out[0], powertools.interlace_combine(out[0], out[1], tables)


def test_sign_of_the_phase():
    """a smooth displacement: both grids see the same field, so the right phase leaves mode (1, 0, 0) where it was"""
    ix = np.arange(16, dtype=np.float64).reshape(16, 1, 1)
    s = np.empty((3,) + SHAPE)
    s[0] = 0.3 * SPACING * np.sin(2 * np.pi * ix / 16)
    s[1] = 0.11 * SPACING
    s[2] = -0.2 * SPACING
    tabs = powertools.interlace_phases(SHAPE)
    d1, dint = _interlaced(s, "cic", tabs)
    err = abs(dint[1, 0, 0] - d1[1, 0, 0]) / abs(d1[1, 0, 0])
    _, dwrong = _interlaced(s, "cic", [np.conj(t) for t in tabs])
    wrong = abs(dwrong[1, 0, 0] - d1[1, 0, 0]) / abs(d1[1, 0, 0])
    print("relative change of mode (1,0,0): %.4g, with the opposite sign %.4g" % (err, wrong))
    assert err <= 0.05
    assert wrong > 0.05


def test_odd_images_cancel():
    """one particle: the interlaced value at a mode is the sum over the aliased images with an EVEN sum of image indices"""
    n, q, mode = 16, (3, 0, 0), (5, 3, 2)
    disp = np.array([0.37 * SPACING, 0.0, 0.0])
    s = _single(SHAPE, q, disp)
    d1, dint = _interlaced(s, "cic", powertools.interlace_phases(SHAPE))
    # the position as the paint quantises it, in cells
    x = [q[0] + np.floor(0.37 * 65536.0) / 65536.0, float(q[1]), float(q[2])]
    j = np.arange(-4000, 4001)
    per_axis, parity = [], []
    for a in range(3):
        qa = mode[a] + n * j.astype(np.float64)
        per_axis.append(np.sinc(qa / n) ** 2 * np.exp(-2j * np.pi * qa * x[a] / n))
        parity.append(j % 2)
    even = [np.sum(p[par == 0]) for p, par in zip(per_axis, parity)]
    odd = [np.sum(p[par == 1]) for p, par in zip(per_axis, parity)]
    # even sum of the three indices: (e, e, e) or two odd ones
    want = even[0] * even[1] * even[2] + even[0] * odd[1] * odd[2] + odd[0] * even[1] * odd[2] + odd[0] * odd[1] * even[2]
    got = dint[mode]
    print("|interlaced - even images| = %.3g, |plain - interlaced| = %.3g" % (abs(got - want), abs(d1[mode] - got)))
    assert abs(got - want) <= 1e-4
    assert abs(d1[mode] - got) > 1e-2


@pytest.mark.parametrize("ctype", [np.complex64, np.complex128], ids=lambda t: np.dtype(t).name)
def test_combine_definition_equals_the_oracle(ctype):
    rng = np.random.RandomState(4)
    shape = (4, 6, 8)
    kshape = (4, 6, 5)
    S = (rng.normal(size=kshape) + 1j * rng.normal(size=kshape)).astype(ctype)
    K = (rng.normal(size=kshape) + 1j * rng.normal(size=kshape)).astype(ctype)
    for tabs in (None, powertools.interlace_phases(shape), [None, orc.phases(shape)[1], None]):
        out = powertools.interlace_combine(S, K, tabs)
        assert out.dtype == ctype and np.array_equal(out, orc.combine(S, K, tabs))
    assert np.array_equal(powertools.interlace_combine(S, K, None), ((S.astype(np.complex128) + K.astype(np.complex128)) * 0.5).astype(ctype))


@pytest.mark.parametrize("scheme", ["cic", "tsc"])
def test_numpy_generator(scheme):
    gen = Generator(*SHAPE, SPACING, backend="numpy")
    rt = gen.plan_c2r.data_out.dtype
    s = (np.random.RandomState(8).normal(scale=0.8, size=(3,) + SHAPE) * SPACING).astype(rt)
    gen.set_particle_displacements(s)
    with pytest.raises(RuntimeError, match="interlaced"):
        gen.measure_power_spectrum(source="kspace")
    field = gen.paint_particles(interlaced=True, assignment=scheme)
    K, want, dropped = orc.interlaced(s, INV_H, ORDERS[scheme], rt)
    assert field.dtype == rt and field.shape == SHAPE and gen.particles_dropped == dropped == 0
    assert np.array_equal(field, want.astype(rt))
    kept = gen.measure_power_spectrum(source="kspace", window=scheme)
    multi = gen.measure_power_multipoles(source="kspace", window=scheme, los=0)
    plain = gen.measure_power_spectrum(source="kspace")
    # the same measurement of the returned field, in float64 (the kept spectrum is Hermitian: irfftn loses nothing)
    g64 = Generator(*SHAPE, SPACING, backend="numpy", dtype=np.complex128) if rt != np.float64 else gen
    again = g64.measure_power_spectrum(want, window=scheme)
    ok = again["nmodes"] > 0
    assert np.array_equal(kept["nmodes"], again["nmodes"])
    assert np.allclose(kept["Pk"][ok], again["Pk"][ok], rtol=1e-12, atol=0) and np.allclose(kept["k"][ok], again["k"][ok], rtol=1e-12, atol=0)
    assert np.allclose(multi["P0"][ok], g64.measure_power_multipoles(want, window=scheme, los=0)["P0"][ok], rtol=1e-12, atol=0)
    assert np.allclose(plain["Pk"][ok], g64.measure_power_spectrum(want)["Pk"][ok], rtol=1e-12, atol=0)


def test_source_argument_errors():
    gen = Generator(*SHAPE, SPACING, backend="numpy")
    s = np.zeros((3,) + SHAPE)
    s[0] = 0.2 * SPACING
    gen.set_particle_displacements(s)
    gen.paint_particles(interlaced=True)
    gen.measure_power_spectrum(source="kspace")
    with pytest.raises(ValueError, match="field"):
        gen.measure_power_spectrum(np.zeros(SHAPE), source="kspace")
    with pytest.raises(ValueError, match="field"):
        gen.measure_power_multipoles(np.zeros(SHAPE), source="kspace")
    with pytest.raises(ValueError, match="source"):
        gen.measure_power_spectrum(source="stash")
    gen.measure_power_multipoles(source="kspace")                # the errors above changed nothing
    gen.paint_particles()                                        # a plain paint replaces the interlaced field: its spectrum goes too
    with pytest.raises(RuntimeError, match="interlaced"):
        gen.measure_power_multipoles(source="kspace")
    gen.paint_particles(interlaced=True)
    gen.generate_delta_field(seed=1)
    with pytest.raises(RuntimeError, match="interlaced"):
        gen.measure_power_spectrum(source="kspace")
    # a measurement of the field replaces it too, as on the hip backend (where generic plans transform into the k buffer)
    for measure in (gen.measure_power_spectrum, lambda: gen.measure_power_multipoles(window="cic")):
        gen.set_particle_displacements(s)                        # (a new field dropped them)
        gen.paint_particles(interlaced=True)
        gen.measure_power_spectrum(source="kspace")
        measure()
        with pytest.raises(RuntimeError, match="interlaced"):
            gen.measure_power_spectrum(source="kspace")
