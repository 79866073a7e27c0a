"""The triangular-shaped cloud on the CPU: the weight table, the numpy backend (randomfield_amd/particles.py order=3,
Generator(backend='numpy') assignment='tsc') against tests/tsc_oracle.py.  Everything here is fixed by the definitions of DESIGN.md
section 3.18 -- integer weights, float64 steps rounded one by one -- so the comparisons are exact."""
import numpy as np
import pytest

import cic_oracle as corc
import gather_oracle as gorc
import tsc_oracle as orc

SPACING = 0.5            # a power of two: whole and half cells are exact in float32
INV_H = [1.0 / SPACING] * 3
REALS = [np.float32, np.float64]
COEFF = 0.3


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else np.dtype(v).name


def all_sets(shape, rt):
    sets = dict(orc.displacement_sets(shape, SPACING))
    sets.update(orc.extra_sets(shape, SPACING))
    return {name: s.astype(rt) for name, s in sets.items()}


def test_weight_table_over_every_t():
    from randomfield_amd import particles
    t = np.arange(65537, dtype=np.int64)
    tau = np.where(t >= 32768, t - 32768, t + 32768)
    table = np.array([orc.weights(int(v)) for v in t], np.int64)
    wm, w0, wp = table.T
    assert np.all(wm + w0 + wp == 65536)
    assert table.min() >= 0 and table.max() <= 49153
    assert np.all(wp - wm == tau - 32768)
    # Wm(tau) = Wp(65536 - tau): by tau, for tau in [1, 65535]
    by_tau = np.empty((65536, 3), np.int64)
    by_tau[tau[:65536]] = table[:65536]
    assert np.array_equal(by_tau[1:, 0], by_tau[:0:-1, 2])
    assert by_tau[0].tolist() == [32768, 32768, 0] and orc.weights(65536) == orc.weights(0)
    assert np.all(by_tau[:363, 2] == 0) and by_tau[363, 2] == 1
    # within 1 (Wm, Wp) and 2 (W0) units of the parabola
    s = np.arange(65536) / 65536.0
    assert np.all(np.abs(by_tau[:, 0] - 0.5 * (1 - s) ** 2 * 65536) <= 1) and np.all(np.abs(by_tau[:, 2] - 0.5 * s * s * 65536) <= 1)
    assert np.all(np.abs(by_tau[:, 1] - (0.5 + s - s * s) * 65536) <= 2)
    # the package's table: a row of particles on one axis, t = k for the particle displaced by k / 65536 of a cell
    disp = np.zeros((3, 2, 2, 65536))
    disp[2] = (np.arange(65536) / 65536.0)[None, None, :]
    _, _, w = particles._axis_tsc(disp[2], 1.0, 2)
    assert np.array_equal(np.stack([np.asarray(v)[0, 0] for v in w], 1).astype(np.int64), table[:65536])


@pytest.mark.parametrize("rt", REALS, ids=_ids)
@pytest.mark.parametrize("shape", [(4, 6, 8), (2, 2, 2), (10, 12, 70)], ids=_ids)
def test_numpy_backend_equals_the_oracle(shape, rt):
    from randomfield_amd import particles
    rng = np.random.RandomState(sum(shape))
    W = rng.normal(size=shape).astype(rt)
    G0 = rng.normal(size=shape).astype(rt)
    for name, s in all_sets(shape, rt).items():
        A, dropped = particles.paint_counts(s, INV_H, order=3)
        want, wdrop = orc.paint(s, INV_H)
        assert A.dtype == np.uint64 and dropped == wdrop == 0 and np.array_equal(A, want), name
        assert orc.total(A) == s[0].size * orc.ONE, name
        out, dropped = particles.gather(s, INV_H, W, order=3)
        assert out.dtype == rt and np.array_equal(out, orc.gather(s, INV_H, W)[0]), name
        out, _ = particles.gather(s, INV_H, W, COEFF, False, G0.copy(), order=3)
        assert np.array_equal(out, orc.gather(s, INV_H, W, COEFF, False, G0)[0]), name
        # order 2 is what it was: the default, and equal to the cloud-in-cell oracles
        A2, _ = particles.paint_counts(s, INV_H)
        assert np.array_equal(A2, particles.paint_counts(s, INV_H, order=2)[0]) and np.array_equal(A2, corc.paint(s, INV_H)[0]), name
        g2, _ = particles.gather(s, INV_H, W)
        assert np.array_equal(g2, particles.gather(s, INV_H, W, order=2)[0]) and np.array_equal(g2, gorc.gather(s, INV_H, W)[0]), name
    s = all_sets(shape, rt)["rms0.6"].copy()
    s[1][1, 1, 1] = np.nan
    s[2][0, 1, 0] = np.inf
    A, dropped = particles.paint_counts(s, INV_H, order=3)
    want, wdrop = orc.paint(s, INV_H)
    assert dropped == wdrop == 2 and np.array_equal(A, want) and orc.total(A) == (s[0].size - 2) * orc.ONE
    out, dropped = particles.gather(s, INV_H, W, order=3)
    assert dropped == 2 and np.array_equal(out, orc.gather(s, INV_H, W)[0]) and out[1, 1, 1] == 0
    out, _ = particles.gather(s, INV_H, W, COEFF, False, G0.copy(), order=3)
    assert np.array_equal(out, orc.gather(s, INV_H, W, COEFF, False, G0)[0]) and out[1, 1, 1] == G0[1, 1, 1]
    with pytest.raises(ValueError, match="order"):
        particles.paint_counts(s, INV_H, order=4)
    with pytest.raises(ValueError, match="order"):
        particles.gather(s, INV_H, W, order=1)


def test_uniform_displacements_paint_one_particle_per_cell():
    from randomfield_amd import particles
    shape = (6, 4, 10)
    for cells in (0.0, 3.0, -2.5):
        s = np.full((3,) + shape, cells * SPACING)
        A, dropped = particles.paint_counts(s, INV_H, order=3)
        assert dropped == 0 and np.all(A == np.uint64(orc.ONE)), cells


def test_linear_field_is_interpolated_to_the_weight_quantum():
    """W = iz: away from the wrap the first moment of the weights is the quantised position (Wp - Wm = tau - 32768 exactly), so the
    gathered value is iz + floor(u_z 65536) / 65536: below iz + u_z by less than 2^-16"""
    from randomfield_amd import particles
    shape = (4, 6, 32)
    W = np.broadcast_to(np.arange(shape[2], dtype=np.float64), shape).copy()
    s = orc.extra_sets(shape, SPACING)["rms0.6"] * 3.0
    g, dropped = particles.gather(s, INV_H, W, order=3)
    lo = np.arange(shape[2])[None, None, :] + orc.axis_terms(s[2], INV_H[2], 2)[3]        # the lowest of the three cells, unwrapped
    inside = (lo >= 0) & (lo + 2 <= shape[2] - 1)                                         # neither the cells nor the particle wrap
    assert dropped == 0 and 0 < np.count_nonzero(inside) < inside.size
    exact = np.arange(shape[2], dtype=np.float64)[None, None, :] + s[2] * INV_H[2]
    assert np.all(np.abs(exact - g)[inside] < 2.0 ** -16)


@pytest.mark.parametrize("dtype", [np.complex64, np.complex128], ids=_ids)
def test_numpy_generator_round_trip(dtype):
    from randomfield_amd import Generator
    shape = (16, 16, 16)
    rt = np.float32 if dtype == np.complex64 else np.float64
    gen = Generator(*shape, SPACING, backend="numpy", dtype=dtype)
    field = gen.generate_delta_field(seed=11, save_potential=True).copy()
    s = orc.extra_sets(shape, SPACING)["rms0.6"].astype(rt)
    s[0][3, 4, 5] = np.nan
    gen.set_particle_displacements(s)
    painted = gen.paint_particles(assignment="tsc").copy()
    A, wdrop = orc.paint(s, INV_H)
    assert painted.dtype == rt and np.array_equal(painted, orc.delta(A, rt)) and gen.particles_dropped == 1 == wdrop
    assert not np.array_equal(painted, gen.paint_particles().copy())                 # the default is cloud in cell, as before
    assert np.array_equal(gen.paint_particles(assignment="cic"), corc.delta(corc.paint(s, INV_H)[0], rt))
    res = gen.measure_power_spectrum(gen.paint_particles(assignment="tsc").copy(), window="tsc")
    assert res is not None
    got = gen.interpolate_at_particles(field, slot=1, coeff=COEFF, assignment="tsc")
    assert np.array_equal(got, orc.gather(s, INV_H, field, COEFF)[0]) and gen.particles_dropped == 1
    got2 = gen.interpolate_at_particles(slot=1, coeff=-1.5, first=False, assignment="tsc")
    assert np.array_equal(got2, orc.gather(s, INV_H, field, -1.5, False, got)[0])
    assert np.array_equal(gen.interpolate_at_particles(field), gorc.gather(s, INV_H, field)[0])
    for call in (lambda: gen.paint_particles(assignment="pcs"), lambda: gen.interpolate_at_particles(assignment="ngp"),
                 lambda: gen.paint_particles(assignment=3)):
        with pytest.raises(ValueError, match="assignment"):
            call()
