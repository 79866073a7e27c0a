"""rf_realise_lognormal and rf_realise_scaled_potential(factor_z) against np.longdouble maps of the plain call's field at EVERY row
length of the z pass, and the accumulating y pass behind the first at every column length in both tile-addressing regimes -- run
with -m gpu on an MI355X.

row_c2r_kernel<C, LognormalIO> and <C, ScaleZRowIO> are GPU instantiations of their own at each of the eight row lengths and two
dtypes (one-pass rows store cell by cell, multi-pass rows through Pre<R> / store_row; float64 rows of >= 512 complex keep the exp
table in the tile's LDS pad slots), and col_kernel<C, +1, AccColIO> at each of the nine column lengths; the other tests reach a
handful of them, with exp arguments below 7.  Table, tables that sweep the argument to 40 / 60, guards, references and bounds are
tests/epilogue_matrix.py's; tests/test_emulator_epilogue_matrix.py puts the same table through the CPU emulator, so a case that
fails here and passes there is a fault of the GPU build or launch, not of the phase functions -- as the first run of this file
found: sigma = 0 on plans with ny = 8 or 16, whose accumulating pass was launched without the LDS its wave sums go through
(rf_tile_launch.h lds_of; CHANGES.md)."""
import pytest

import epilogue_matrix as em
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

# every (dtype, M) of RF_ROW_SIZES for both z IOs, every (dtype, N) of RF_COL_SIZES in both regimes of the accumulating pass
em.coverage_guard(em.CASES)
assert [c for c in em.CASES if c[0] == "z"] == em.Z_CASES and len(em.Z_CASES) == len(em.header_sizes("RF_ROW_SIZES"))

SPACING = 2.5
SCALE = -2.5e-3
RESIDENT_CASE = (("z", 256), (32, 16, 256))     # float32 plan: the per-z factor once from resident float32 deviates too


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


def make_plan(hip, shape, dtype, power):
    from randomfield_amd import powertools
    plan = hip.DevicePlan(*shape, dtype)
    assert plan.tiled
    plan.set_kgrid(*powertools.ksq_axes(*shape, SPACING))
    plan.set_power(*cpu_ref.sigma_table(power["k"], power["Pk"], *shape, SPACING))
    return plan


def _lognormal(plan, what, shape, dtype, n, seed, noise, with_density=True):
    plan.realise(seed=seed, noise=noise)
    delta = plan.download_real()
    growth, density = em.sweep_tables(delta, dtype, n, with_density)
    plan.set_z_tables(growth, density)
    sigma = plan.realise_lognormal(seed=seed, noise=noise)
    rho = plan.download_real()
    mean, std = plan.moments()
    em.check_lognormal(what, rho, sigma, mean, std * std + mean * mean, delta, growth, density, dtype, shape)


@pytest.mark.parametrize("axis,n", em.CASES, ids=em.case_id)
def test_lognormal_store_and_accumulating_y_pass(hip, default_power, axis, n):
    first = em.plans(axis, n)[0][0]
    for shape, dtype in em.plans(axis, n):
        nx, ny, nz = shape
        plan = make_plan(hip, shape, dtype, default_power)
        noise = cpu_ref.reference_noise(n, nx * ny * (nz // 2 + 1))
        _lognormal(plan, "lognormal", shape, dtype, n, 0, noise)
        if axis == "z":
            _lognormal(plan, "lognormal, native", shape, dtype, n, 21 + n, None)
        if (axis, n) == em.NO_DENSITY_CASE and shape == first:
            _lognormal(plan, "lognormal, no density", shape, dtype, n, 0, noise, with_density=False)
        plan.close()


@pytest.mark.parametrize("axis,n", em.Z_CASES, ids=em.case_id)
def test_per_z_factor_store(hip, default_power, axis, n):
    for shape, dtype in em.plans(axis, n):
        plan = make_plan(hip, shape, dtype, default_power)
        fz = em.factor_z(shape[2], n)
        resident = dtype == em.C64 and ((axis, n), shape) == RESIDENT_CASE
        for noise in (None, "resident") if resident else (None,):
            if noise is not None:
                plan.reference_noise(99, single=True)          # the replayed stream resident as float32 pairs
            assert plan.can_regenerate_potential(noise)
            plan.realise_scaled_potential(seed=77 + n, noise=noise, scale=SCALE)
            plain = plan.download_real()
            plan.realise_scaled_potential(seed=77 + n, noise=noise, scale=SCALE, factor_z=fz)
            got = plan.download_real()
            mean, std = plan.moments()
            what = "per-z factor" if noise is None else "per-z factor, resident"
            em.check_zscale(what, got, mean, std * std + mean * mean, plain, fz, dtype, shape)
        plan.close()
