"""The table, references and bounds of tests/epilogue_matrix.py through the CPU emulator: the z pass's stores that do arithmetic
(LognormalRowIO, ScaleZRowIO) at every row length and the accumulating y pass (AccColIO) at every column length in both regimes --
the counterpart of tests/test_gpu_epilogue_matrix.py.  The input of a case is a unit normal half spectrum, symmetrised (DC 0: the
Parseval sum is the variance); the plain field is the emulator's own c2r of it.

And exp_scaled64 by itself (rf_fft_row.h: a 64-entry table, a degree-4 polynomial, ldexp by k >> 6 with k negative half the time)
over its whole finite range against np.longdouble: relative error <= 5e-14 -- the documented 4e-14 (first dropped term) + 1 ulp,
3.92e-14 measured at t = -63482.5 -- on rf_exp2_tab and on the copy LognormalRowIO<double, 1> stages into its tile's pad slots."""
import numpy as np
import pytest

import emu_util
import epilogue_matrix as em


def test_the_table_covers_every_instantiation():
    em.coverage_guard(em.CASES)
    with pytest.raises(AssertionError):
        em.coverage_guard(em.CASES[1:])                 # a row length less
    with pytest.raises(AssertionError):
        em.coverage_guard(em.CASES[:-1])                # a column length less


def _lognormal(ks, delta, dtype, shape, n, with_density=True):
    growth, density = em.sweep_tables(delta, dtype, n, with_density)
    rho, sigma, s1, s2 = emu_util.c2r_lognormal(ks, growth, density)
    what = "lognormal" if with_density else "lognormal, no density"
    em.check_lognormal(what, rho, sigma, s1 / rho.size, s2 / rho.size, delta, growth, density, dtype, shape)


@pytest.mark.parametrize("axis,n", em.CASES, ids=em.case_id)
def test_lognormal_store_and_accumulating_y_pass(axis, n):
    for i, (shape, dtype) in enumerate(em.plans(axis, n)):
        ks = em.am.half_spectra(shape, dtype, n)[0]
        delta = emu_util.c2r(ks)[0]
        _lognormal(ks, delta, dtype, shape, n)
        if (axis, n) == em.NO_DENSITY_CASE and shape == em.plans(axis, n)[0][0]:
            _lognormal(ks, delta, dtype, shape, n, with_density=False)


@pytest.mark.parametrize("axis,n", em.Z_CASES, ids=em.case_id)
def test_per_z_factor_store(axis, n):
    for shape, dtype in em.plans(axis, n):
        ks = em.am.half_spectra(shape, dtype, n)[0]
        plain = emu_util.c2r(ks)[0]
        fz = em.factor_z(shape[2], n)
        got, s1, s2 = emu_util.c2r_zscale(ks, fz)
        em.check_zscale("per-z factor", got, s1 / got.size, s2 / got.size, plain, fz, dtype, shape)


# ---- exp_scaled64 on the host -------------------------------------------------------------------------------------------------------
UNIT = np.longdouble(np.log(np.longdouble(2))) / 64        # an argument t stands for exp(t ln2 / 64)
EXP_BOUND = 5e-14


def _exp_arguments():
    rng = np.random.RandomState(64)
    lo, hi = -708.0 * 64 / np.log(2.0), 709.0 * 64 / np.log(2.0)
    k = np.arange(-65000, 65001, dtype=np.float64)
    tie = k + 0.5                                          # the tie of rint; its neighbours sit where |f| is largest
    return np.concatenate([rng.uniform(lo, hi, 10 ** 6), k, tie, np.nextafter(tie, -np.inf), np.nextafter(tie, np.inf)])


@pytest.mark.parametrize("stride", [1, 18])
def test_exp_scaled64_over_its_finite_range(stride):
    t = _exp_arguments()
    assert t.size == 10 ** 6 + 4 * 130001
    ref = np.exp(t.astype(np.longdouble) * UNIT)
    assert np.all(np.isfinite(ref.astype(np.float64))) and float(ref.min()) >= np.finfo(np.float64).tiny
    got = emu_util.exp_scaled64(t, stride)
    err = np.abs(got.astype(np.longdouble) - ref) / ref
    assert err.size == t.size and np.all(np.isfinite(got))
    i = int(np.argmax(err))
    print("exp_scaled64<%d>: worst relative error %.3e at t = %r, measured / bound = %.3g" % (stride, float(err[i]), float(t[i]), float(err[i]) / EXP_BOUND))
    em.WORST[("exp_scaled64<%d>" % stride, "c128")] = (float(err[i]) / EXP_BOUND, float(t[i]))
    assert float(err[i]) <= EXP_BOUND, "exp_scaled64<%d>(%r): relative error %.3e" % (stride, float(t[i]), float(err[i]))


@pytest.mark.parametrize("stride", [1, 18])
def test_exp_scaled64_outside_its_range(stride):
    big = np.array([1e6, 1e7, 1e9, 1e10, 1e19, 1e100, 1e300])
    assert np.all(emu_util.exp_scaled64(big, stride) == np.inf)
    small = emu_util.exp_scaled64(-big, stride)
    assert np.all(small == 0.0) and not np.any(np.signbit(small))
    assert np.all(np.isnan(emu_util.exp_scaled64(np.array([np.nan, -np.nan]), stride)))
    # rint(+-inf) = +-inf and f = inf - inf: NaN, where libm's exp gives inf / 0 (rf_fft_row.h says so above exp_scaled64)
    assert np.all(np.isnan(emu_util.exp_scaled64(np.array([np.inf, -np.inf]), stride)))
