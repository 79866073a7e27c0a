"""Shared by tests/test_power_measure.py and tests/test_gpu_power_measure.py: an independent float64 numpy oracle of the binned power
spectrum estimator (csrc/rf_core.h power_cell), random Hermitian half spectra, and the statistical check against the input table.

The oracle shares no estimator code with powertools.bin_power: only the per-axis k^2 tables (the plan's input) are common; its weights
come from an index comparison, its bins from searchsorted on the squared edges and its sums from np.bincount."""
import numpy as np

C64, C128 = np.complex64, np.complex128
RTOL = 1e-9         # sums of non-negative float64 terms: the summation error is <= n 2^-53 < 2e-11 for the <= 1e5 ... 1e6 cells used here


def ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else ("c64" if v == C64 else "c128")


def k2_grid(shape, spacing):
    """k^2 of every cell from the per-axis tables the plan is given (powertools.ksq_axes -- the estimator's INPUT: the bin decision is
    exact only on the same float64 tables), summed in the definition's order"""
    from randomfield_amd import powertools
    kx2, ky2, kz2 = powertools.ksq_axes(*shape, spacing)
    return (kx2[:, None, None] + ky2[None, :, None]) + kz2[None, None, :]


def weights(shape):
    nx, ny, nz = shape
    iz = np.arange(nz // 2 + 1)
    wz = np.where((iz == 0) | (iz == nz // 2), 1, 2)
    return np.broadcast_to(wz[None, None, :], (nx, ny, nz // 2 + 1)).copy()


def oracle(kdata, shape, spacing, edges, k2=None):
    """(count, sum_k, sum_p, dropped weight) of the definition, in float64"""
    edges = np.asarray(edges, np.float64)
    nbins = len(edges) - 1
    k2 = (k2_grid(shape, spacing) if k2 is None else k2).ravel()
    w = weights(shape).ravel()
    b = np.searchsorted(edges * edges, k2, "right") - 1
    ok = (b >= 0) & (b < nbins)
    ok[0] = False
    p = kdata.real.astype(np.float64).ravel() ** 2 + kdata.imag.astype(np.float64).ravel() ** 2
    count = np.bincount(b[ok], weights=w[ok], minlength=nbins)
    assert np.all(count == np.round(count))
    sum_k = np.bincount(b[ok], weights=(w * np.sqrt(k2))[ok], minlength=nbins)
    sum_p = np.bincount(b[ok], weights=(w * p)[ok], minlength=nbins)
    dropped = int(w[~ok].sum()) - int(w[0])
    return count.astype(np.uint64), sum_k, sum_p, dropped


def spectrum(shape, dtype, seed=11):
    """a random half spectrum whose planes kz = 0 and nz/2 are Hermitian in (kx, ky), as a forward transform of a real field gives"""
    nx, ny, nz = shape
    rng = np.random.RandomState(seed)
    data = (rng.normal(size=(nx, ny, nz // 2 + 1)) + 1j * rng.normal(size=(nx, ny, nz // 2 + 1))) * rng.uniform(0.1, 3.0, size=(nx, ny, nz // 2 + 1))
    for kz in (0, nz // 2):
        plane = data[:, :, kz]
        mirror = np.conj(np.roll(plane[::-1, ::-1], (1, 1), axis=(0, 1)))
        data[:, :, kz] = 0.5 * (plane + mirror)
    return np.ascontiguousarray(data.astype(dtype))


def pack(kdata):
    """the packed array [nx][ny][nz/2] the tiled forward passes leave: slot kz = 0 holds A0 + i A_nyq (the inverse of the unpack formula)"""
    nzc = kdata.shape[2] - 1
    W = np.ascontiguousarray(kdata[:, :, :nzc]).copy()
    W[:, :, 0] = (kdata[:, :, 0] + 1j * kdata[:, :, nzc]).astype(kdata.dtype)
    return W


def unpack(W):
    """unpack_kspace_kernel's formula in the array's own precision: what the packed sweep must see"""
    nx, ny, nzc = W.shape
    rt = W.real.dtype.type
    K = np.empty((nx, ny, nzc + 1), W.dtype)
    K[:, :, :nzc] = W
    a = W[:, :, 0]
    b = np.roll(a[::-1, ::-1], (1, 1), axis=(0, 1))
    K[:, :, 0].real = rt(0.5) * (a.real + b.real)
    K[:, :, 0].imag = rt(0.5) * (a.imag - b.imag)
    K[:, :, nzc].real = rt(0.5) * (a.imag + b.imag)
    K[:, :, nzc].imag = rt(0.5) * (b.real - a.real)
    return K


def assert_sums(got, want, what=""):
    count, sum_k, sum_p = got
    assert count.dtype == np.uint64 and np.array_equal(count, want[0]), what + ": counts differ"
    for name, g, w in (("sum_k", sum_k, want[1]), ("sum_p", sum_p, want[2])):
        nz = w != 0
        err = float(np.max(np.abs(g[nz] - w[nz]) / w[nz])) if nz.any() else 0.0
        print("%s %s: max relative difference %.3e" % (what, name, err))
        assert np.all(g[~nz] == 0), what + ": " + name + " not zero in an empty bin"
        assert err <= RTOL, what + ": " + name


def table_power_in_bins(power, shape, spacing, edges):
    """the input table's P -- sigma interpolated linearly in log10 k as the generator interpolates it, squared -- averaged with the
    weights w over each bin's modes"""
    k2 = k2_grid(shape, spacing).ravel()
    w = weights(shape).ravel().astype(np.float64)
    nbins = len(edges) - 1
    b = np.searchsorted(np.asarray(edges) ** 2, k2, "right") - 1
    ok = (b >= 0) & (b < nbins)
    ok[0] = False
    p = np.interp(0.5 * np.log10(k2[ok]), np.log10(power["k"]), np.sqrt(power["Pk"])) ** 2
    num = np.bincount(b[ok], weights=w[ok] * p, minlength=nbins)
    den = np.bincount(b[ok], weights=w[ok], minlength=nbins)
    with np.errstate(invalid="ignore", divide="ignore"):
        return num / den


def assert_matches_table(result, power, shape, spacing, edges, what=""):
    """every bin with nmodes >= 100 within 5 sqrt(2 / nmodes) of the table: |delta(k)|^2 of a mode is exponentially distributed and
    nmodes / 2 modes are independent, so the relative scatter of a bin is sqrt(2 / nmodes)"""
    want = table_power_in_bins(power, shape, spacing, edges)
    big = result["nmodes"] >= 100
    assert big.sum() >= 8, what + ": too few populated bins to mean anything"
    units = np.abs(result["Pk"][big] / want[big] - 1.0) / np.sqrt(2.0 / result["nmodes"][big].astype(np.float64))
    print("%s: max deviation %.2f sigma over %d bins" % (what, units.max(), big.sum()))
    assert np.all(units <= 5.0), what
