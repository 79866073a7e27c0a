"""Shared by tests/test_power_multipoles.py and tests/test_gpu_power_multipoles.py: an independent float64 numpy oracle of the power
spectrum multipole estimator (csrc/rf_core.h multipole_cell), a brute-force sum over the full cube, random compensation tables.

The oracle shares no estimator code with powertools.bin_multipoles: only the per-axis k^2 tables (the plan's input) are common.  Bins
and weights are tests/power_oracle.py's (index comparison, searchsorted on the squared edges); mu^2 is formed per cell from the
line-of-sight table, the compensation as an outer product, the sums with np.bincount."""
import numpy as np

import power_oracle as po

RTOL = po.RTOL      # sums of non-negative float64 terms, a handful of roundings per term: n 2^-53 << 1e-9 for the < 1e6 cells used here
NAMES = ("sum_k", "m0", "m2", "m4")


def axis_tables(shape, spacing):
    from randomfield_amd import powertools
    return powertools.ksq_axes(*shape, spacing)


def mu2_grid(shape, spacing, los):
    """k_los^2 / k^2 of every cell of the half spectrum (0 at DC, which is dropped anyway)"""
    tabs = axis_tables(shape, spacing)
    k2 = po.k2_grid(shape, spacing)
    sel = [None, None, None]
    sel[los] = slice(None)
    klos2 = np.broadcast_to(tabs[los][tuple(sel)], k2.shape)
    out = np.zeros(k2.shape)
    np.divide(klos2, k2, out=out, where=k2 > 0)
    return out


def comp_grid(shape, comp):
    nx, ny, nz = shape
    grid = np.ones((nx, ny, nz // 2 + 1))
    if comp is None:
        return None
    cx, cy, cz = comp
    if cx is not None:
        grid = grid * np.asarray(cx, np.float64)[:, None, None]
    if cy is not None:
        grid = grid * np.asarray(cy, np.float64)[None, :, None]
    if cz is not None:
        grid = grid * np.asarray(cz, np.float64)[None, None, :]
    return grid


def oracle(kdata, shape, spacing, edges, los, comp=None):
    """(count, sum_k, m0, m2, m4, dropped weight) of the definition, in float64"""
    edges = np.asarray(edges, np.float64)
    nbins = len(edges) - 1
    k2 = po.k2_grid(shape, spacing).ravel()
    w = po.weights(shape).ravel()
    b = np.searchsorted(edges * edges, k2, "right") - 1
    ok = (b >= 0) & (b < nbins)
    ok[0] = False
    e = kdata.real.astype(np.float64).ravel() ** 2 + kdata.imag.astype(np.float64).ravel() ** 2
    c = comp_grid(shape, comp)
    if c is not None:
        e = c.ravel() * e
    mu2 = mu2_grid(shape, spacing, los).ravel()
    count = np.bincount(b[ok], weights=w[ok], minlength=nbins)
    assert np.all(count == np.round(count))
    sum_k = np.bincount(b[ok], weights=(w * np.sqrt(k2))[ok], minlength=nbins)
    m0 = np.bincount(b[ok], weights=(w * e)[ok], minlength=nbins)
    m2 = np.bincount(b[ok], weights=(w * e * mu2)[ok], minlength=nbins)
    m4 = np.bincount(b[ok], weights=(w * e * mu2 * mu2)[ok], minlength=nbins)
    dropped = int(w[~ok].sum()) - int(w[0])
    return count.astype(np.uint64), sum_k, m0, m2, m4, dropped


def full_cube(field, spacing, edges, los):
    """(m0, m2, m4) summed over the FULL cube np.fft.fftn(field), weight 1 per mode: no half-spectrum weights at all"""
    shape = field.shape
    lam = spacing / (2 * np.pi)
    k = [np.fft.fftfreq(n, lam) for n in shape]
    # the same float64 tables (and sum order) as the half spectrum's, so that a mode and its mirror take the same bin
    k2 = (k[0][:, None, None] ** 2 + k[1][None, :, None] ** 2) + k[2][None, None, :] ** 2
    sel = [None, None, None]
    sel[los] = slice(None)
    klos2 = np.broadcast_to((k[los] ** 2)[tuple(sel)], k2.shape)
    mu2 = np.zeros(k2.shape)
    np.divide(klos2, k2, out=mu2, where=k2 > 0)
    edges = np.asarray(edges, np.float64)
    nbins = len(edges) - 1
    b = np.searchsorted(edges * edges, k2.ravel(), "right") - 1
    ok = (b >= 0) & (b < nbins)
    ok[0] = False
    p = (np.abs(np.fft.fftn(field.astype(np.float64))) ** 2).ravel()
    mu2 = mu2.ravel()
    return tuple(np.bincount(b[ok], weights=(p * mu2 ** j)[ok], minlength=nbins) for j in (0, 1, 2))


def random_tables(shape, seed=5):
    """three positive tables drawn uniformly from [0.5, 2]"""
    nx, ny, nz = shape
    rng = np.random.RandomState(seed)
    return tuple(rng.uniform(0.5, 2.0, size=n) for n in (nx, ny, nz // 2 + 1))


def assert_sums(got, want, what=""):
    count = got[0]
    assert count.dtype == np.uint64 and np.array_equal(count, want[0]), what + ": counts differ"
    for name, g, w in zip(NAMES, got[1:5], want[1:5]):
        nz = w != 0
        err = float(np.max(np.abs(g[nz] - w[nz]) / w[nz])) if nz.any() else 0.0
        print("%s %s: max relative difference %.3e" % (what, name, err))
        assert np.all(g[~nz] == 0), what + ": " + name + " not zero in an empty bin"
        assert err <= RTOL, what + ": " + name
