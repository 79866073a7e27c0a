"""Shared by tests/test_bispectrum_host.py and tests/test_gpu_bispectrum.py: float64 numpy oracles of the binned bispectrum estimator
(rf_measure_bispectrum; csrc/rf_core.h shell_cell, bispectrum_add), by two routes that share nothing but the shell of a cell.

FFT oracle: the half spectrum masked by np.searchsorted(e2, k2, 'right') - 1 with the DC cell dropped, np.fft.irfftn, products summed
exactly (math.fsum) or in np.longdouble.  Explicit oracle: the O(N^2) sum of delta(k1) delta(k2) delta(k3) over all ordered pairs of
modes with k3 = -(k1 + k2) modulo the grid, for grids of at most 1024 cells (the counts alone up to 4096).  N^2 s_FFT = the explicit sum; N^2 s_unit = the count.

Only the per-axis k^2 tables (the plan's input: the bin decision is exact only on the same float64 tables) are taken from the package."""
import math

import numpy as np

import power_oracle as po

C64, C128 = np.complex64, np.complex128
FSUM_LIMIT = 3 * 10 ** 7         # terms up to which the sums go through math.fsum (exact); np.longdouble above


def shells(shape, spacing, edges):
    """the shell of every cell of the half spectrum [nx][ny][nz/2 + 1], -1 = none (the DC cell, cells outside all bins)"""
    edges = np.asarray(edges, np.float64)
    k2 = po.k2_grid(shape, spacing)
    b = np.searchsorted(edges * edges, k2.ravel(), "right") - 1
    b[(b < 0) | (b >= len(edges) - 1)] = -1
    b[0] = -1
    return b.reshape(k2.shape)


def amplitude(shape, amp):
    """(ax[ix] ay[iy]) az[iz] in float64, None tables = ones"""
    one = np.ones(1)
    ax, ay, az = (one if t is None else np.asarray(t, np.float64) for t in (amp if amp is not None else (None, None, None)))
    return (ax[:, None, None] * ay[None, :, None]) * az[None, None, :]


def masked(kdata, sh, shell, amp=None, unit=False):
    """the definition's restricted cell in the array's own type: kept cells bit for bit (no tables), the float64 product rounded once
    per component (tables), 1 (unit); dropped cells 0"""
    keep = sh == shell
    out = np.zeros(kdata.shape, kdata.dtype)
    if unit:
        out[keep] = 1.0
    elif amp is None:
        out[keep] = kdata[keep]
    else:
        a = np.broadcast_to(amplitude(None, amp), kdata.shape)
        out.real[keep] = (a * kdata.real.astype(np.float64))[keep]
        out.imag[keep] = (a * kdata.imag.astype(np.float64))[keep]
    return out


def shell_fields(kdata, shape, spacing, edges, amp=None, unit=False):
    """D_b for every bin: float64 irfftn (1/N) of the masked spectrum, the mask applied to the array as the device was given it"""
    sh = shells(shape, spacing, edges)
    return [np.fft.irfftn(masked(kdata, sh, b, amp, unit).astype(C128), s=shape, axes=(0, 1, 2)) for b in range(len(edges) - 1)]


def triple_sums(fields, triples):
    """(sum, sum of |term|) per triple over dense real fields of any real type: every term ((double)D1 (double)D2) (double)D3 as the
    device forms it, the terms summed exactly (math.fsum) or in np.longdouble"""
    f = [np.asarray(a, np.float64).ravel() for a in fields]
    exact = len(triples) * f[0].size <= FSUM_LIMIT
    s, sa = np.empty(len(triples), np.float64), np.empty(len(triples), np.float64)
    for i, (b1, b2, b3) in enumerate(np.asarray(triples).reshape(-1, 3)):
        term = (f[b1] * f[b2]) * f[b3]
        if exact:
            s[i], sa[i] = math.fsum(term), math.fsum(np.abs(term))
        else:
            s[i], sa[i] = float(np.sum(term.astype(np.longdouble))), float(np.sum(np.abs(term).astype(np.longdouble)))
    return s, sa


def reduction_bound(cells, abs_sums):
    """what a float64 sum of `cells` terms in any order may differ from the exact sum of the same terms by: (cells - 1) roundings of
    partial sums no larger than sum |term|, each 2^-53 relative -- taken four times over"""
    return 4.0 * cells * 2.0 ** -53 * np.asarray(abs_sums)


def fft_oracle(kdata, shape, spacing, edges, triples, amp=None, unit=False):
    """s(b1, b2, b3) by the FFT route"""
    return triple_sums(shell_fields(kdata, shape, spacing, edges, amp, unit), triples)[0]


def full_spectrum(kdata, shape):
    """all nx ny nz modes from the half spectrum: delta(-k) = conj delta(k)"""
    nx, ny, nz = shape
    full = np.empty(shape, C128)
    full[:, :, :nz // 2 + 1] = kdata
    ix, iy = (-np.arange(nx)) % nx, (-np.arange(ny)) % ny
    for iz in range(nz // 2 + 1, nz):
        full[:, :, iz] = np.conj(kdata[ix][:, iy][:, :, nz - iz])
    return full


def full_shells(shape, spacing, edges):
    nx, ny, nz = shape
    half = shells(shape, spacing, edges)
    sh = np.empty(shape, half.dtype)
    sh[:, :, :nz // 2 + 1] = half
    for iz in range(nz // 2 + 1, nz):          # (k^2 is even in every component: the tables of a k grid)
        sh[:, :, iz] = half[:, :, nz - iz]
    return sh


def explicit_oracle(kdata, shape, spacing, edges, triples, unit=False, exact=False):
    """(sums, counts): per triple the sum of delta(k1) delta(k2) delta(k3) over ordered triangles k_i in shell b_i, k1 + k2 + k3 = 0
    modulo the grid, and their number.  sums = N^2 s.  exact: only the triangles whose signed mode numbers (in [-n/2, n/2)) sum to
    zero as integers -- the others close through aliasing alone."""
    nx, ny, nz = shape
    assert nx * ny * nz <= (4096 if unit else 1024), "the explicit sum is O(N^2) (counts alone: integer work, up to 16^3)"
    sh = full_shells(shape, spacing, edges).ravel()
    d = np.ones(nx * ny * nz, C128) if unit else full_spectrum(np.asarray(kdata, C128), shape).ravel()
    ix, iy, iz = (a.ravel() for a in np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"))
    triples = np.asarray(triples).reshape(-1, 3)
    sums, counts = np.zeros(len(triples), np.float64), np.zeros(len(triples), np.int64)
    cache = {}
    for t, (b1, b2, b3) in enumerate(triples):
        if (b1, b2) not in cache:
            i1, i2 = np.nonzero(sh == b1)[0], np.nonzero(sh == b2)[0]
            j3 = ((((-(ix[i1][:, None] + ix[i2][None, :])) % nx) * ny + (-(iy[i1][:, None] + iy[i2][None, :])) % ny) * nz
                  + (-(iz[i1][:, None] + iz[i2][None, :])) % nz)
            s3 = sh[j3]
            if exact:
                sx, sy, sz = ((a + n // 2) % n - n // 2 for a, n in ((ix, nx), (iy, ny), (iz, nz)))
                aliased = ((sx[i1][:, None] + sx[i2][None, :] + sx[j3] != 0) | (sy[i1][:, None] + sy[i2][None, :] + sy[j3] != 0)
                           | (sz[i1][:, None] + sz[i2][None, :] + sz[j3] != 0))
                s3 = np.where(aliased, -2, s3)
            cache = {(b1, b2): (s3, (d[i1][:, None] * d[i2][None, :]) * d[j3])}
        s3, prod = cache[(b1, b2)]
        hit = s3 == b3
        counts[t] = int(hit.sum())
        total = prod[hit]
        sums[t] = math.fsum(total.real)
        assert abs(math.fsum(total.imag)) <= 1e-9 * (1.0 + float(np.abs(total).sum())), "the triangle sum of a real field is real"
    return sums, counts


def symmetric_tables(shape, seed=3):
    """three positive per-axis tables that are even in the mode number, as window tables are: the masked spectrum stays Hermitian"""
    rng = np.random.RandomState(seed)
    nx, ny, nz = shape
    tabs = []
    for n in (nx, ny):
        t = rng.uniform(0.5, 2.0, size=n)
        tabs.append(np.ascontiguousarray(0.5 * (t + t[(-np.arange(n)) % n])))
    tabs.append(rng.uniform(0.5, 2.0, size=nz // 2 + 1))
    return tabs


def plane_waves(shape, modes, amps, phases):
    """sum_i a_i cos(k_i . x + phi_i) with integer mode vectors k_i, float64"""
    grid = np.meshgrid(*[np.arange(n) / float(n) for n in shape], indexing="ij")
    out = np.zeros(shape, np.float64)
    for m, a, p in zip(modes, amps, phases):
        out += a * np.cos(2 * np.pi * sum(mi * g for mi, g in zip(m, grid)) + p)
    return out


def mode_k(shape, spacing, m):
    return 2 * np.pi / spacing * math.sqrt(sum((mi / float(n)) ** 2 for mi, n in zip(m, shape)))
