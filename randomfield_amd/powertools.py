"""
Utilities for working with tabulated power spectra -- host-side mirror of
``randomfield/powertools.py`` (file:line citations are to the reference).

These functions operate on host (numpy) arrays exactly like the reference's and
exist so that the free-function API keeps working.  The GPU path does not call
them per cell: :class:`randomfield_amd.generate.Generator` hands the O(n) tables
computed by :func:`ksq_axes` and :func:`sigma_table` to the HIP kernels, which
evaluate rows K and T (|k| and sigma(k)) on the fly inside the first FFT pass.
"""
from __future__ import annotations

import os.path

import numpy as np

from . import transform

__all__ = ["get_k_bounds", "create_ksq_grids", "ksq_axes", "fill_with_log10k", "validate_power", "filter_power",
           "sigma_table", "tabulate_sigmas", "load_default_power", "make_power", "bin_power", "default_k_edges",
           "power_estimate", "bin_multipoles", "multipole_estimate", "window_compensation", "bispectrum_triples",
           "default_bispectrum_edges", "bin_bispectrum", "bispectrum_estimate"]


def grid_k_range(shape, spacing):
    """(k_min, k_max) of an (nx, ny, nz) grid: the fundamental mode of the longest axis and the corner of the
    Nyquist cube (powertools.py:19-23)."""
    fundamental = 2 * np.pi / spacing
    return fundamental / max(shape), fundamental * np.sqrt(3) / 2


def get_k_bounds(data, spacing, packed=True):
    """Bounds of wavenumber values for the specified grid (powertools.py:16-24)."""
    return grid_k_range(transform.expanded_shape(data, packed=packed), spacing)


def ksq_axes(nx, ny, nz, spacing, packed=True):
    """Per-axis float64 tables of k_a(i)**2 (powertools.py:27-34).

    These three O(n) tables are what the HIP kernels consume (``rf_set_kgrid``)."""
    lambda0 = spacing / (2 * np.pi)
    kx = np.fft.fftfreq(nx, lambda0)
    ky = np.fft.fftfreq(ny, lambda0)
    kz = np.fft.fftfreq(nz, lambda0)
    if packed:
        kz = kz[:nz // 2 + 1]
    return kx ** 2, ky ** 2, kz ** 2


def default_k_edges(shape, spacing, nbins=None):
    """``nbins + 1`` linear bin edges in k from ``k_min`` to ``k_max`` of :func:`grid_k_range` (the fundamental mode of the longest
    axis ... the corner of the Nyquist cube); the last edge is nudged up by an ulp so that the corner mode is counted
    (and the first one down where rounding would otherwise lose the fundamental mode).
    ``nbins`` defaults to ``min(shape) // 2``."""
    if nbins is None:
        nbins = min(shape) // 2
    nbins = int(nbins)
    if not 1 <= nbins <= 1024:
        raise ValueError("nbins must be between 1 and 1024.")
    k_min, k_max = grid_k_range(shape, spacing)
    edges = np.linspace(k_min, k_max, nbins + 1)
    # the bin rule compares SQUARES (e * e against the sum of the three k**2 tables): the nudge goes to the first float whose square
    # lies above the corner cell's k**2 as those tables give it -- one ulp above k_max, or a few where the roundings differ
    corner = sum(float(t[n // 2]) for t, n in zip(ksq_axes(*shape, spacing), shape))
    last = np.nextafter(max(edges[-1], k_max, np.sqrt(corner)), np.inf)
    while last * last <= corner:
        last = np.nextafter(last, np.inf)
    edges[-1] = last
    # ... and likewise the first edge may not lie above the fundamental mode of the longest axis as its table gives it
    lowest = min(float(t[1]) for t in ksq_axes(*shape, spacing))
    while edges[0] * edges[0] > lowest:
        edges[0] = np.nextafter(edges[0], 0.0)
    return edges


def bin_power(kdata, spacing, edges):
    """Per-bin sums of the binned power spectrum of a half spectrum -- the numpy statement of the definition the device call
    ``rf_measure_power`` implements (csrc/rf_core.h power_cell).

    ``kdata`` is ``(nx, ny, nz/2 + 1)`` complex, unnormalised forward-transform values delta(k).  Cell (ix, iy, iz) has
    ``k2 = (kx2[ix] + ky2[iy]) + kz2[iz]`` in float64 and the weight w = 1 on the planes iz = 0 and iz = nz/2, 2 elsewhere; it belongs
    to bin b iff ``edges[b]**2 <= k2 < edges[b+1]**2`` (the edges are squared once, no sqrt in the decision).  The DC cell and cells
    outside all bins are dropped.  Returns ``(count, sum_k, sum_p)``: the uint64 sum of w, and the float64 sums of ``w * sqrt(k2)``
    and ``w * |delta(k)|**2`` per bin."""
    edges = np.asarray(edges, np.float64).ravel()
    nbins = len(edges) - 1
    if not 1 <= nbins <= 1024 or edges[0] < 0 or not np.all(np.diff(edges) > 0):
        raise ValueError("edges must be 2 ... 1025 strictly increasing non-negative values.")
    nx, ny, nz = transform.expanded_shape(kdata, packed=True)
    kx2, ky2, kz2 = ksq_axes(nx, ny, nz, spacing)
    k2 = (kx2[:, None, None] + ky2[None, :, None]) + kz2[None, None, :]
    b = np.searchsorted(edges * edges, k2.ravel(), side="right") - 1
    w = np.full(k2.shape, 2, np.int64)
    w[:, :, 0] = 1
    w[:, :, nz // 2] = 1
    w = w.ravel()
    keep = (b >= 0) & (b < nbins)
    keep[0] = False                          # the DC cell
    b, w = b[keep], w[keep]
    re = kdata.real.astype(np.float64).ravel()[keep]
    im = kdata.imag.astype(np.float64).ravel()[keep]
    count = np.bincount(b, weights=w, minlength=nbins).astype(np.uint64)      # (exact: integers far below 2**53)
    sum_k = np.bincount(b, weights=w * np.sqrt(k2.ravel()[keep]), minlength=nbins)
    sum_p = np.bincount(b, weights=w * (re * re + im * im), minlength=nbins)
    return count, sum_k, sum_p


def power_estimate(count, sum_k, sum_p, shape, spacing):
    """The structured array ('k', 'Pk', 'nmodes') of the sums of :func:`bin_power` / ``DevicePlan.measure_power``: with
    N = nx ny nz and V = N spacing**3, ``k = sum_k / count`` and ``Pk = (V / N**2) sum_p / count``; NaN in empty bins."""
    n = float(shape[0]) * float(shape[1]) * float(shape[2])
    out = np.empty(len(count), [("k", float), ("Pk", float), ("nmodes", np.uint64)])
    c = np.asarray(count, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out["k"] = np.where(c > 0, np.asarray(sum_k) / c, np.nan)
        out["Pk"] = np.where(c > 0, (spacing ** 3 / n) * np.asarray(sum_p) / c, np.nan)
    out["nmodes"] = count
    return out


_WINDOW_ORDER = {"ngp": 1, "cic": 2, "tsc": 3}


def window_compensation(shape, scheme):
    """The three per-axis float64 tables ``sinc(pi m / n)**(-2 p)`` (lengths nx, ny, nz/2 + 1) that divide the mass-assignment window
    out of |delta(k)|**2: m the signed frequency index, sinc(0) = 1, p = 1, 2, 3 for ``'ngp'``, ``'cic'``, ``'tsc'``; the entry at
    Nyquist is ``(pi / 2)**(2 p)``.  This is the standard correction for well-mixed particles; on a cold lattice with sub-cell
    displacements the paint is a finite difference of the displacement and the window is not this one."""
    if scheme not in _WINDOW_ORDER:
        raise ValueError("Invalid window scheme: {0!r} (expected 'ngp', 'cic' or 'tsc').".format(scheme))
    p = _WINDOW_ORDER[scheme]
    nx, ny, nz = (int(n) for n in shape)
    tabs = []
    for n, count in ((nx, nx), (ny, ny), (nz, nz // 2 + 1)):
        m = np.rint(np.fft.fftfreq(n) * n)[:count]            # signed index (the Nyquist entry's sign does not matter: sinc is even)
        tabs.append(np.sinc(m / n) ** (-2.0 * p))              # np.sinc(x) = sin(pi x) / (pi x)
    return tuple(tabs)


def interlace_phases(shape):
    """The three per-axis complex128 tables ``p_a[i] = exp(+i pi m / n_a)`` (lengths nx, ny, nz/2 + 1; m the signed mode number of
    index i, from cos / sin of ``pi * m / n`` in float64) that undo the half-cell shift of an interlaced paint's second grid: with the
    particles at u + 1/2 that grid's spectrum is ``exp(-i pi m / n)`` per axis times the unshifted one, so the interlaced field is
    ``(delta1 + p delta2) / 2`` with p = px[ix] py[iy] pz[iz] (``rf_kspace_interlace``; Sefusatti et al. 2016).

    ``p_a[0] = 1`` exactly.  ``p_a[n_a / 2] = 0`` exactly: the Hermitian part of ``exp(+-i pi / 2)``.  That keeps
    ``p(-k) = conj(p(k))``, so the combined spectrum is Hermitian and its inverse transform is the real field; the planes at an axis'
    own Nyquist index therefore hold ``delta1 / 2``.  They lie at |k| >= k_Nyq, beyond what a measurement up to k_Nyq reads."""
    nx, ny, nz = (int(n) for n in shape)
    tabs = []
    for n, count in ((nx, nx), (ny, ny), (nz, nz // 2 + 1)):
        m = np.rint(np.fft.fftfreq(n) * n)[:count]
        arg = np.pi * m / n
        p = np.cos(arg) + 1j * np.sin(arg)
        p[0] = 1.0
        if n % 2 == 0:
            p[n // 2] = 0.0
        tabs.append(p.astype(np.complex128))
    return tuple(tabs)


def interlace_combine(stashed, kdata, tables=None):
    """``(S + p K) / 2`` per cell of two half spectra with p = px[ix] py[iy] pz[iz] -- the numpy statement of the definition the
    device call ``rf_kspace_interlace`` implements (csrc/rf_core.h interlace_cell).  ``tables``: None or three complex per-axis tables
    (each may be None = all ones).  All in float64 on real arrays, one numpy operation per rounding: a = px py
    (ar = xr yr - xi yi, ai = xr yi + xi yr), p = a pz and q = p K in the same form, then 0.5 (S + q) per component, rounded once
    to the type of ``kdata``."""
    S, K = np.asarray(stashed), np.asarray(kdata)
    tabs = [None] * 3 if tables is None else list(tables)
    parts = []
    for a, n in enumerate(K.shape):
        t = np.ones(n, np.complex128) if tabs[a] is None else np.asarray(tabs[a], np.complex128).ravel()
        if len(t) != n:
            raise ValueError("phase table {0} needs {1} entries.".format(a, n))
        index = [None] * 3
        index[a] = slice(None)
        parts.append((np.ascontiguousarray(t.real)[tuple(index)], np.ascontiguousarray(t.imag)[tuple(index)]))

    def mul(xr, xi, yr, yi):
        rr, ii, ri, ir = xr * yr, xi * yi, xr * yi, xi * yr
        return rr - ii, ri + ir
    with np.errstate(invalid="ignore", over="ignore"):
        ar, ai = mul(*parts[0], *parts[1])
        pr, pi = mul(ar, ai, *parts[2])
        qr, qi = mul(pr, pi, K.real.astype(np.float64), K.imag.astype(np.float64))
        out = np.empty(K.shape, K.dtype)
        out.real = 0.5 * (S.real.astype(np.float64) + qr)
        out.imag = 0.5 * (S.imag.astype(np.float64) + qi)
    return out


def _compensation_tables(compensation, shape):
    lengths = (shape[0], shape[1], shape[2] // 2 + 1)
    tabs = [None] * 3 if compensation is None else list(compensation)
    if len(tabs) != 3:
        raise ValueError("compensation must be three per-axis tables (each may be None).")
    out = []
    for t, n in zip(tabs, lengths):
        if t is not None:
            t = np.asarray(t, np.float64).ravel()
            if len(t) != n or not np.all(np.isfinite(t) & (t > 0)):
                raise ValueError("a compensation table must hold {0} finite positive values.".format(n))
        out.append(t)
    return out


def bin_multipoles(kdata, spacing, edges, los, compensation=None):
    """Per-bin sums of the power spectrum multipoles of a half spectrum along grid axis ``los`` (0, 1, 2) -- the numpy statement of the
    definition the device call ``rf_measure_multipoles`` implements (csrc/rf_core.h multipole_cell).

    Cells, k2, bins and weights w as in :func:`bin_power`.  ``mu2 = klos2 / k2`` with klos2 the line-of-sight axis' own table entry;
    ``compensation``: None or three tables (nx, ny, nz/2 + 1 finite positive values, each may be None = ones), c = (cx[ix] cy[iy])
    cz[iz]; e = c |delta(k)|**2.  Returns ``(count, sum_k, m0, m2, m4)``: the uint64 sum of w and the float64 sums of ``w sqrt(k2)``,
    ``w e``, ``w (e mu2)`` and ``w ((e mu2) mu2)`` per bin."""
    edges = np.asarray(edges, np.float64).ravel()
    nbins = len(edges) - 1
    if not 1 <= nbins <= 1024 or edges[0] < 0 or not np.all(np.diff(edges) > 0):
        raise ValueError("edges must be 2 ... 1025 strictly increasing non-negative values.")
    if los not in (0, 1, 2):
        raise ValueError("Invalid los: {0!r} (expected 0, 1 or 2).".format(los))
    if kdata.ndim != 3 or kdata.shape[2] < 2:
        raise ValueError("kdata must be an (nx, ny, nz/2 + 1) half spectrum.")
    nx, ny, nz = kdata.shape[0], kdata.shape[1], 2 * (kdata.shape[2] - 1)      # (any even nz: the generic plans' shapes too)
    cx, cy, cz = _compensation_tables(compensation, (nx, ny, nz))
    kx2, ky2, kz2 = ksq_axes(nx, ny, nz, spacing)
    k2 = (kx2[:, None, None] + ky2[None, :, None]) + kz2[None, None, :]
    klos2 = np.broadcast_to((kx2[:, None, None], ky2[None, :, None], kz2[None, None, :])[los], k2.shape)
    b = np.searchsorted(edges * edges, k2.ravel(), side="right") - 1
    w = np.full(k2.shape, 2, np.int64)
    w[:, :, 0] = 1
    w[:, :, nz // 2] = 1
    w = w.ravel()
    keep = (b >= 0) & (b < nbins)
    keep[0] = False                          # the DC cell
    b, w = b[keep], w[keep]
    k2k = k2.ravel()[keep]
    re = kdata.real.astype(np.float64).ravel()[keep]
    im = kdata.imag.astype(np.float64).ravel()[keep]
    e = re * re + im * im
    if compensation is not None:
        one = np.ones(1)
        c = ((one if cx is None else cx)[:, None, None] * (one if cy is None else cy)[None, :, None]) * (one if cz is None else cz)[None, None, :]
        e = np.broadcast_to(c, k2.shape).ravel()[keep] * e
    with np.errstate(divide="ignore", invalid="ignore"):
        mu2 = np.where(k2k > 0, klos2.ravel()[keep] / k2k, 0.0)
    e2m = e * mu2
    count = np.bincount(b, weights=w, minlength=nbins).astype(np.uint64)      # (exact: integers far below 2**53)
    sum_k = np.bincount(b, weights=w * np.sqrt(k2k), minlength=nbins)
    m0 = np.bincount(b, weights=w * e, minlength=nbins)
    m2 = np.bincount(b, weights=w * e2m, minlength=nbins)
    m4 = np.bincount(b, weights=w * (e2m * mu2), minlength=nbins)
    return count, sum_k, m0, m2, m4


def multipole_estimate(count, sum_k, m0, m2, m4, shape, spacing):
    """The structured array ('k', 'P0', 'P2', 'P4', 'nmodes') of the sums of :func:`bin_multipoles` /
    ``DevicePlan.measure_multipoles``: with Mj = (V / N**2) mj / count, ``P0 = M0``, ``P2 = (5/2)(3 M2 - M0)`` and
    ``P4 = (9/8)(35 M4 - 30 M2 + 3 M0)`` (the Legendre polynomials in mu, (2l + 1) normalisation); NaN in empty bins."""
    n = float(shape[0]) * float(shape[1]) * float(shape[2])
    out = np.empty(len(count), [("k", float), ("P0", float), ("P2", float), ("P4", float), ("nmodes", np.uint64)])
    c = np.asarray(count, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        M0, M2, M4 = (np.where(c > 0, (spacing ** 3 / n) * np.asarray(m, np.float64) / c, np.nan) for m in (m0, m2, m4))
        out["k"] = np.where(c > 0, np.asarray(sum_k) / c, np.nan)
    out["P0"] = M0
    out["P2"] = 2.5 * (3.0 * M2 - M0)
    out["P4"] = 1.125 * (35.0 * M4 - 30.0 * M2 + 3.0 * M0)
    out["nmodes"] = count
    return out


def default_bispectrum_edges(shape, spacing, nbins=None):
    """``nbins + 1`` linear bin edges in k for :func:`bin_bispectrum`: from the fundamental mode of the longest axis (the first edge of
    :func:`default_k_edges`) up to 2/3 of the smallest axis' Nyquist frequency.  Below that bound three modes of the grid cannot sum
    to a non-zero multiple of the grid's period, so no triangle closes through aliasing only.  ``nbins`` defaults to
    ``min(shape) // 3`` (bins about one fundamental mode of the shortest axis wide), at most 32."""
    if nbins is None:
        nbins = max(1, min(min(shape) // 3, 32))
    nbins = int(nbins)
    if not 1 <= nbins <= 32:
        raise ValueError("nbins must be between 1 and 32.")
    k_nyq = np.pi / spacing
    first = default_k_edges(shape, spacing, 1)[0]
    if not first < (2.0 / 3.0) * k_nyq:
        raise ValueError("the grid has no modes below 2/3 of its Nyquist frequency.")
    return np.linspace(first, (2.0 / 3.0) * k_nyq, nbins + 1)


def bispectrum_triples(edges, which="closed"):
    """The ``(ntriples, 3)`` integer array of bin triples b1 <= b2 <= b3 of ``nbins + 1`` edges, in lexicographic order.  ``'all'``:
    every such triple.  ``'closed'``: those whose shells can hold a closed triangle k1 + k2 + k3 = 0 with |k_i| in shell b_i, i.e.
    ``edges[b3] < edges[b1 + 1] + edges[b2 + 1]`` -- for edges up to 2/3 of the Nyquist frequency the others hold no triangle at
    all; beyond it triangles that close modulo the grid appear in triples this rule drops.  ``'equilateral'``: b1 = b2 = b3."""
    edges = np.asarray(edges, np.float64).ravel()
    nbins = len(edges) - 1
    if nbins < 1:
        raise ValueError("edges must hold at least two values.")
    if which not in ("closed", "all", "equilateral"):
        raise ValueError("Invalid which: {0!r} (expected 'closed', 'all' or 'equilateral').".format(which))
    if which == "equilateral":
        return np.repeat(np.arange(nbins, dtype=np.intc)[:, None], 3, axis=1)
    out = [(b1, b2, b3) for b1 in range(nbins) for b2 in range(b1, nbins) for b3 in range(b2, nbins)
           if which == "all" or edges[b3] < edges[b1 + 1] + edges[b2 + 1]]
    return np.asarray(out, np.intc).reshape(-1, 3)


def bin_bispectrum(kdata, spacing, edges, triples, amp=None, unit=False):
    """The triple sums of the FFT bispectrum estimator -- the numpy statement of the definition the device call
    ``rf_measure_bispectrum`` implements (csrc/rf_core.h shell_cell, bispectrum_add), in float64 throughout.

    ``kdata``: the ``(nx, ny, nz/2 + 1)`` half spectrum of unnormalised forward-transform values.  Shells are the bins of
    :func:`bin_power` (``edges`` squared once, the DC cell in none).  ``D_b = irfftn`` (1/N) of the spectrum restricted to shell b,
    times ``amp = (ax[ix] ay[iy]) az[iz]`` where tables are given; ``unit=True``: 1 inside the shells.  Returns
    ``sum3[t] = sum_x D_b1 D_b2 D_b3`` per row of ``triples``; N**2 sum3 is the sum of delta(k1) delta(k2) delta(k3) over the ordered
    triangles k_i in shell b_i that close modulo the grid."""
    edges = np.asarray(edges, np.float64).ravel()
    nbins = len(edges) - 1
    if not 1 <= nbins <= 32 or edges[0] < 0 or not np.all(np.diff(edges) > 0):
        raise ValueError("edges must be 2 ... 33 strictly increasing non-negative values.")
    triples = np.asarray(triples).reshape(-1, 3)
    if not len(triples) or not np.all((0 <= triples[:, 0]) & (triples[:, 0] <= triples[:, 1]) & (triples[:, 1] <= triples[:, 2]) & (triples[:, 2] < nbins)):
        raise ValueError("every triple must satisfy 0 <= b1 <= b2 <= b3 < nbins.")
    if kdata.ndim != 3 or kdata.shape[2] < 2:
        raise ValueError("kdata must be an (nx, ny, nz/2 + 1) half spectrum.")
    nx, ny, nz = kdata.shape[0], kdata.shape[1], 2 * (kdata.shape[2] - 1)
    kx2, ky2, kz2 = ksq_axes(nx, ny, nz, spacing)
    k2 = (kx2[:, None, None] + ky2[None, :, None]) + kz2[None, None, :]
    b = (np.searchsorted(edges * edges, k2.ravel(), side="right") - 1).reshape(k2.shape)
    b[0, 0, 0] = -1                          # the DC cell
    if unit:
        data = np.ones(k2.shape, np.complex128)
    else:
        data = np.asarray(kdata, np.complex128)
        if amp is not None:
            ax, ay, az = _compensation_tables(amp, (nx, ny, nz))
            one = np.ones(1)
            data = data * (((one if ax is None else ax)[:, None, None] * (one if ay is None else ay)[None, :, None]) * (one if az is None else az)[None, None, :])
    fields = {}
    for s in np.unique(triples):
        fields[int(s)] = np.fft.irfftn(np.where(b == s, data, 0.0), s=(nx, ny, nz), axes=(0, 1, 2))
    return np.array([np.sum((fields[int(t[0])] * fields[int(t[1])]) * fields[int(t[2])]) for t in triples], np.float64)


def bispectrum_estimate(triples, sum3, sum3_unit, count, sum_k, sum_p, shape, spacing):
    """The structured array ('bins', 'k1', 'k2', 'k3', 'B', 'Q', 'ntriangles') of the sums of :func:`bin_bispectrum` /
    ``DevicePlan.measure_bispectrum`` (``sum3`` of the data, ``sum3_unit`` of the unit run) and of :func:`bin_power` on the same edges
    and spectrum (``count, sum_k, sum_p`` -- or a compensated ``m0`` for ``sum_p``).  With N = nx ny nz and V = N spacing**3:
    ``ntriangles = rint(N**2 sum3_unit)``, ``B = (V**2 / N**3) sum3 / sum3_unit``, ``k_i`` the mean |k| of shell b_i's modes and
    ``Q = B / (P1 P2 + P2 P3 + P3 P1)`` with ``P = (V / N**2) sum_p / count``; rows without a triangle hold NaN in B and Q."""
    triples = np.asarray(triples).reshape(-1, 3)
    n = float(shape[0]) * float(shape[1]) * float(shape[2])
    P = power_estimate(count, sum_k, sum_p, shape, spacing)
    out = np.empty(len(triples), [("bins", np.intc, (3,)), ("k1", float), ("k2", float), ("k3", float), ("B", float), ("Q", float),
                                  ("ntriangles", float)])
    out["bins"] = triples
    for i, name in enumerate(("k1", "k2", "k3")):
        out[name] = P["k"][triples[:, i]]
    s_unit = np.asarray(sum3_unit, np.float64)
    out["ntriangles"] = np.rint(n * n * s_unit) + 0.0           # (never -0)
    p1, p2, p3 = (P["Pk"][triples[:, i]] for i in range(3))
    with np.errstate(divide="ignore", invalid="ignore"):
        B = np.where(out["ntriangles"] > 0, (spacing ** 6 / n) * np.asarray(sum3, np.float64) / s_unit, np.nan)
        out["B"] = B
        out["Q"] = B / (p1 * p2 + p2 * p3 + p3 * p1)
    return out


def create_ksq_grids(data, spacing, packed):
    """Sparse broadcastable grids of kx**2, ky**2, kz**2 (powertools.py:27-37)."""
    nx, ny, nz = transform.expanded_shape(data, packed=packed)
    kx2, ky2, kz2 = ksq_axes(nx, ny, nz, spacing, packed=packed)
    return np.meshgrid(kx2, ky2, kz2, sparse=True, indexing="ij")


def fill_with_log10k(data, spacing, packed=True):
    """
    Fill an array with values of log10(k) (powertools.py:40-61).

    Note that the value at [0, 0, 0] will be log10(0) = -inf.  Built from the
    three axis tables: the (nx, ny) plane of kx**2 + ky**2 is formed in float64
    and rounded to the array's real type once, kz**2 is then added to it in
    float64 and the sum rounded again -- the same two roundings per cell as the
    reference's in-place ufunc chain, which is what makes the result
    bit-identical to it -- then log10 and the halving in the array's real type.
    """
    kx2, ky2, kz2 = ksq_axes(*transform.expanded_shape(data, packed=packed), spacing, packed=packed)
    re = data.real
    plane = np.add.outer(kx2, ky2).astype(re.dtype)
    np.add(plane[:, :, None], kz2[None, None, :], out=re, casting="same_kind")
    with np.errstate(divide="ignore"):
        np.log10(re, out=re)
    np.multiply(re, re.dtype.type(0.5), out=re)
    data.imag = 0
    return data


# validate_power: (test on the table -> True when it FAILS, message), checked in this order (powertools.py:64-82)
_POWER_RULES = (
    (lambda p: not np.all(np.isfinite(p["k"])), "Power spectrum has some invalid values of k."),
    (lambda p: not np.all(np.isfinite(p["Pk"])), "Power spectrum has some invalid values of P(k)."),
    (lambda p: not np.array_equal(p["k"], np.unique(p["k"])), "Power spectrum k values are not strictly increasing."),
    (lambda p: p["k"][0] <= 0, "Power spectrum min(k) is <= 0."),
    (lambda p: np.any(p["Pk"] < 0), "Power values P(k) are not all non-negative."),
)


def validate_power(power):
    """Validates a power spectrum (powertools.py:64-82); returns it."""
    if not isinstance(power, np.ndarray):
        raise ValueError("Invalid type for power: {0}.".format(type(power)))
    if not {"k", "Pk"} <= set(power.dtype.names or ()):
        raise ValueError('Missing required fields "k", "Pk" in power.')
    for fails, message in _POWER_RULES:
        if fails(power):
            raise ValueError(message)
    return power


def filter_power(power, sigma, out=None):
    """
    Apply a Gaussian filtering to a power spectrum (powertools.py:85-122):
    P(k) -> P(k) * exp(-(k*sigma)**2), i.e. delta(r) is convolved with a 3D
    Gaussian of width sigma.  ``out=None`` returns a filtered copy, ``out=power``
    filters in place, any other ``out`` receives the filtered table.
    """
    if sigma < 0:
        raise ValueError("Invalid smoothing sigma: {0}.".format(sigma))
    if out is None:
        out = power.copy()
    elif out is not power:
        if validate_power(power).shape != out.shape:
            raise ValueError("Output power has wrong shape: {0}.".format(out.shape))
        out[...] = power
    if sigma > 0:
        np.multiply(out["Pk"], np.exp(-np.square(power["k"] * sigma)), out=out["Pk"])
    return out


def sigma_table(power, shape, spacing):
    """
    The two float64 tables of the sigma(k) interpolator (powertools.py:139-154):
    x_i = log10 k_i and s_i = N3 * sqrt(P_i / (2 Vbox)), after the reference's
    range check that the table covers the grid's [k_min, k_max].
    These are what the HIP kernels consume (``rf_set_power``).
    """
    k, Pk = validate_power(power)["k"], power["Pk"]
    cells = shape[0] * shape[1] * shape[2]
    volume = cells * spacing ** 3
    table_lo, table_hi = np.min(k), np.max(k)
    if table_lo <= 0:
        raise ValueError("Power uses min(k) <= 0: {0}.".format(table_lo))
    grid_lo, grid_hi = grid_k_range(shape, spacing)
    if table_lo > grid_lo or table_hi < grid_hi:
        raise ValueError("Power k range [{0}:{1}] does not cover data k range [{2}:{3}]."
                         .format(table_lo, table_hi, grid_lo, grid_hi))
    return np.log10(k), cells * np.sqrt(Pk / (2 * volume))


def tabulate_sigmas(data, power, spacing, packed=True):
    """
    Replace an array of log10(k) values with the corresponding sigmas
    (powertools.py:125-164):  sigma**2 = (nx*ny*nz) * P(k) / (2 * Vbox).

    sigma is interpolated linearly in log10(k), zero outside the table
    (so the -inf at [0,0,0] becomes 0).
    """
    shape = transform.expanded_shape(data, packed=packed)
    log10_k, sigma = sigma_table(power, shape, spacing)
    data.real = np.interp(data.real, log10_k, sigma, left=0.0, right=0.0)
    return data


def make_power(k, Pk):
    """Build the structured array (fields 'k', 'Pk') the API expects."""
    k = np.asarray(k, float)
    power = np.empty(len(k), dtype=[("k", float), ("Pk", float)])
    power["k"] = k
    power["Pk"] = Pk
    return power


def load_default_power(scaled_by_h=True, h=None):
    """
    Loads the default power spectrum P(k, z=0) (powertools.py:167-197): 500 rows,
    1e-4 <= k <= 22 h/Mpc, Planck13 via CLASS; units h/Mpc and (Mpc/h)**3.

    The table is stored as ``data/default_power.npz`` (binary copy of the
    reference's data file).  ``scaled_by_h=False`` converts to 1/Mpc and Mpc**3 and
    needs the Hubble parameter ``h`` (the reference takes it from its astropy
    cosmology, which is outside this package's scope: Planck13 has h = 0.6777).
    """
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "default_power.npz")
    try:
        table = np.load(path)
    except IOError:
        raise RuntimeError("Unable to load default_power.npz")
    power = make_power(table["k"], table["Pk"])
    if scaled_by_h is False:
        if h is None:
            raise ValueError("load_default_power(scaled_by_h=False) needs h= (e.g. 0.6777 for Planck13).")
        power["k"] *= h
        power["Pk"] /= h ** 3
    return power
