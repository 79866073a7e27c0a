"""User power tables for the value tests of the generation pass (helpers, no tests).

Every GPU value test before these used the 500-row default power, far wider than any grid's k range; the native path's float32 sigma
lookup (csrc/rf_host.h build_fast_records, csrc/rf_core.h fast_sigma / sigma_lookup) has branches that table never reaches: all-zero
guard bins, 256- and 512-bin records, the fall-back to the exact kernel, 2-row tables, tables that end inside the grid, and cells ON a
table edge.  The builders below return (k, Pk) for a shape and spacing; all sample the default power's shape, interpolated log-log, so
the error budget of the existing native tests (1e-5 rms) carries over.

    hug         100 rows, k[0] = k_min and k[-1] = k_max exactly as cpu_ref.k_bounds returns them: the fundamental and corner modes
                sit ON the edges (the edge rule, csrc/rf_core.h RF_EDGE_TOL)
    hug2        the 2-row version
    control     hug widened by 5 % at both ends: no cell near an edge, no guard bin
    dense       log-uniform rows over the control range, closer than a 510th of the padded grid range: the records would need more
                than 512 bins, the plan runs the exact kernel
    clustered   20 log-uniform rows over the hug range plus a pair of close knots: 256 or 512 records (two of them guard bins)
    kinked      control with a run of rows Pk = 0 inside: sigma falls to 0, stays there, rises again (the slope changes sign)
    band        low-pass / band-pass tables whose edges lie strictly inside the grid's range (rf_set_power does not ask for coverage;
                cpu_ref.sigma_table and the package's powertools.sigma_table do, so these go through DevicePlan / the emulator only)

Edges that fall inside the grid's range (band, the zero run of kinked) are put at the geometric midpoint between two neighbouring
distinct grid |k| values that lie at least 2.2e-4 dex apart, so that no mode is within 1e-4 dex of one: fifty times RF_EDGE_TOL, where
every chain -- oracle, exact kernel, fast kernel -- must give the same answer.
"""
import functools
import math
import os

import numpy as np

from oracle import cpu_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CLEAR_DEX = 1e-4                 # no grid mode within this of an edge that lies inside the grid's range
MIN_GAP_DEX = 2.2e-4             # ... so a gap must be this wide to take an edge at its midpoint
TABLES = ("control", "hug", "hug2", "dense", "clustered256", "clustered512", "kinked", "band_low", "band_pass")
COVERING = tuple(t for t in TABLES if not t.startswith("band"))          # what cpu_ref.sigma_table accepts


@functools.lru_cache(maxsize=None)
def _default():
    d = np.load(os.path.join(GOLDEN, "default_power.npz"))
    return np.log10(d["k"]), np.log10(d["Pk"])


def default_shape(k):
    """the default power at k, interpolated log-log"""
    lk, lp = _default()
    return 10.0 ** np.interp(np.log10(k), lk, lp)


def _logspace(klo, khi, n):
    """n log-uniform rows whose ends are klo and khi exactly"""
    k = np.logspace(np.log10(klo), np.log10(khi), n)
    k[0], k[-1] = klo, khi
    return k


def grid_range(shape, spacing):
    """(xlo, xhi): the padded log10 k range over which the library builds the fast records (rf_capi.hip build_fast)"""
    kmin, kmax = cpu_ref.k_bounds(*shape, spacing)
    return np.log10(kmin) - 0.01, np.log10(kmax) + 0.01


@functools.lru_cache(maxsize=None)
def grid_modes(shape):
    """Distinct |k|^2 of the packed grid as exact integers q (|k|^2 = q (2 pi / (L spacing))^2, L = lcm of the axes), from the integer
    index triples, with the number of packed cells at each; the DC cell is left out."""
    nx, ny, nz = shape
    L = math.lcm(nx, ny, nz)
    def axis(n, half=False):
        i = np.arange(n, dtype=np.int64)
        i[i >= (n + 1) // 2] -= n
        return ((i[: n // 2 + 1] if half else i) * (L // n)) ** 2
    q = (axis(nx)[:, None, None] + axis(ny)[None, :, None] + axis(nz, True)[None, None, :]).reshape(-1)
    q, count = np.unique(q[q > 0], return_counts=True)
    return L, q, count


@functools.lru_cache(maxsize=None)
def mode_log10k(shape, spacing):
    """(log10|k| of every distinct non-DC mode, packed cells at each), float64"""
    L, q, count = grid_modes(tuple(shape))
    return 0.5 * np.log10(q.astype(np.float64)) + np.log10(2 * np.pi / (L * spacing)), count


class NoClearEdge(Exception):
    """the modes of this grid leave no gap of MIN_GAP_DEX where the table would need an edge"""


def clear_gaps(shape, spacing):
    """(log10 k of the midpoint, fraction of the non-DC packed cells below it) of every gap of at least MIN_GAP_DEX between two
    neighbouring distinct grid |k|, ascending.  Long thin grids have such gaps only among their first modes: the squares of a long
    axis fill everything above."""
    x, count = mode_log10k(shape, spacing)
    cum = np.cumsum(count) / count.sum()
    ok = np.nonzero(np.diff(x) >= MIN_GAP_DEX)[0]
    return 0.5 * (x[ok] + x[ok + 1]), cum[ok]


def _nearest(frac, target, allowed):
    idx = np.nonzero(allowed)[0]
    if idx.size == 0:
        raise NoClearEdge()
    return int(idx[np.argmin(np.abs(frac[idx] - target))])


def assert_clear(shape, spacing, k_edges):
    """regime guard: no grid mode within CLEAR_DEX of an edge"""
    x, _ = mode_log10k(shape, spacing)
    for ke in k_edges:
        d = float(np.min(np.abs(x - np.log10(ke))))
        assert d > CLEAR_DEX, "a mode of %r lies %.3g dex from the edge k = %r" % (shape, d, ke)


def outside_fraction(shape, spacing, k):
    """fraction of the non-DC packed cells outside [k[0], k[-1]]"""
    x, count = mode_log10k(shape, spacing)
    out = (x < np.log10(k[0])) | (x > np.log10(k[-1]))
    return float(count[out].sum() / count.sum())


def hug(shape, spacing, nrows=100):
    kmin, kmax = cpu_ref.k_bounds(*shape, spacing)
    k = _logspace(kmin, kmax, nrows)
    return k, default_shape(k)


def hug2(shape, spacing):
    return hug(shape, spacing, 2)


def control(shape, spacing, nrows=100):
    kmin, kmax = cpu_ref.k_bounds(*shape, spacing)
    k = _logspace(kmin / 1.05, kmax * 1.05, nrows)
    return k, default_shape(k)


def dense(shape, spacing):
    xlo, xhi = grid_range(shape, spacing)
    kmin, kmax = cpu_ref.k_bounds(*shape, spacing)
    h = (xhi - xlo) / 700.0                                    # < a 510th of the records' range: two knots in some bin at 510 bins
    nrows = int(np.ceil(np.log10(1.05 ** 2 * kmax / kmin) / h)) + 1
    k = _logspace(kmin / 1.05, kmax * 1.05, nrows)
    return k, default_shape(k)


def clustered(shape, spacing, nb):
    """20 log-uniform rows over the hug range and two knots 1.5 bins of the next finer bin count apart, centred in one bin of every
    coarser count: nb = 256 (254 + 2 guard bins) or 512 (510 + 2)."""
    assert nb in (256, 512)
    kmin, kmax = cpu_ref.k_bounds(*shape, spacing)
    x0, x1 = np.log10(kmin) - cpu_ref.EDGE_TOL, np.log10(kmax) + cpu_ref.EDGE_TOL      # what the records span (margins included)
    R = x1 - x0
    if nb == 256:
        c, s = x0 + 60.5 * R / 126, 1.5 * R / 254              # inside bin 60 of 126; more than one bin of 254 apart
    else:
        c, s = x0 + 121.5 * R / 254, 1.5 * R / 510             # inside bin 121 of 254 = inside bin 60 of 126; apart at 510
    k = np.sort(np.concatenate([_logspace(kmin, kmax, 20), 10.0 ** np.array([c - s / 2, c + s / 2])]))
    assert np.all(np.diff(np.log10(k)) > s / 4)
    return k, default_shape(k)


def kinked(shape, spacing, nrows=60):
    xe, fe = clear_gaps(shape, spacing)
    a = _nearest(fe, 0.02, np.ones(fe.size, bool))             # (2 % and 6 % of the cells below: a third and a half of the Nyquist k
    b = _nearest(fe, 0.06, np.abs(xe - xe[a]) >= 0.04)         # on a cube; a run wide enough for 126 bins to keep its knots apart)
    ka, kb = 10.0 ** xe[min(a, b)], 10.0 ** xe[max(a, b)]
    k0, _ = control(shape, spacing, nrows)
    # the ramps into and out of the run span a factor 2 in k: about as steep per dex as the default power itself falls, so that the last
    # ulp of log10|k| moves sigma no more than it does there (the k-space bounds were set on the default table)
    k = np.unique(np.concatenate([k0[(k0 < ka / 2) | (k0 > kb * 2)], _logspace(ka, kb, 3)]))
    Pk = default_shape(k)
    Pk[(k >= ka) & (k <= kb)] = 0.0
    assert Pk[0] > 0 and Pk[-1] > 0 and k[0] == k0[0] and k[-1] == k0[-1]
    assert_clear(shape, spacing, (ka, kb))
    return k, Pk


def band(shape, spacing, kind, nrows=50):
    """low: from below k_min to an edge with about half of the cells above it; pass: about 15 % below and 35 % above.  On long thin
    grids the edges move to where the gaps are; NoClearEdge if no choice leaves 10 % - 90 % of the cells outside."""
    kmin, kmax = cpu_ref.k_bounds(*shape, spacing)
    xe, fe = clear_gaps(shape, spacing)
    if kind == "low":
        hi = _nearest(fe, 0.50, (fe >= 0.10) & (fe <= 0.90))
        klo, khi = kmin / 1.05, 10.0 ** xe[hi]
        edges = (khi,)
    else:
        hi = _nearest(fe, 0.65, (fe >= 0.10) & (fe <= 0.90))
        lo = _nearest(fe, 0.15, (np.arange(fe.size) < hi) & (fe + (1.0 - fe[hi]) <= 0.90))
        klo, khi = 10.0 ** xe[lo], 10.0 ** xe[hi]
        edges = (klo, khi)
    k = _logspace(klo, khi, nrows)
    assert_clear(shape, spacing, edges)
    f = outside_fraction(shape, spacing, k)
    assert 0.10 <= f <= 0.90, "%.3f of the cells of %r lie outside the %s-pass table" % (f, shape, kind)
    return k, default_shape(k)


def build(name, shape, spacing):
    shape = tuple(shape)
    if name == "clustered256":
        return clustered(shape, spacing, 256)
    if name == "clustered512":
        return clustered(shape, spacing, 512)
    if name == "band_low":
        return band(shape, spacing, "low")
    if name == "band_pass":
        return band(shape, spacing, "pass")
    return {"hug": hug, "hug2": hug2, "control": control, "dense": dense, "kinked": kinked}[name](shape, spacing)


def expected_path(name):
    """the generation kernel a tiled plan must report for the table (rf_diag_generation_path)"""
    return "exact" if name == "dense" else "fast"


# ---- the oracle without the reference's coverage check ------------------------------------------
def sigma_table(k, Pk, shape, spacing):
    """(log10 k, sigma) as cpu_ref.sigma_table (powertools.py:139-154) forms them, without the range check of :147-150"""
    n3 = shape[0] * shape[1] * shape[2]
    return np.log10(np.asarray(k, np.float64)), n3 * np.sqrt(np.asarray(Pk, np.float64) / (2 * n3 * spacing ** 3))


def oracle_kspace(shape, spacing, k, Pk, noise, dtype=np.complex64, edge_tol=cpu_ref.EDGE_TOL):
    """generate.py:191-199 through cpu_ref's stages with the HIP path's edge rule (cpu_ref.EDGE_TOL; 0 = the reference's own
    last-bit outcome) and no coverage check"""
    data = cpu_ref.fill_log10k(*shape, spacing, dtype)
    xt, st = sigma_table(k, Pk, shape, spacing)
    data.real = cpu_ref.interp_sigma(data.real, xt, st, edge_tol)
    cpu_ref.randomize(data, noise=noise)
    return cpu_ref.symmetrize_packed(data)


def oracle_field(shape, spacing, k, Pk, noise, dtype=np.complex64, edge_tol=cpu_ref.EDGE_TOL):
    """(k space, delta, rms): the float64 transform of that k space, rounded once to the plan's real type; rms in float64"""
    ks = oracle_kspace(shape, spacing, k, Pk, noise, dtype, edge_tol)
    delta = cpu_ref.c2r(ks, double_fft=True)
    return ks, delta, float(np.std(delta.astype(np.float64)))
