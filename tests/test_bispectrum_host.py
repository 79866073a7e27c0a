"""The binned bispectrum without a GPU: the two oracles of tests/bispectrum_oracle.py against each other, the closed form for three
plane waves through Generator(backend='numpy') and through the CPU emulator (emu_kspace_shell, the emulated c2r, emu_bispectrum_sums:
the cell functions the device kernels call), the shell filter's and the sums' own contracts, powertools.bispectrum_triples against
explicit triangle counts, and the feature bit.

Bounds.  Oracle against oracle: 1e-12 of the largest sum (float64 transforms of <= 2048 cells).  The emulator's sums against the exact
sum (math.fsum) of the same terms: 4 cells 2^-53 sum|term| -- a float64 sum of `cells` terms in any order is within
(cells - 1) 2^-53 sum|term| of it.  Plane waves: 1e-9 of the closed form through float64 numpy, 1e-4 through the emulator's complex64
transform (tests/axis_matrix.py holds it to 1e-5 rms of the field; three factors)."""
import ctypes
import os
import re

import numpy as np
import pytest

import bispectrum_oracle as bo
import emu_util
import power_oracle as po
from power_oracle import C64, C128

SPACING = 2.5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_vp = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)
_dp = lambda a: None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def kf(n):
    return 2 * np.pi / (n * SPACING)


def ksq(shape):
    from randomfield_amd import powertools
    return [np.ascontiguousarray(t) for t in powertools.ksq_axes(*shape, SPACING)]


def emu_shell(kdata, shape, edges, shell, amp=None, unit=False):
    kx2, ky2, kz2 = ksq(shape)
    edges = np.ascontiguousarray(edges, np.float64)
    kdata = np.ascontiguousarray(kdata)
    out = np.full(kdata.shape, np.nan, kdata.dtype)
    tabs = [None] * 3 if amp is None else [None if t is None else np.ascontiguousarray(t, np.float64) for t in amp]
    rc = emu_util.lib().emu_kspace_shell(int(kdata.dtype == C128), *shape, _dp(kx2), _dp(ky2), _dp(kz2), _vp(kdata), _dp(edges), len(edges) - 1,
                                         int(shell), *[_dp(t) for t in tabs], int(unit), _vp(out))
    assert rc == 0, rc
    return out


def emu_sums(fields, triples):
    F = np.ascontiguousarray(np.stack([np.asarray(f).ravel() for f in fields]))
    assert F.dtype in (np.float32, np.float64)
    tri = np.ascontiguousarray(np.asarray(triples).reshape(-1, 3), np.intc)
    out = np.full(len(tri), np.nan, np.float64)
    rc = emu_util.lib().emu_bispectrum_sums(int(F.dtype == np.float64), ctypes.c_longlong(F.shape[1]), F.shape[0], _vp(F), _vp(tri), len(tri), _dp(out))
    assert rc == 0, rc
    return out


def emu_c2r(kdata, shape):
    tiled = all(n & (n - 1) == 0 for n in shape)
    return (emu_util.c2r if tiled else emu_util.generic_c2r)(kdata)[0]


def all_triples(nbins):
    from randomfield_amd import powertools
    return powertools.bispectrum_triples(np.arange(nbins + 1.0), "all")


# ---- 1. the two oracles -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,nbins", [((8, 8, 16), 4), ((4, 6, 8), 3)], ids=po.ids)
def test_fft_and_explicit_oracles_agree(shape, nbins):
    n = float(np.prod(shape))
    edges = np.linspace(0.9 * kf(max(shape)), 0.95 * np.pi / SPACING, nbins + 1)      # (up to Nyquist: aliased triangles are in both)
    triples = all_triples(nbins)
    src = po.spectrum(shape, C128)
    want, counts = bo.explicit_oracle(src, shape, SPACING, edges, triples)
    got = n * n * bo.fft_oracle(src, shape, SPACING, edges, triples)
    err = np.max(np.abs(got - want)) / np.max(np.abs(want))
    print("%s: FFT against explicit, %.3e of the largest; %d triangles" % (shape, err, counts.sum()))
    assert err <= 1e-12
    unit = n * n * bo.fft_oracle(src, shape, SPACING, edges, triples, unit=True)
    ucounts = bo.explicit_oracle(None, shape, SPACING, edges, triples, unit=True)[1]
    assert np.array_equal(ucounts, counts) and counts.sum() > 0
    assert np.array_equal(np.rint(unit).astype(np.int64), counts) and np.max(np.abs(unit - counts)) <= 1e-6


# ---- 2. three plane waves ---------------------------------------------------------------------------------------------------------
WAVE_SHAPE = (8, 8, 16)
WAVE_MODES = [(0, 1, 0), (1, 1, 2), (-1, -2, -2)]         # |k| = 1, 1.73, 2.45 fundamental modes of the 8-cell axes; they sum to 0
WAVE_AMPS, WAVE_PHASES = (0.7, 1.3, 0.9), (0.4, -1.1, 2.3)
# edges in units of that fundamental mode (all below 2/3 of the Nyquist frequency, 2.67), the triple holding the modes, n_perm
WAVE_CASES = [([0.5, 1.5, 2.0, 2.6], (0, 1, 2), 1), ([0.2, 0.5, 1.5, 2.6], (1, 2, 2), 2), ([0.2, 0.5, 2.6], (1, 1, 1), 6)]


def wave_expected(nperm):
    n = float(np.prod(WAVE_SHAPE))
    return 2.0 * nperm * (n / 2) ** 3 * np.prod(WAVE_AMPS) * np.cos(np.sum(WAVE_PHASES))


def check_waves(n2s, triples, holder, nperm, rtol, what):
    want = wave_expected(nperm)
    at = [i for i, t in enumerate(triples) if tuple(t) == holder]
    assert len(at) == 1
    err = abs(n2s[at[0]] - want) / abs(want)
    others = np.delete(n2s, at[0])
    print("%s %s: %.3e of the closed form, other triples at most %.3e of it" % (what, holder, err, np.max(np.abs(others)) / abs(want) if len(others) else 0.0))
    assert err <= rtol
    assert np.all(np.abs(others) <= rtol * abs(want))


@pytest.mark.parametrize("edges,holder,nperm", WAVE_CASES, ids=["distinct", "1-2-2", "equal"])
def test_plane_waves_numpy_generator(edges, holder, nperm):
    from randomfield_amd import Generator
    field = bo.plane_waves(WAVE_SHAPE, WAVE_MODES, WAVE_AMPS, WAVE_PHASES)
    for m in WAVE_MODES:
        assert edges[0] * kf(8) <= bo.mode_k(WAVE_SHAPE, SPACING, m) < edges[-1] * kf(8)
    gen = Generator(*WAVE_SHAPE, SPACING, backend="numpy", dtype=C128)
    res = gen.measure_bispectrum(field, k_edges=np.array(edges) * kf(8), triangles="all")
    n = float(np.prod(WAVE_SHAPE))
    ok = res["ntriangles"] > 0
    assert ok[[tuple(t) == holder for t in res["bins"]]].all()
    assert np.all(np.isnan(res["B"][~ok])) and np.all(np.isnan(res["Q"][~ok]))
    n2s = np.where(ok, res["B"] * res["ntriangles"] * n / SPACING ** 6, 0.0)        # B = (h^6 / N) s / s_unit, ntriangles = N^2 s_unit
    check_waves(n2s, res["bins"], holder, nperm, 1e-9, "numpy backend")
    # the three modes are what the bins' mean |k| and P see
    row = res[[tuple(t) == holder for t in res["bins"]]][0]
    assert row["Q"] == row["Q"] and row["k1"] <= row["k2"] <= row["k3"]


@pytest.mark.parametrize("dtype,rtol", [(C128, 1e-9), (C64, 1e-4)], ids=po.ids)
@pytest.mark.parametrize("edges,holder,nperm", WAVE_CASES, ids=["distinct", "1-2-2", "equal"])
def test_plane_waves_emulator(edges, holder, nperm, dtype, rtol):
    field = bo.plane_waves(WAVE_SHAPE, WAVE_MODES, WAVE_AMPS, WAVE_PHASES)
    src = np.ascontiguousarray(np.fft.rfftn(field).astype(dtype))
    e = np.array(edges) * kf(8)
    fields = [emu_c2r(emu_shell(src, WAVE_SHAPE, e, b), WAVE_SHAPE) for b in range(len(e) - 1)]
    triples = all_triples(len(e) - 1)
    n = float(np.prod(WAVE_SHAPE))
    check_waves(n * n * emu_sums(fields, triples), triples, holder, nperm, rtol, "emulator")


# ---- 3. the shell filter ----------------------------------------------------------------------------------------------------------
def grid_edges(shape):
    """edges taken from the grid's own |k| values whose squares are those k^2 again: cells sit exactly on them"""
    k2 = np.unique(po.k2_grid(shape, SPACING))
    k2 = k2[k2 > 0]
    exact = k2[np.sqrt(k2) ** 2 == k2]
    assert len(exact) >= 4
    return np.sqrt(exact[np.linspace(0, len(exact) - 1, 4).astype(int)])


@pytest.mark.parametrize("shape,dtype", [((8, 8, 16), C64), ((8, 8, 16), C128), ((4, 6, 8), C64), ((6, 10, 14), C128)], ids=po.ids)
def test_emulator_shell_filter(shape, dtype):
    src = po.spectrum(shape, dtype)
    edges = grid_edges(shape)
    sh = bo.shells(shape, SPACING, edges)
    k2 = po.k2_grid(shape, SPACING)
    amp = bo.symmetric_tables(shape)
    count = np.zeros(3, np.uint64)
    sk, sp = np.zeros(3), np.zeros(3)
    kx2, ky2, kz2 = ksq(shape)
    rc = emu_util.lib().emu_measure_power(int(dtype == C128), *shape, 0, _dp(kx2), _dp(ky2), _dp(kz2), _vp(src), _dp(np.ascontiguousarray(edges)), 3,
                                          _vp(count), _dp(sk), _dp(sp))
    assert rc == 0
    on_edge = 0
    for b in range(3):
        keep = sh == b
        M = emu_shell(src, shape, edges, b)
        assert np.array_equal(M[keep].view(np.uint8), src[keep].view(np.uint8)), "kept cells are the input's, bit for bit"
        assert np.all(M[~keep] == 0)
        assert np.array_equal(emu_shell(src, shape, edges, b, amp), bo.masked(src, sh, b, amp)), "the float64 product rounded once"
        U = emu_shell(src, shape, edges, b, amp, unit=True)
        assert np.array_equal(U, keep.astype(dtype)), "the unit form is exactly 0 or 1, whatever the tables"
        # a cell whose k^2 equals an edge belongs to the upper shell, and rf_measure_power's bin holds exactly the kept cells
        lower, upper = k2 == edges[b] ** 2, k2 == edges[b + 1] ** 2
        assert lower.any() and upper.any() and keep[lower].all() and not keep[upper].any()
        on_edge += int(lower.sum())
        assert int((po.weights(shape) * keep).sum()) == int(count[b])
    assert on_edge > 0 and sh[0, 0, 0] == -1


def test_emulator_shell_filter_refuses():
    shape = (4, 6, 8)
    src = po.spectrum(shape, C64)
    kx2, ky2, kz2 = ksq(shape)
    out = np.empty_like(src)
    bad = np.ones(4)
    bad[2] = -1.0
    for edges, shell, tab in (([0.1, 0.3], 1, None), ([0.3, 0.1], 0, None), ([0.1, 0.3], 0, bad)):
        e = np.ascontiguousarray(edges, np.float64)
        rc = emu_util.lib().emu_kspace_shell(0, *shape, _dp(kx2), _dp(ky2), _dp(kz2), _vp(src), _dp(e), len(e) - 1, shell, _dp(tab), None, None, 0, _vp(out))
        assert rc == -1


# ---- 4. the sums ------------------------------------------------------------------------------------------------------------------
SUM_CASES = [((8, 8, 16), C64, 12), ((8, 8, 16), C128, 12), ((8, 8, 16), C64, 32), ((8, 8, 16), C128, 32), ((4, 6, 8), C64, 5), ((6, 10, 14), C128, 7)]


def random_fields(shape, dtype, nbins, seed=9):
    rt = np.float32 if dtype == C64 else np.float64
    rng = np.random.RandomState(seed)
    return [np.ascontiguousarray((rng.normal(size=shape) * rng.uniform(0.1, 10.0)).astype(rt)) for _ in range(nbins)]


@pytest.mark.parametrize("shape,dtype,nbins", SUM_CASES, ids=po.ids)
def test_emulator_sums_against_fsum(shape, dtype, nbins):
    triples = all_triples(nbins)
    assert len(triples) == nbins * (nbins + 1) * (nbins + 2) // 6 and (nbins, len(triples)) in ((12, 364), (32, 5984), (5, 35), (7, 84))
    fields = random_fields(shape, dtype, nbins)
    want, absum = bo.triple_sums(fields, triples)
    got = emu_sums(fields, triples)
    bound = bo.reduction_bound(int(np.prod(shape)), absum)
    worst = np.max(np.abs(got - want) / bound)
    print("%s %s %d triples: worst difference %.3f of the bound" % (shape, po.ids(dtype), len(triples), worst))
    assert np.all(np.abs(got - want) <= bound)
    dup = emu_sums(fields, np.concatenate([triples[:3], triples[:3]]))
    assert np.array_equal(dup[:3], dup[3:]) and np.array_equal(dup[:3], got[:3]), "duplicates are allowed and give the same bits"


def test_emulator_sums_refuse_bad_triples():
    fields = random_fields((4, 6, 8), C64, 3)
    F = np.ascontiguousarray(np.stack([f.ravel() for f in fields]))
    out = np.zeros(1)
    for t in ((1, 0, 2), (0, 1, 3), (-1, 0, 0)):
        tri = np.array([t], np.intc)
        assert emu_util.lib().emu_bispectrum_sums(0, ctypes.c_longlong(F.shape[1]), 3, _vp(F), _vp(tri), 1, _dp(out)) == -1


# ---- 5. bispectrum_triples --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 8, 16), (16, 16, 16)], ids=po.ids)
def test_closed_triples_are_the_ones_with_triangles(shape):
    """Below 2/3 of the Nyquist frequency no triangle closes through aliasing, so a triple holds a triangle iff its shells admit one:
    asserted in both directions.  The rule is a statement about the continuum; on the lattice it needs shells about a fundamental mode
    of the longest axis wide (four bins here: 1.08 of them) -- narrower shells can be closed on paper and hold no lattice triangle
    (five bins at 16^3: two such triples; their rows are NaN).
    With edges up to the Nyquist frequency the triangles that close only modulo the grid are there, in both the FFT estimator and
    the count.  They sit in 'closed' triples: wrapping a component into [-n/2, n/2) never lengthens a vector, so |k3| <= |k1| + |k2|
    holds for them too and the rule never drops a triple that holds a triangle -- what it no longer says is that the triangles of
    a triple close exactly."""
    from randomfield_amd import powertools
    edges = powertools.default_bispectrum_edges(shape, SPACING, 4)
    assert edges[-1] <= (2.0 / 3.0) * np.pi / SPACING
    every = powertools.bispectrum_triples(edges, "all")
    closed = {tuple(t) for t in powertools.bispectrum_triples(edges, "closed")}
    counts = bo.explicit_oracle(None, shape, SPACING, edges, every, unit=True)[1]
    for t, c in zip(every, counts):
        assert (tuple(t) in closed) == (c > 0), (tuple(t), int(c))
    assert closed and len(closed) < len(every) and {tuple(t) for t in powertools.bispectrum_triples(edges, "equilateral")} <= closed
    assert np.array_equal(bo.explicit_oracle(None, shape, SPACING, edges, every, unit=True, exact=True)[1], counts), "no aliased triangle below 2/3 Nyquist"
    nyq = np.linspace(edges[0], np.pi / SPACING, len(edges))
    every = powertools.bispectrum_triples(nyq, "all")
    closed = {tuple(t) for t in powertools.bispectrum_triples(nyq, "closed")}
    counts = bo.explicit_oracle(None, shape, SPACING, nyq, every, unit=True)[1]
    exact = bo.explicit_oracle(None, shape, SPACING, nyq, every, unit=True, exact=True)[1]
    aliased = counts - exact
    print("%s: %d of %d triangles close through aliasing alone, in %d triples" % (shape, aliased.sum(), counts.sum(), (aliased > 0).sum()))
    assert np.all(aliased >= 0) and aliased.sum() > 0
    assert all(tuple(t) in closed for t, c in zip(every, counts) if c > 0)


def test_triples_and_default_edges_arguments():
    from randomfield_amd import powertools
    e = np.array([0.1, 0.2, 0.45, 0.6])
    assert [tuple(t) for t in powertools.bispectrum_triples(e, "equilateral")] == [(0, 0, 0), (1, 1, 1), (2, 2, 2)]
    assert len(powertools.bispectrum_triples(e, "all")) == 10
    closed = {tuple(t) for t in powertools.bispectrum_triples(e, "closed")}
    assert (0, 0, 2) not in closed and (0, 0, 1) in closed          # e[2] = 0.45 >= 0.2 + 0.2 > e[1]
    with pytest.raises(ValueError):
        powertools.bispectrum_triples(e, "open")
    with pytest.raises(ValueError):
        powertools.default_bispectrum_edges((8, 8, 8), SPACING, 33)
    d = powertools.default_bispectrum_edges((16, 16, 32), SPACING, 6)
    assert len(d) == 7 and np.all(np.diff(d) > 0) and d[-1] == (2.0 / 3.0) * np.pi / SPACING and d[0] ** 2 <= powertools.ksq_axes(16, 16, 32, SPACING)[2][1]


# ---- 6. the feature bit -----------------------------------------------------------------------------------------------------------
def test_feature_bit_and_version():
    from randomfield_amd import _hip
    header = open(os.path.join(ROOT, "include", "randomfield_hip.h")).read()
    assert re.search(r"RF_FEATURE_BISPECTRUM\s*=\s*1\s*<<\s*22\b", header)
    assert re.search(r"#define RF_ABI_MAJOR 5\b", header) and re.search(r"#define RF_ABI_MINOR 5\b", header)
    assert _hip.FEATURES["bispectrum"] == 1 << 22
    assert "bispectrum" in _hip.abi_features()
    assert _hip.abi_version() == (5, 5)
    for name in ("rf_measure_bispectrum", "rf_bispectrum_release"):
        assert name in _hip.SIGNATURES and re.search(r"\bint %s\(" % name, header)
    for name in ("rf_bispectrum_download_shell", "rf_bispectrum_set_max_workgroups", "rf_bispectrum_geometry"):
        assert name in _hip.DIAG_SIGNATURES
