"""The binned power spectrum estimator (csrc/rf_core.h power_cell / power_load) without a GPU: powertools.bin_power and the emulator's
emu_measure_power -- the same cell and bin function the device sweep runs, over an array in API layout and in the packed layout of the
tiled forward passes -- against the float64 numpy oracle of tests/power_oracle.py; the edge cases of the bin rule; the numpy backend of
Generator.measure_power_spectrum against the input table; the ABI surface (version 5.5 unchanged, feature bit 15).

Tolerances.  Counts are integers and must be exact.  sum_k and sum_p are sums of non-negative float64 terms: the summation error is at
most n 2^-53 < 2e-11 relative for the at most 1e5 cells used here; rtol 1e-9 is that with a 50-fold margin.  The statistical check:
|delta(k)|^2 of a mode is exponentially distributed and nmodes / 2 modes of a bin are independent, so a bin scatters by
sqrt(2 / nmodes) around the table; 5 of those units are asserted on bins with nmodes >= 100 (the measured maximum is 2.3; a wrong
weight or a wrong V / N^2 shows as tens)."""
import ctypes

import numpy as np
import pytest

import emu_util
import power_oracle as po
from power_oracle import C64, C128
from randomfield_amd import powertools

SPACING = 2.5
SHAPES = [(4, 6, 8), (6, 4, 12), (16, 16, 16)]
_c_dp = ctypes.POINTER(ctypes.c_double)


@pytest.fixture(scope="module")
def lib():
    lib = emu_util.lib()
    lib.emu_measure_power.argtypes = [ctypes.c_int] * 5 + [_c_dp] * 3 + [ctypes.c_void_p, _c_dp, ctypes.c_int,
                                                                        ctypes.POINTER(ctypes.c_ulonglong), _c_dp, _c_dp]
    lib.emu_measure_power.restype = ctypes.c_int
    return lib


def emu_power(lib, data, shape, edges, packed=False, spacing=SPACING):
    nx, ny, nz = shape
    tabs = [np.ascontiguousarray(t, np.float64) for t in powertools.ksq_axes(nx, ny, nz, spacing)]
    edges = np.ascontiguousarray(edges, np.float64)
    nbins = len(edges) - 1
    count, sum_k, sum_p = np.full(nbins, 7, np.uint64), np.full(nbins, np.nan), np.full(nbins, np.nan)
    data = np.ascontiguousarray(data)
    assert data.shape == (nx, ny, nz // 2 + (0 if packed else 1))
    rc = lib.emu_measure_power(int(data.dtype == C128), nx, ny, nz, int(packed), *[t.ctypes.data_as(_c_dp) for t in tabs],
                               data.ctypes.data_as(ctypes.c_void_p), edges.ctypes.data_as(_c_dp), nbins,
                               count.ctypes.data_as(ctypes.POINTER(ctypes.c_ulonglong)), sum_k.ctypes.data_as(_c_dp), sum_p.ctypes.data_as(_c_dp))
    assert rc == 0
    return count, sum_k, sum_p


def edge_sets(shape):
    """16 linear bins over the whole range, and 12 log-spaced bins strictly inside it (cells fall off both ends)"""
    k_min, k_max = powertools.grid_k_range(shape, SPACING)
    return [powertools.default_k_edges(shape, SPACING, 16), np.geomspace(1.7 * k_min, 0.8 * k_max, 13)]


def total_weight(shape):
    return int(po.weights(shape).sum()) - 1


@pytest.mark.parametrize("dtype", [C64, C128], ids=po.ids)
@pytest.mark.parametrize("shape", SHAPES, ids=po.ids)
def test_bin_power_against_the_oracle(shape, dtype):
    data = po.spectrum(shape, dtype)
    for edges in edge_sets(shape):
        want = po.oracle(data, shape, SPACING, edges)
        got = powertools.bin_power(data, SPACING, edges)
        po.assert_sums(got, want, "bin_power")
        assert int(got[0].sum()) + want[3] == total_weight(shape)
    # the default edges cover every mode but DC: nothing is dropped
    assert int(powertools.bin_power(data, SPACING, powertools.default_k_edges(shape, SPACING))[0].sum()) == total_weight(shape)


@pytest.mark.parametrize("dtype", [C64, C128], ids=po.ids)
@pytest.mark.parametrize("shape", SHAPES, ids=po.ids)
def test_emulator_api_layout_against_the_oracle(lib, shape, dtype):
    data = po.spectrum(shape, dtype)
    for edges in edge_sets(shape):
        want = po.oracle(data, shape, SPACING, edges)
        got = emu_power(lib, data, shape, edges)
        po.assert_sums(got, want, "emulator")
        assert int(got[0].sum()) + want[3] == total_weight(shape)
        again = emu_power(lib, data, shape, edges)
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two calls differ"


@pytest.mark.parametrize("dtype", [C64, C128], ids=po.ids)
@pytest.mark.parametrize("shape", SHAPES, ids=po.ids)
def test_emulator_packed_layout_equals_api_layout(lib, shape, dtype):
    data = po.spectrum(shape, dtype)
    W = po.pack(data)                      # kz = 0 slot: A0 + i A_nyq, rounded to the dtype
    seen = po.unpack(W)                    # what the unpack formula gives back in that dtype: `data` up to that rounding
    eps = np.finfo(W.real.dtype).eps
    assert np.max(np.abs(seen - data)) <= 4 * eps * np.max(np.abs(data))
    for edges in edge_sets(shape):
        api = emu_power(lib, seen, shape, edges)
        got = emu_power(lib, W, shape, edges, packed=True)
        po.assert_sums(got, api, "packed vs API layout")
        po.assert_sums(got, po.oracle(seen, shape, SPACING, edges), "packed vs oracle")
        if dtype == C128:                  # (float64: the rounding of the packing itself is far below the tolerance)
            po.assert_sums(got, po.oracle(data, shape, SPACING, edges), "packed vs the original spectrum")
        again = emu_power(lib, W, shape, edges, packed=True)
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two calls differ"


def _exact_edge_cell(shape):
    """a cell whose k^2 is the exact square of a float64: an edge there puts e * e exactly on the cell"""
    k2 = po.k2_grid(shape, SPACING)
    root = np.sqrt(k2)
    hits = np.argwhere((root * root == k2) & (k2 > 0) & (k2 < k2.max()))
    assert len(hits)
    return tuple(hits[len(hits) // 2]), k2


def test_cell_on_a_squared_edge_goes_to_the_upper_bin(lib):
    shape = (16, 16, 16)
    data = po.spectrum(shape, C128)
    cell, k2 = _exact_edge_cell(shape)
    e = float(np.sqrt(k2[cell]))
    edges = np.array([0.0, e, 2.0 * np.sqrt(k2.max())])
    on_edge = k2 == k2[cell]
    want = po.oracle(data, shape, SPACING, edges)
    # the oracle itself puts the cells with k^2 == e^2 into bin 1
    w = po.weights(shape)
    assert int(want[0][0]) == int(w[(k2 < e * e)].sum()) - 1 and int(want[0][1]) == int(w[k2 >= e * e].sum()) and on_edge.sum() >= 1
    for got in (powertools.bin_power(data, SPACING, edges), emu_power(lib, data, shape, edges)):
        po.assert_sums(got, want, "edge cell")
    # ... and one ulp more moves exactly those cells down
    edges2 = edges.copy()
    edges2[1] = np.nextafter(e, np.inf)
    moved = emu_power(lib, data, shape, edges2)
    assert int(moved[0][0]) - int(want[0][0]) == int(w[on_edge].sum())


def test_cells_outside_the_edges_and_dc_are_dropped(lib):
    shape = (6, 4, 12)
    data = po.spectrum(shape, C64)
    data[0, 0, 0] = 1e6                                  # a huge DC value must not show anywhere
    k2 = po.k2_grid(shape, SPACING)
    w = po.weights(shape)
    lo, hi = 0.4 * np.sqrt(k2.max()), 0.7 * np.sqrt(k2.max())
    edges = np.array([lo, 0.5 * (lo + hi), hi])
    inside = (k2 >= lo * lo) & (k2 < hi * hi)
    assert (k2[k2 > 0] < lo * lo).any() and (k2 >= hi * hi).any()
    for got in (powertools.bin_power(data, SPACING, edges), emu_power(lib, data, shape, edges)):
        assert int(got[0].sum()) == int(w[inside].sum())
        po.assert_sums(got, po.oracle(data, shape, SPACING, edges), "inner edges")
    # edges[0] = 0: k^2 = 0 lies in bin 0 by the rule, and is dropped because it is the DC cell
    edges0 = np.array([0.0, 2.0 * np.sqrt(k2.max())])
    for got in (powertools.bin_power(data, SPACING, edges0), emu_power(lib, data, shape, edges0)):
        assert int(got[0][0]) == total_weight(shape)
        p = data.real.astype(np.float64) ** 2 + data.imag.astype(np.float64) ** 2
        p[0, 0, 0] = 0.0                                 # (left out before the sum: subtracting 1e12 afterwards would cancel)
        want_p = float((w * p).sum())
        assert abs(got[2][0] - want_p) <= po.RTOL * want_p


def test_one_bin_and_1024_bins(lib):
    shape = (16, 16, 16)
    data = po.spectrum(shape, C64)
    k_min, k_max = powertools.grid_k_range(shape, SPACING)
    for nbins in (1, 1024):
        edges = powertools.default_k_edges(shape, SPACING, nbins)
        assert len(edges) == nbins + 1
        want = po.oracle(data, shape, SPACING, edges)
        for got in (powertools.bin_power(data, SPACING, edges), emu_power(lib, data, shape, edges)):
            po.assert_sums(got, want, "%d bins" % nbins)
            assert int(got[0].sum()) == total_weight(shape)
        res = powertools.power_estimate(*want[:3], shape=shape, spacing=SPACING)
        empty = want[0] == 0
        assert res.dtype.names == ("k", "Pk", "nmodes")
        assert np.all(np.isnan(res["k"][empty])) and np.all(np.isnan(res["Pk"][empty]))
        assert np.all(np.isfinite(res["k"][~empty])) and np.all(np.isfinite(res["Pk"][~empty]))
        assert np.all((res["k"][~empty] >= edges[:-1][~empty]) & (res["k"][~empty] < edges[1:][~empty]))
        if nbins == 1024:
            assert empty.sum() > 100           # (969 distinct |k| at most on a 16^3 grid)
    with pytest.raises(ValueError):
        powertools.default_k_edges(shape, SPACING, 1025)
    for bad in ([0.1, 0.1, 0.2], [-0.1, 0.2], [0.3, 0.2], [0.1]):
        with pytest.raises(ValueError):
            powertools.bin_power(data, SPACING, bad)


@pytest.mark.parametrize("shape,seed", [((32, 32, 32), 123), ((40, 60, 80), 7)], ids=["32x32x32", "40x60x80"])
def test_numpy_generator_recovers_the_input_power(shape, seed):
    from randomfield_amd import Generator
    gen = Generator(*shape, SPACING, backend="numpy")
    field = gen.generate_delta_field(seed=seed, save_potential=False)
    kept = field.copy()
    res = gen.measure_power_spectrum(nbins=16)
    assert res.dtype.names == ("k", "Pk", "nmodes") and len(res) == 16
    assert np.array_equal(gen.plan_c2r.data_out, kept), "the numpy backend must leave the field alone"
    edges = powertools.default_k_edges(shape, SPACING, 16)
    assert int(res["nmodes"].sum()) == total_weight(shape)
    po.assert_matches_table(res, gen.power, shape, SPACING, edges, "numpy %s" % (shape,))
    # an explicit field and explicit edges give the same answer
    res2 = gen.measure_power_spectrum(kept, k_edges=edges)
    assert all(np.array_equal(res[n], res2[n], equal_nan=True) for n in res.dtype.names)
    with pytest.raises(ValueError):
        gen.measure_power_spectrum(kept[:-1])


def test_abi_surface():
    from randomfield_amd import _hip
    assert _hip.FEATURES["power_measure"] == 1 << 15
    assert (_hip.ABI_MAJOR, _hip.ABI_MINOR) == (5, 5)
    assert (_hip.RF_POWER_FROM_KSPACE, _hip.RF_POWER_FROM_FIELD) == (0, 1)
    assert "rf_measure_power" in _hip.SIGNATURES
    _hip.load()
    assert _hip.abi_version() == (5, 5)
    assert "power_measure" in _hip.abi_features()
    assert hasattr(_hip.DevicePlan, "measure_power")
