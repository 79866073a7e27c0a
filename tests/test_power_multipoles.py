"""The power spectrum multipole estimator (csrc/rf_core.h multipole_cell) without a GPU: the oracle of tests/multipole_oracle.py checked
against identities it does not share code with; powertools.bin_multipoles and the emulator's emu_measure_multipoles -- the cell
function the device sweep runs, over the API and the packed layout -- against that oracle; window_compensation, multipole_estimate;
redshift-space displacements and the Kaiser signature on the numpy backend; the ABI surface (version 5.5 unchanged, feature bit 18).

Tolerances.  Counts are integers and must be exact.  sum_k, m0, m2, m4 are sums of non-negative float64 terms, each term a handful of
roundings: the error is at most (n + 8) 2^-53 relative for the < 1e5 cells here, rtol 1e-9 (power_oracle.RTOL) is far above it.  The
oracle's identities hold to 1e-12 (measured <= 7e-15).  The Kaiser check is no precision test: linear theory for f = 1 gives
P2 / P0 = (4/3 + 4/7) / (1 + 2/3 + 1/5) = 1.02 along the shifted axis and -0.51 across it; the asserted ranges [0.8, 1.3] and
[-0.75, -0.25] tell the three axes, the sign and the Legendre factors apart (measured over seeds 1-3: 0.95 ... 1.19, -0.39 ... -0.60).

Without a GPU no plan exists, so the only argument error rf_measure_multipoles itself can be shown is the null plan; a bad los, bad
edges and a bad table entry are shown to the emulator's entry point and to bin_multipoles, which check them as the library does (the
library's own refusals: tests/test_gpu_power_multipoles.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

import emu_util
import multipole_oracle as mo
import power_oracle as po
from power_oracle import C64, C128
from randomfield_amd import powertools
from test_gpu_power_measure import edge_sets

SPACING = 2.5
CASES = [((16, 16, 16), C64), ((16, 16, 16), C128), ((4, 6, 8), C64), ((30, 14, 22), C64), ((16, 32, 64), C64)]
SHAPES = [(16, 16, 16), (4, 6, 8), (30, 14, 22), (16, 32, 64)]
_c_dp = ctypes.POINTER(ctypes.c_double)
_c_up = ctypes.POINTER(ctypes.c_ulonglong)


@pytest.fixture(scope="module")
def lib():
    lib = emu_util.lib()
    lib.emu_measure_multipoles.argtypes = [ctypes.c_int] * 6 + [_c_dp] * 3 + [ctypes.c_void_p, _c_dp, ctypes.c_int] + [_c_dp] * 3 + [_c_up] + [_c_dp] * 4
    lib.emu_measure_multipoles.restype = ctypes.c_int
    return lib


def emu_multipoles(lib, data, shape, edges, los, comp=None, packed=False, expect=0):
    nx, ny, nz = shape
    tabs = [np.ascontiguousarray(t, np.float64) for t in powertools.ksq_axes(nx, ny, nz, SPACING)]
    edges = np.ascontiguousarray(edges, np.float64)
    nbins = len(edges) - 1
    count = np.full(max(nbins, 1), 7, np.uint64)
    sums = [np.full(max(nbins, 1), np.nan) for _ in range(4)]
    data = np.ascontiguousarray(data)
    assert data.shape == (nx, ny, nz // 2 + (0 if packed else 1))
    comp = [None] * 3 if comp is None else [None if t is None else np.ascontiguousarray(t, np.float64) for t in comp]
    rc = lib.emu_measure_multipoles(int(data.dtype == C128), nx, ny, nz, int(packed), int(los), *[t.ctypes.data_as(_c_dp) for t in tabs],
                                    data.ctypes.data_as(ctypes.c_void_p), edges.ctypes.data_as(_c_dp), nbins,
                                    *[None if t is None else t.ctypes.data_as(_c_dp) for t in comp],
                                    count.ctypes.data_as(_c_up), *[s.ctypes.data_as(_c_dp) for s in sums])
    assert rc == expect
    return (count,) + tuple(sums)


# ---- the oracle is not its own judge --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=po.ids)
def test_oracle_identities(shape):
    field = np.random.RandomState(8).normal(size=shape)
    kdata = np.fft.rfftn(field, axes=(0, 1, 2))
    for edges in edge_sets(shape):
        plain = po.oracle(kdata, shape, SPACING, edges)
        per_los = [mo.oracle(kdata, shape, SPACING, edges, los) for los in range(3)]
        for got in per_los:
            assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1])
            assert np.array_equal(got[2], plain[2]), "m0 without compensation is power_oracle's sum_p, bit for bit"
            assert got[5] == plain[3]
        m0 = per_los[0][2]
        total = per_los[0][3] + per_los[1][3] + per_los[2][3]            # mu_x^2 + mu_y^2 + mu_z^2 = 1
        assert np.all(np.abs(total - m0) <= 1e-12 * m0)
        for los in range(3):                                             # the half-spectrum weights against the full cube, weight 1 per mode
            f0, f2, f4 = mo.full_cube(field, SPACING, edges, los)
            for name, half, full in (("m0", per_los[los][2], f0), ("m2", per_los[los][3], f2), ("m4", per_los[los][4], f4)):
                err = float(np.max(np.abs(half - full) / np.where(full > 0, full, 1.0)))
                print("%s los %d %s: half spectrum vs full cube %.2e" % (shape, los, name, err))
                assert err <= 1e-12


# ---- bin_multipoles and the emulator against the oracle -----------------------------------------------------------------------
@pytest.mark.parametrize("shape,dtype", CASES, ids=po.ids)
def test_bin_multipoles_against_the_oracle(shape, dtype):
    data = po.spectrum(shape, dtype)
    for comp in (None, mo.random_tables(shape)):
        for edges in edge_sets(shape):
            for los in range(3):
                want = mo.oracle(data, shape, SPACING, edges, los, comp)
                got = powertools.bin_multipoles(data, SPACING, edges, los, comp)
                mo.assert_sums(got, want, "bin_multipoles los %d" % los)
    # one table alone: the two others are ones
    only_y = (None, mo.random_tables(shape)[1], None)
    edges = edge_sets(shape)[0]
    mo.assert_sums(powertools.bin_multipoles(data, SPACING, edges, 1, only_y), mo.oracle(data, shape, SPACING, edges, 1, only_y), "one table")
    # null tables: count, sum_k, m0 are bin_power's (which takes the reference's shapes alone: nz a multiple of 4)
    if shape[2] % 4 == 0:
        plain = powertools.bin_power(data, SPACING, edges)
        got = powertools.bin_multipoles(data, SPACING, edges, 0)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], plain))


@pytest.mark.parametrize("shape,dtype", CASES, ids=po.ids)
def test_emulator_against_the_oracle(lib, shape, dtype):
    data = po.spectrum(shape, dtype)
    W = po.pack(data)
    seen = po.unpack(W)                    # what the unpack formula gives back in that dtype: the packed sweep must see this
    for comp in (None, mo.random_tables(shape)):
        for edges in edge_sets(shape):
            for los in range(3):
                want = mo.oracle(data, shape, SPACING, edges, los, comp)
                got = emu_multipoles(lib, data, shape, edges, los, comp)
                mo.assert_sums(got, want, "emulator los %d" % los)
                again = emu_multipoles(lib, data, shape, edges, los, comp)
                assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two calls differ"
                packed = emu_multipoles(lib, W, shape, edges, los, comp, packed=True)
                mo.assert_sums(packed, mo.oracle(seen, shape, SPACING, edges, los, comp), "emulator packed los %d" % los)
    # null tables: count, sum_k and m0 are emu_measure_power's, term for term
    import test_power_measure as tpm
    lib.emu_measure_power.argtypes = [ctypes.c_int] * 5 + [_c_dp] * 3 + [ctypes.c_void_p, _c_dp, ctypes.c_int, _c_up, _c_dp, _c_dp]
    lib.emu_measure_power.restype = ctypes.c_int
    for edges in edge_sets(shape):
        plain = tpm.emu_power(lib, data, shape, edges)
        got = emu_multipoles(lib, data, shape, edges, 2)
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], plain)), "null tables: not power_cell's terms"


def test_argument_errors_without_a_device(lib):
    shape = (4, 6, 8)
    data = po.spectrum(shape, C64)
    edges = edge_sets(shape)[0]
    good = mo.random_tables(shape)
    emu_multipoles(lib, data, shape, edges, 0, good)
    for los in (-1, 3):
        emu_multipoles(lib, data, shape, edges, los, expect=-1)
        with pytest.raises(ValueError):
            powertools.bin_multipoles(data, SPACING, edges, los)
    for bad in ([0.1, 0.1, 0.2], [-0.1, 0.2], [0.3, 0.2]):
        emu_multipoles(lib, data, shape, bad, 0, expect=-1)
        with pytest.raises(ValueError):
            powertools.bin_multipoles(data, SPACING, bad, 0)
    for axis in range(3):
        for value in (0.0, -1.0, np.nan, np.inf):
            tabs = [t.copy() for t in good]
            tabs[axis][-1] = value
            emu_multipoles(lib, data, shape, edges, 0, tabs, expect=-1)
            with pytest.raises(ValueError):
                powertools.bin_multipoles(data, SPACING, edges, 0, tabs)
    with pytest.raises(ValueError):
        powertools.bin_multipoles(data, SPACING, edges, 0, (good[0][:-1], good[1], good[2]))


# ---- window compensation and the Legendre combinations ------------------------------------------------------------------------
@pytest.mark.parametrize("scheme,p", [("ngp", 1), ("cic", 2), ("tsc", 3)])
def test_window_compensation(scheme, p):
    for n in (8, 22, 64):
        tabs = powertools.window_compensation((n, n, n), scheme)
        assert [len(t) for t in tabs] == [n, n, n // 2 + 1] and all(t.dtype == np.float64 for t in tabs)
        m = np.arange(n)
        m = np.where(m > n // 2, m - n, m).astype(np.float64)            # signed frequency index, written out
        x = np.pi * m / n
        sinc = np.ones(n)
        sinc[1:] = np.sin(x[1:]) / x[1:]
        window = sinc ** (2 * p)
        for t in tabs:
            assert np.all(np.abs(t * window[:len(t)] - 1.0) <= 1e-14)
            assert np.all(np.isfinite(t)) and t[0] == 1.0
            assert abs(t[n // 2] - (np.pi / 2) ** (2 * p)) <= 1e-14 * t[n // 2]
    tabs = powertools.window_compensation((8, 22, 64), scheme)
    assert [len(t) for t in tabs] == [8, 22, 33]
    for wrong in ("pcs", "CIC", None, 2):
        with pytest.raises(ValueError):
            powertools.window_compensation((8, 8, 8), wrong)


def test_multipole_estimate():
    shape, spacing = (8, 8, 8), 2.0
    norm = spacing ** 3 / 512.0
    count = np.array([4, 0, 10, 2], np.uint64)
    sum_k = np.array([2.0, 0.0, 7.0, 3.0])
    m0 = np.array([8.0, 0.0, 30.0, 5.0])
    # bin 0: isotropic (M2 = M0 / 3, M4 = M0 / 5); bin 2: all power along the line of sight (mu = 1); bin 3: all across it (mu = 0)
    m2 = np.array([8.0 / 3.0, 0.0, 30.0, 0.0])
    m4 = np.array([8.0 / 5.0, 0.0, 30.0, 0.0])
    res = powertools.multipole_estimate(count, sum_k, m0, m2, m4, shape=shape, spacing=spacing)
    assert res.dtype.names == ("k", "P0", "P2", "P4", "nmodes")
    assert np.array_equal(res["nmodes"], count)
    assert all(np.isnan(res[n][1]) for n in ("k", "P0", "P2", "P4"))
    assert res["k"][0] == 0.5 and res["k"][2] == 0.7 and res["k"][3] == 1.5
    assert np.allclose(res["P0"][[0, 2, 3]], norm * np.array([2.0, 3.0, 2.5]), rtol=1e-15)
    assert abs(res["P2"][0]) <= 1e-15 * res["P0"][0] and abs(res["P4"][0]) <= 1e-14 * res["P0"][0]
    # L2(1) = L4(1) = 1 with the (2l + 1) factors 5 and 9; L2(0) = -1/2, L4(0) = 3/8
    assert np.isclose(res["P2"][2], 5.0 * res["P0"][2], rtol=1e-14) and np.isclose(res["P4"][2], 9.0 * res["P0"][2], rtol=1e-14)
    assert np.isclose(res["P2"][3], -2.5 * res["P0"][3], rtol=1e-14) and np.isclose(res["P4"][3], 27.0 / 8.0 * res["P0"][3], rtol=1e-14)
    # P0 is power_estimate's Pk
    assert np.array_equal(res["P0"], powertools.power_estimate(count, sum_k, m0, shape=shape, spacing=spacing)["Pk"], equal_nan=True)


# ---- the Generator on the numpy backend ----------------------------------------------------------------------------------------
def kaiser_edges():
    edges = np.linspace(0, 0.5 * np.pi / 10.0, 5)
    edges[0] = 1e-9
    return edges


def quadrupole_ratio(res):
    """P2 / P0 of the bins' summed moments (P0 and P2 are linear in them: sums weighted by the number of modes)"""
    n = res["nmodes"].astype(np.float64)
    return float((n * res["P2"]).sum() / (n * res["P0"]).sum())


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_kaiser_quadrupole_numpy(axis):
    from randomfield_amd import Generator
    gen = Generator(32, 32, 32, 10.0, backend="numpy")
    gen.generate_delta_field(seed=1)
    gen.particle_displacements(order=2, D1=0.1, rsd_axis=axis, f1=1.0, f2=1.0)
    gen.paint_particles()
    for los in range(3):
        res = gen.measure_power_multipoles(los=los, k_edges=kaiser_edges())
        assert int(res["nmodes"].sum()) == 2102
        ratio = quadrupole_ratio(res)
        print("shift along %d, measured along %d: P2 / P0 = %.3f" % (axis, los, ratio))
        if los == axis:
            assert 0.8 <= ratio <= 1.3
        else:
            assert -0.75 <= ratio <= -0.25


def test_displacement_defaults_and_the_shifted_axis():
    from randomfield_amd import Generator
    gen = Generator(16, 16, 16, SPACING, backend="numpy")
    gen.generate_delta_field(seed=3)
    rt = gen.plan_c2r.data_out.dtype.type
    D1 = 0.7
    psi1 = [gen.calculate_displacement_field(a, order=1).copy() for a in range(3)]
    psi2 = [gen.calculate_displacement_field(a, order=2).copy() for a in range(3)]
    for order in (1, 2):
        plain = gen.particle_displacements(order=order, D1=D1)
        # what the method returned before it knew rsd_axis
        for a in range(3):
            before = rt(D1) * psi1[a]
            if order == 2:
                before += rt(D1 * D1) * psi2[a]
            assert np.array_equal(plain[a], before)
        assert np.array_equal(gen.particle_displacements(order=order, D1=D1, rsd_axis=0, f1=0.0), plain)
        for axis in range(3):
            got = gen.particle_displacements(order=order, D1=D1, rsd_axis=axis, f1=0.5, f2=0.8)
            want = rt(D1 * 1.5) * psi1[axis]
            if order == 2:
                want += rt(D1 * D1 * 1.8) * psi2[axis]
            assert np.array_equal(got[axis], want)
            for other in set(range(3)) - {axis}:
                assert np.array_equal(got[other], plain[other])
        # f2 = None means 2 f1
        assert np.array_equal(gen.particle_displacements(order=order, D1=D1, rsd_axis=1, f1=0.4),
                              gen.particle_displacements(order=order, D1=D1, rsd_axis=1, f1=0.4, f2=0.8))
    with pytest.raises(ValueError):
        gen.particle_displacements(rsd_axis=3)


def test_generator_numpy_window_and_los():
    from randomfield_amd import Generator
    shape = (16, 16, 16)
    gen = Generator(*shape, SPACING, backend="numpy")
    field = gen.generate_delta_field(seed=5, save_potential=False).copy()
    edges = powertools.default_k_edges(shape, SPACING, 8)
    kdata = np.fft.rfftn(field.astype(np.float64), axes=(0, 1, 2))
    plain = gen.measure_power_spectrum(field, k_edges=edges)
    for los in range(3):
        res = gen.measure_power_multipoles(field, los=los, k_edges=edges)
        assert res.dtype.names == ("k", "P0", "P2", "P4", "nmodes")
        assert np.array_equal(res["P0"], plain["Pk"]) and np.array_equal(res["k"], plain["k"]) and np.array_equal(res["nmodes"], plain["nmodes"])
        want = powertools.multipole_estimate(*mo.oracle(kdata, shape, SPACING, edges, los)[:5], shape=shape, spacing=SPACING)
        for name in ("P0", "P2", "P4"):
            assert np.all(np.abs(res[name] - want[name]) <= 1e-9 * want["P0"])
    # a scheme name and the tables it stands for; measure_power_spectrum(window=) is the compensated monopole
    tabs = powertools.window_compensation(shape, "cic")
    by_name = gen.measure_power_multipoles(field, los=2, k_edges=edges, window="cic")
    by_tabs = gen.measure_power_multipoles(field, los=2, k_edges=edges, window=tabs)
    assert all(np.array_equal(by_name[n], by_tabs[n]) for n in by_name.dtype.names)
    want = mo.oracle(kdata, shape, SPACING, edges, 2, tabs)
    comp = gen.measure_power_spectrum(field, k_edges=edges, window="cic")
    assert comp.dtype.names == ("k", "Pk", "nmodes")
    assert np.array_equal(comp["Pk"], by_name["P0"]) and np.array_equal(comp["nmodes"], want[0])
    assert np.all(np.abs(comp["Pk"] / powertools.multipole_estimate(*want[:5], shape=shape, spacing=SPACING)["P0"] - 1.0) <= 1e-9)
    assert np.all(comp["Pk"] > plain["Pk"])                   # every factor is >= 1, and > 1 away from the axes' DC entries
    with pytest.raises(ValueError):
        gen.measure_power_multipoles(field, los=3)
    with pytest.raises(ValueError):
        gen.measure_power_multipoles(field, window="pcs")
    with pytest.raises(ValueError):
        gen.measure_power_multipoles(field, window=(tabs[0], tabs[1], -tabs[2]))


# ---- ABI and header -----------------------------------------------------------------------------------------------------------------
def test_abi_surface():
    from randomfield_amd import _hip
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "randomfield_hip.h")).read()
    assert re.search(r"RF_FEATURE_POWER_MULTIPOLES\s*=\s*1\s*<<\s*18\b", header)
    assert re.search(r"\bint\s+rf_measure_multipoles\s*\(", header)
    assert _hip.FEATURES["power_multipoles"] == 1 << 18
    assert (_hip.ABI_MAJOR, _hip.ABI_MINOR) == (5, 5)
    assert "rf_measure_multipoles" in _hip.SIGNATURES
    lib = _hip.load()
    assert lib.rf_version() == (5 << 16) | 5
    assert lib.rf_abi_features() & (1 << 18)
    assert _hip.abi_version() == (5, 5)
    assert "power_multipoles" in _hip.abi_features()
    assert hasattr(_hip.DevicePlan, "measure_multipoles")


def test_null_plan_is_refused_with_a_message():
    from randomfield_amd import _hip
    lib = _hip.load()
    edges = np.array([0.1, 0.2, 0.3])
    count = np.zeros(2, np.uint64)
    sums = [np.zeros(2) for _ in range(4)]
    rc = lib.rf_measure_multipoles(None, _hip.RF_POWER_FROM_KSPACE, 2, edges.ctypes.data_as(_c_dp), 2, None, None, None,
                                   count.ctypes.data_as(_c_up), *[s.ctypes.data_as(_c_dp) for s in sums])
    assert rc != 0
    assert "null plan" in _hip.last_error()
    with pytest.raises(RuntimeError, match="null plan"):
        _hip.check(rc, "rf_measure_multipoles")
