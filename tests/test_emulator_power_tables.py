"""The generation pass on user power tables (tests/power_tables.py), on the CPU emulator: the exact chain (emu_util.realise,
generate_kspace), the fast float32 chain (realise_fast) and the fast lookup alone (fast_sigma) against the float64 oracle of the same
Philox stream, over tables that reach what the default power never does -- guard bins, 256 / 512 records, the fall-back, 2 rows, a zero
run, edges inside the grid, and cells ON a table edge.

The last is what these tests were written for.  A table that ends exactly on cpu_ref.k_bounds passes the reference's coverage check
with the fundamental and corner modes on its edges; before the edge rule (csrc/rf_core.h RF_EDGE_TOL) the last bit of log10|k| decided
whether those modes exist, differently in the oracle, the exact chain and the fast chain.  Seed 7, native noise, complex64, field error
over rms against the oracle WITHOUT the rule:

    shape, spacing          fast       exact      cells the reference zeroes
    64^3, 2.5               1.2e-5     0.219      7 (DC, fundamentals kept or dropped, corner)
    32 x 16 x 64, 2.5       4e-6       0.247      3
    16 x 32 x 64, 10.0      4e-6       2.6e-3     2
    32^3, 1.0               0.384      0.384      7
    64^3, 2.5, control      1.2e-5     1.2e-5     1 (DC)

Against the oracle WITH the rule (what this file asserts) the C++ sources from before the rule fail 29 of the 69 tests here that do
not ask for declined records: the exact chain's field on hug at the five shapes below by 1.9e-4, 1.6e-3, 9.5e-2, 6.3e-4 and 8.2e-3 rms
(hug2 and the two clustered tables alike), all eight (n, spacing) pairs of the lookup test, and the margin test (sigma 0 where the
edge row's is due).  On an MI355X the
fast kernel before the rule was 0.13 rms (spacing 2.5), 0.26 (1.0), 0.34 (0.7) and 0.027 (10.0) away from today's field on hug at
(64, 32, 128), the exact kernel 0, 0.26, 0.34 and 1.2e-4.

Bounds -- the emulator's own, none new.  Native noise: 2e-5 rms for both chains (test_emulator.py
test_fast_native_generation_matches_oracle: the float32 Box-Muller of libm's sinf / cosf dominates, and both chains of a float32 plan
form their deviates with it; the GPU tests hold the hardware's to 1e-5).  Host deviates through the exact chain: 3e-6 rms, k space
within 5e-7 (complex64) of the largest magnitude (test_generation_and_fused_realisation).  Native k space: 2e-6
(test_native_noise_matches_oracle_philox).  The fast lookup alone: 1e-6 relative (test_fast_sigma_lookup_error_bound).  The defect's
signature is >= 2.6e-3 rms.  Every check prints measured / bound."""
import numpy as np
import pytest

import emu_util
import power_tables as pt
from oracle import cpu_ref

ROWS = [((64, 64, 64), 2.5), ((32, 16, 64), 2.5), ((16, 32, 64), 10.0), ((32, 32, 32), 1.0), ((16, 16, 16), 2.5)]
EDGE_PAIRS = [(64, 2.5), (256, 0.7), (32, 3.3), (64, 10.0), (512, 0.1), (128, 1.0), (16, 2.5), (1024, 2.5)]
# the tiled GPU shapes of tests/test_gpu_power_tables.py: the builders' guards are verified here for them too
GPU_CASES = [((64, 32, 128), 2.5), ((64, 32, 128), 1.0), ((64, 32, 128), 0.7), ((64, 32, 128), 10.0), ((512, 16, 64), 2.5),
             ((1024, 8, 32), 2.5), ((2048, 8, 32), 2.5), ((1024, 8, 16), 2.5), ((40, 60, 80), 2.5)]
SEED = 7
TOL_NATIVE = 2e-5        # * rms
TOL_HOST = 3e-6          # * rms
KTOL_NATIVE = 2e-6       # * max|k space|
KTOL_HOST = 5e-7
NB = {"control": 126, "hug": 128, "hug2": 128, "clustered256": 256, "clustered512": 512, "band_low": 127, "band_pass": 128}


def _id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def report(what, measured, bound):
    print("%-58s %.3e / %.1e" % (what, measured, bound))
    assert measured <= bound, "%s: %.3e > %.1e" % (what, measured, bound)


def records(shape, spacing, k, Pk):
    """number of records the fast lookup needs for the table (guard bins included)"""
    xt, st = pt.sigma_table(k, Pk, shape, spacing)
    x, _ = pt.mode_log10k(shape, spacing)
    return emu_util.fast_sigma(xt, st, *pt.grid_range(shape, spacing), (10.0 ** (2 * x[:4])).astype(np.float32))[2]


@pytest.mark.parametrize("shape,spacing", ROWS + GPU_CASES, ids=_id)
def test_builders_reach_the_regimes_they_are_named_for(shape, spacing):
    """bin counts (emu_util.fast_sigma's nb), the fall-back, the clearance of every inner edge and the share of cells a band table cuts"""
    for name in pt.TABLES:
        try:
            k, Pk = pt.build(name, shape, spacing)
        except pt.NoClearEdge:
            # the squares of a 2048-point axis leave no gap of 2.2e-4 dex with 10 % - 90 % of the cells beyond it
            assert name.startswith("band") and shape == (2048, 8, 32), (name, shape)
            continue
        assert np.all(np.diff(k) > 0) and np.all(Pk >= 0)
        nb = records(shape, spacing, k, Pk)
        print("%-13s %4d rows, %5d records" % (name, len(k), nb))
        if name == "dense":
            assert nb > 512                                             # rf_capi.hip build_fast declines: the exact kernel
        elif name == "kinked":
            assert nb <= 512 and np.count_nonzero(Pk == 0) == 3 and Pk[0] > 0 and Pk[-1] > 0
        else:
            assert nb == NB[name], (name, nb)
        kmin, kmax = cpu_ref.k_bounds(*shape, spacing)
        if name in ("hug", "hug2", "clustered256", "clustered512"):
            assert k[0] == kmin and k[-1] == kmax
        if name.startswith("band"):
            assert k[-1] < kmax and (name == "band_low" or k[0] > kmin)
            pt.assert_clear(shape, spacing, [k[-1]] + ([k[0]] if name == "band_pass" else []))
            assert 0.10 <= pt.outside_fraction(shape, spacing, k) <= 0.90
            with pytest.raises(ValueError):
                cpu_ref.sigma_table(k, Pk, *shape, spacing)
        else:
            cpu_ref.sigma_table(k, Pk, *shape, spacing)                 # the reference's coverage check accepts it


@pytest.mark.parametrize("name", pt.TABLES)
@pytest.mark.parametrize("shape,spacing", ROWS, ids=_id)
def test_both_chains_against_the_oracle(shape, spacing, name):
    nx, ny, nz = shape
    k, Pk = pt.build(name, shape, spacing)
    xt, st = pt.sigma_table(k, Pk, shape, spacing)
    noise = cpu_ref.native_noise(SEED, nx, ny, nz, np.complex64)
    kref, ref, rms = pt.oracle_field(shape, spacing, k, Pk, noise)
    assert rms > 0
    if name in ("control", "dense"):                                    # no cell near an edge: the rule changes nothing
        assert np.array_equal(kref, pt.oracle_kspace(shape, spacing, k, Pk, noise, edge_tol=0.0))
    if name in pt.COVERING:                                             # ... and cpu_ref's own entry point is the same oracle
        assert np.array_equal(kref, cpu_ref.generate_kspace(nx, ny, nz, spacing, k, Pk, noise=noise, edge_tol=cpu_ref.EDGE_TOL))
    n = ref.size

    out, s1, s2 = emu_util.realise(nx, ny, nz, spacing, xt, st, seed=SEED)
    report("%s exact, native: field" % name, np.max(np.abs(out - ref)) / rms, TOL_NATIVE)
    report("%s exact, native: rms" % name, abs(np.sqrt(s2 / n - (s1 / n) ** 2) - rms) / rms, TOL_NATIVE)

    ks = emu_util.generate_kspace(nx, ny, nz, spacing, xt, st, seed=SEED)
    report("%s exact, native: k space" % name, np.max(np.abs(ks - kref)) / np.max(np.abs(kref)), KTOL_NATIVE)
    assert np.array_equal(ks == 0, kref == 0), "%d cells are zero on one side only" % np.count_nonzero((ks == 0) != (kref == 0))

    if pt.expected_path(name) == "fast":
        out, s1, s2 = emu_util.realise_fast(nx, ny, nz, spacing, xt, st, seed=SEED)
        report("%s fast, native: field" % name, np.max(np.abs(out - ref)) / rms, TOL_NATIVE)
        report("%s fast, native: rms" % name, abs(np.sqrt(s2 / n - (s1 / n) ** 2) - rms) / rms, TOL_NATIVE)
    else:
        assert records(shape, spacing, k, Pk) > 512

    hnoise = cpu_ref.reference_noise(SEED, nx * ny * (nz // 2 + 1))
    kref, ref, rms = pt.oracle_field(shape, spacing, k, Pk, hnoise)
    out, s1, s2 = emu_util.realise(nx, ny, nz, spacing, xt, st, noise=hnoise)
    report("%s exact, host deviates: field" % name, np.max(np.abs(out - ref)) / rms, TOL_HOST)
    ks = emu_util.generate_kspace(nx, ny, nz, spacing, xt, st, noise=hnoise)
    report("%s exact, host deviates: k space" % name, np.max(np.abs(ks - kref)) / np.max(np.abs(kref)), KTOL_HOST)
    assert np.array_equal(ks == 0, kref == 0)


def kernel_k2(n, spacing, ix, iy, iz):
    """|k|^2 of cell (signed indices) as the fast kernels form it (rf_core.h fast_kxy2 / fast_k2): float32 dk * index per axis, then
    fmaf(kx, kx, ky * ky) and fmaf(kz, kz, kxy) -- the products are exact in extended precision, so one rounding each is the fma"""
    f32, ld = np.float32, np.longdouble
    dk = f32(np.sqrt(cpu_ref.ksq_axes(n, n, n, spacing)[0][1]))        # (float)sqrt(kx2[1]), rf_capi.hip build_fast
    kx, ky, kz = f32(f32(ix) * dk), f32(f32(iy) * dk), f32(f32(iz) * dk)
    kxy = f32(ld(kx) * ld(kx) + ld(f32(ky * ky)))
    return f32(ld(kz) * ld(kz) + ld(kxy))


@pytest.mark.parametrize("n,spacing", EDGE_PAIRS, ids=_id)
def test_lookups_agree_on_a_hugging_edge(n, spacing):
    """The fundamental and corner modes of a cubic grid whose table ends exactly on k_min and k_max: the fast float32 lookup, the
    exact lookup and the oracle all give the edge row's sigma.  Before the rule (64, 2.5), (256, 0.7), (32, 3.3), (64, 10) and
    (512, 0.1) gave 0 on one side and sigma(edge) on the other; (128, 1.0), (16, 2.5) and (1024, 2.5) happened to agree."""
    shape = (n, n, n)
    for name in ("hug", "hug2"):
        k, Pk = pt.build(name, shape, spacing)
        xt, st = pt.sigma_table(k, Pk, shape, spacing)
        h = n // 2
        k2 = np.array([kernel_k2(n, spacing, 1, 0, 0), kernel_k2(n, spacing, 0, -1, 0), kernel_k2(n, spacing, 0, 0, 1),
                       kernel_k2(n, spacing, -h, -h, h)], np.float32)
        want = np.array([st[0], st[0], st[0], st[-1]])
        fast, exact, nb = emu_util.fast_sigma(xt, st, *pt.grid_range(shape, spacing), k2)
        oracle = cpu_ref.interp_sigma(0.5 * np.log10(k2.astype(np.float64)), xt, st, cpu_ref.EDGE_TOL)
        # a chain that places the cell up to 1e-6 dex inside the edge (its own error, see RF_EDGE_TOL) interpolates there
        slope = np.abs(np.array([(st[1] - st[0]) / (xt[1] - xt[0])] * 3 + [(st[-1] - st[-2]) / (xt[-1] - xt[-2])]))
        for what, got in (("fast", fast), ("exact", exact), ("oracle", oracle)):
            assert np.all(got > 0), (what, got)
            report("%s n=%d spacing=%g: %s sigma on the edges" % (name, n, spacing, what),
                   np.max(np.abs(got - want) / (1e-6 * want + 1e-6 * slope)), 1.0)


def test_edge_rule_margin():
    """Outside the table by less than half of EDGE_TOL: the edge row's sigma, in every chain.  Outside by 1e-5 dex or more: 0.  (In
    between the float32 chains may differ: their own error on log10|k| is up to 1e-6 dex, see RF_EDGE_TOL.)"""
    shape, spacing = (64, 64, 64), 2.5
    k, Pk = pt.build("hug", shape, spacing)
    xt, st = pt.sigma_table(k, Pk, shape, spacing)
    near, far = np.array([0.0, 1e-7, 5e-7, 1e-6]), np.array([1e-5, 1e-4, 1e-3, 5e-3])
    for edge, sign, sig in ((xt[0], -1.0, st[0]), (xt[-1], +1.0, st[-1])):
        k2 = (10.0 ** (2 * (edge + sign * np.concatenate([near, far])))).astype(np.float32)
        fast, exact, nb = emu_util.fast_sigma(xt, st, *pt.grid_range(shape, spacing), k2)
        oracle = cpu_ref.interp_sigma(0.5 * np.log10(k2.astype(np.float64)), xt, st, cpu_ref.EDGE_TOL)
        for what, got in (("fast", fast), ("exact", exact), ("oracle", oracle)):
            report("%s: sigma within the margin" % what, np.max(np.abs(got[:near.size] / sig - 1)), 1e-6)
            assert np.all(got[near.size:] == 0), (what, got)
        # inside, next to the edge: the interpolated value, continuous with the edge row's
        k2 = (10.0 ** (2 * (edge - sign * np.array([1e-6, 1e-4])))).astype(np.float32)
        fast, exact, nb = emu_util.fast_sigma(xt, st, *pt.grid_range(shape, spacing), k2)
        report("fast against exact just inside", np.max(np.abs(fast / exact - 1)), 1e-6)
        assert np.all(np.abs(exact / sig - 1) < 1e-3)
    assert np.array_equal(cpu_ref.interp_sigma(np.array([-np.inf, np.nan]), xt, st, cpu_ref.EDGE_TOL), [0.0, 0.0])


def test_records_are_declined_when_the_margin_cannot_be_resolved():
    """build_fast_records bounds the float32 chain's error on log10|k| by 2^-24 (5 max|x| + span) and declines a table that needs
    the margin when that exceeds RF_EDGE_TOL: a box of 64 cells of 2e6 Mpc/h has |log10 k| up to 7.3, the bound is 2.3e-6 dex.  The
    same grid with a table that reaches beyond it needs no margin and keeps its records."""
    shape, spacing = (64, 64, 64), 2.0e6
    xlo, xhi = pt.grid_range(shape, spacing)
    assert 2.0 ** -24 * (5 * max(abs(xlo), abs(xhi)) + (xhi - xlo - 0.02)) > cpu_ref.EDGE_TOL
    k, Pk = pt.hug(shape, spacing)
    Pk = pt.default_shape(k * 1e6)                                   # (the default table ends at k = 1e-4: borrow its shape higher up)
    k2 = (10.0 ** (2 * pt.mode_log10k(shape, spacing)[0][:4])).astype(np.float32)
    with pytest.raises(AssertionError):                              # emu_fast_sigma returns -3: no records
        emu_util.fast_sigma(*pt.sigma_table(k, Pk, shape, spacing), xlo, xhi, k2)
    k = pt.control(shape, spacing)[0]
    assert emu_util.fast_sigma(*pt.sigma_table(k, pt.default_shape(k * 1e6), shape, spacing), xlo, xhi, k2)[2] == 126


def test_default_power_is_untouched_by_the_rule(default_power):
    """No cell of any grid used here lies within 1e-3 dex of the default table's ends, so the oracle with and without the rule is
    one array, and the fast records are those of a range that ends inside the table."""
    k, Pk = default_power["k"], default_power["Pk"]
    for shape, spacing in ROWS:
        x, _ = pt.mode_log10k(shape, spacing)
        assert x.min() - np.log10(k[0]) > 1e-3 and np.log10(k[-1]) - x.max() > 1e-3
        noise = cpu_ref.native_noise(SEED, *shape, np.complex64)
        a = cpu_ref.generate_kspace(*shape, spacing, k, Pk, noise=noise)
        assert np.array_equal(a, cpu_ref.generate_kspace(*shape, spacing, k, Pk, noise=noise, edge_tol=cpu_ref.EDGE_TOL))
        assert records(shape, spacing, k, Pk) in (126, 254, 510)                   # no guard bin
