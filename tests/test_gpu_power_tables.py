"""Value tests of the native generation pass on user power tables (tests/power_tables.py) -- run with -m gpu on an MI355X.

Every other GPU value test feeds the 500-row default power, which is wider than any grid and reaches one branch of the float32 sigma
lookup (csrc/rf_host.h build_fast_records, csrc/rf_core.h fast_sigma / sigma_lookup).  Here: 126 / 254 / 510 real bins, all-zero guard
bins on either side, the automatic fall-back to the exact kernel, 2 rows, a zero run, tables that end inside the grid, and tables
that end ON the grid's k_min / k_max (the edge rule, RF_EDGE_TOL), through v_log_f32 and OCML's log10f instead of the host's libm that
tests/test_emulator_power_tables.py runs.  The shapes are the smallest that select each generation kernel (nx = 64: one tile; 512;
1024; 2048 as two half transforms; float64 at 64 and at 1024 as two half transforms; float64 at 2048: no fast kernel; generic); the
spacings 1.0, 0.7 and 10.0 on (64, 32, 128) change which way a cell on a hugging edge rounds.

The oracle is tests/power_tables.py oracle_field: cpu_ref's stages in float64 on cpu_ref's restatement of the same Philox stream, with
the edge rule and without the reference's coverage check.  Bounds are the project's own (test_gpu_parity.py
test_native_rng_matches_oracle_restatement): 1e-5 rms for the fast flavour on either plan type and for the exact chain of a complex64
plan, TOL_F64 for the exact chain of a complex128 plan; k space within the same tol of its largest magnitude, and the set of
exactly-zero cells is the oracle's.  Every test asserts which kernel ran (rf_diag_generation_path) and prints measured / bound.

Left out: band tables on (2048, 8, 32) -- the squares of a 2048-point axis leave no gap of 2.2e-4 dex between neighbouring |k| with
10 % - 90 % of the cells beyond it, so no edge can be 1e-4 dex clear of every mode (tests/test_emulator_power_tables.py asserts
exactly that)."""
import functools

import numpy as np
import pytest

import power_tables as pt
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

C64, C128 = np.complex64, np.complex128
TOL_F32 = 1e-5          # * rms, the north-star tolerance (tests/test_gpu_parity.py)
TOL_F64 = 1e-11
SEED = 7

# (shape, dtype, spacing, fused generic generation or None on tiled plans)
GRIDS = ([((64, 32, 128), dt, sp, None) for dt in (C64, C128) for sp in (2.5, 1.0, 0.7, 10.0)] +
         [((512, 16, 64), C64, 2.5, None), ((1024, 8, 32), C64, 2.5, None), ((2048, 8, 32), C64, 2.5, None),
          ((1024, 8, 16), C128, 2.5, None), ((40, 60, 80), C64, 2.5, False), ((40, 60, 80), C64, 2.5, True)])


def _feasible(name, shape, spacing):
    try:
        pt.build(name, shape, spacing)
    except pt.NoClearEdge:
        assert name.startswith("band") and shape == (2048, 8, 32)
        return False
    return True


CASES = [g + (name,) for g in GRIDS for name in pt.TABLES if _feasible(name, g[0], g[2])]


def _id(v):
    if isinstance(v, tuple):
        return "x".join(map(str, v))
    if v is C64 or v is C128:
        return "c64" if v is C64 else "c128"
    return {None: "tiled", False: "unfused", True: "fused"}[v] if v is None or isinstance(v, bool) else str(v)


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


@functools.lru_cache(maxsize=None)
def native_noise(shape, dtype):
    """cpu_ref's restatement of the plan's Philox stream for SEED: computed once per grid, shared, read-only"""
    noise = cpu_ref.native_noise(SEED, *shape, dtype)
    noise.setflags(write=False)
    return noise


def report(what, measured, bound):
    print("%-64s %.3e / %.1e" % (what, measured, bound))
    assert measured <= bound, "%s: %.3e > %.1e" % (what, measured, bound)


def make_plan(hip, shape, dtype, spacing, k, Pk):
    """rf_set_kgrid + rf_set_power with (log10 k, sigma) as powertools.py:153-154 forms them; no coverage check (the C API has none)"""
    from randomfield_amd import powertools
    plan = hip.DevicePlan(*shape, dtype)
    plan.set_kgrid(*powertools.ksq_axes(*shape, spacing))
    plan.set_power(*pt.sigma_table(k, Pk, shape, spacing))
    return plan


def check_field(plan, ref, rms, tol, what):
    d = plan.download_real()
    assert d.shape == ref.shape and d.dtype == ref.dtype
    report(what + ": field", float(np.max(np.abs(d - ref))) / rms, tol)
    mean, std = plan.moments()
    report(what + ": rms", abs(std - rms) / rms, tol)
    assert abs(mean) <= 1e-6 * rms


@pytest.mark.parametrize("shape,dtype,spacing,fused,name", CASES, ids=_id)
def test_native_generation_against_oracle(hip, shape, dtype, spacing, fused, name):
    k, Pk = pt.build(name, shape, spacing)
    kref, ref, rms = pt.oracle_field(shape, spacing, k, Pk, native_noise(shape, dtype), dtype)
    assert rms > 0
    tol_exact = TOL_F32 if dtype == C64 else TOL_F64
    plan = make_plan(hip, shape, dtype, spacing, k, Pk)
    try:
        assert plan.tiled == (fused is None)
        if fused is not None:
            plan.set_fused_generation(fused)
        path = plan.generation_path()
        assert path == (pt.expected_path(name) if plan.tiled else "exact"), "%s table on %r ran the %s kernel" % (name, shape, path)
        tag = "%s %s" % (name, path)
        plan.realise(seed=SEED)
        check_field(plan, ref, rms, TOL_F32 if path == "fast" else tol_exact, tag)
        plan.set_exact_generation(True)
        assert plan.generation_path() == "exact"
        plan.realise(seed=SEED)
        check_field(plan, ref, rms, tol_exact, "%s exact (flag)" % name)
        plan.set_exact_generation(False)
        assert plan.generation_path() == path
        plan.generate(seed=SEED)
        ks = plan.download_k()
        report("%s k space" % name, float(np.max(np.abs(ks - kref)) / np.max(np.abs(kref))), tol_exact)
        diff = np.count_nonzero((ks == 0) != (kref == 0))
        assert diff == 0, "%d cells are exactly zero on one side only (%d in the oracle)" % (diff, np.count_nonzero(kref == 0))
        print("%-64s %d" % ("%s exactly-zero cells" % name, np.count_nonzero(kref == 0)))
    finally:
        plan.close()


def test_float64_2048_runs_the_exact_kernel(hip):
    """float64 plans have no fast generation kernel at nx = 2048 (rf_capi.hip build_fast, col_fastgen_supported): whatever the table,
    the plan reports and runs the exact chain -- held to TOL_F64."""
    shape, spacing = (2048, 8, 32), 2.5
    for name in ("control", "hug"):
        k, Pk = pt.build(name, shape, spacing)
        kref, ref, rms = pt.oracle_field(shape, spacing, k, Pk, native_noise(shape, C128), C128)
        plan = make_plan(hip, shape, C128, spacing, k, Pk)
        try:
            assert plan.generation_path() == "exact"
            plan.realise(seed=SEED)
            check_field(plan, ref, rms, TOL_F64, "%s float64 nx = 2048" % name)
        finally:
            plan.close()


@pytest.mark.parametrize("name", ["hug", "band_low", "band_pass"])
def test_resident_stream_fast_path(hip, name):
    """The reference's MT19937 stream replayed on the device as float32 pairs and read by the fast generation pass (SRC = 2): the same
    records, another consumer of fast_sigma."""
    shape, spacing, seed = (64, 32, 128), 2.5, 11
    k, Pk = pt.build(name, shape, spacing)
    noise = cpu_ref.reference_noise(seed, shape[0] * shape[1] * (shape[2] // 2 + 1))
    kref, ref, rms = pt.oracle_field(shape, spacing, k, Pk, noise, C64)
    plan = make_plan(hip, shape, C64, spacing, k, Pk)
    try:
        assert plan.generation_path() == "fast"
        plan.reference_noise(seed, single=True)
        assert plan.can_regenerate_potential("resident")                  # the float32 pairs are resident, not a float64 fall-back
        plan.realise(0, "resident")
        check_field(plan, ref, rms, TOL_F32, "%s fast, resident float32 stream" % name)
    finally:
        plan.close()


@pytest.mark.parametrize("rng", ["native", "reference"])
def test_generator_with_a_hugging_table(hip, rng):
    """What a user does: a table built from the grid's own k_bounds, handed to Generator(backend='hip')."""
    from randomfield_amd import Generator
    from randomfield_amd.powertools import make_power
    shape, spacing, seed = (64, 32, 128), 2.5, 11
    k, Pk = pt.build("hug", shape, spacing)
    kmin, kmax = cpu_ref.k_bounds(*shape, spacing)
    assert k[0] == kmin and k[-1] == kmax
    gen = Generator(*shape, spacing, power=make_power(k, Pk), backend="hip", rng=rng)
    try:
        d = gen.generate_delta_field(seed=seed, save_potential=False)
        noise = (cpu_ref.native_noise(seed, *shape, C64) if rng == "native" else
                 cpu_ref.reference_noise(seed, shape[0] * shape[1] * (shape[2] // 2 + 1)))
        kref, ref, rms = pt.oracle_field(shape, spacing, k, Pk, noise, C64)
        assert gen.plan_c2r.device.generation_path() == "fast"
        report("Generator(rng=%r) hug: field" % rng, float(np.max(np.abs(np.asarray(d) - ref))) / rms, TOL_F32)
        report("Generator(rng=%r) hug: rms" % rng, abs(float(gen.delta_field_rms) - rms) / rms, TOL_F32)
    finally:
        gen.plan_c2r.device.close()
