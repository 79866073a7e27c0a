"""The generation pass fused into the x FFT, mode by mode against cpu_ref's float64 stages, at EVERY x length, in both dtypes, for every
FastV<slab, pot, src, halves> of rf_select.h and every launch form of fastgen_sequence, and the exact kernel behind them -- run with
-m gpu on an MI355X.

The other GPU tests pin the fast variants at nx in {16, 64, 512, 1024, 2048} with max |field - oracle| <= 1e-5 rms, which one mode
that is 1e-3 off does not move (4e-6 rms on (N, 8, 128)); here every mode of the half spectrum is held to c sigma_m (1 + |n_m|) + the
floor of its window, with c a few 1e-6 (tests/generation_matrix.py: table, guards, oracle, bounds, the classes' c and where they
come from), and the stored potential -- the pass's own k-space values, no floor -- to the exact Hermitian structure of its planes
kz = 0 and nz / 2.  The windows through a float32 transform are blunt (the field route's floor is above c everywhere, the
regenerated scaled potential's below it at the lowest k of the smallest grids only); what pins those variants mode by mode is the
stored-potential route here and the loads window of the emulator twin.  Every plan, the ranks of J, K and K' included, asserts that
it runs the fast kernel.
tests/test_emulator_generation_matrix.py puts the same table through the CPU emulator and holds the table against rf_select.h, so
a case that fails here and passes there is a fault of the GPU build or launch, not of the phase functions."""
import numpy as np
import pytest

import generation_matrix as gm
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

C64, C128 = gm.C64, gm.C128


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


def make_plan(hip, shape, dtype, power, nranks=1, rank=0):
    from randomfield_amd import powertools
    plan = hip.DevicePlan(*shape, dtype, nranks=nranks, rank=rank)
    assert plan.tiled
    plan.set_kgrid(*powertools.ksq_axes(*shape, gm.SPACING))
    plan.set_power(*cpu_ref.sigma_table(power["k"], power["Pk"], *shape, gm.SPACING))
    if dtype == C64:
        plan.set_mt_segment_blocks(gm.mt_blocks(shape))
    return plan


def stored_potential(plan):
    plan.load_potential(1.0)
    return plan.download_k()


def twice(call, fetch):
    """the call's result, after a second identical call has reproduced it bit for bit"""
    call()
    first = fetch()
    call()
    second = fetch()
    for a, b in zip(first, second):
        assert np.array_equal(a, b), "a second identical call changed the result"
    return first


def single_rank(plan, vid, shape, dtype, power):
    """variants A - I on the (shape, dtype)'s one plan: (field, potential or None, moments() std)"""
    native_seed, stream_seed = gm.seeds(shape[0])
    assert plan.generation_path() == ("fast" if gm.fast_supported(dtype, shape[0]) else "exact")
    seed, noise = native_seed, None
    if vid in gm.C64_ONLY:
        single = vid != "D"
        first = gm.stream_segments(stream_seed, shape[0] * shape[1] * (shape[2] // 2 + 1), gm.mt_blocks(shape))
        assert gm.rows_cut(first, shape) >= 1, (shape, "no row of the grid is cut by a segment boundary")
        assert plan.reference_noise(stream_seed, single=single) >= shape[0] * shape[1] * (shape[2] // 2 + 1)
        # E - G: the float32 pairs are resident (src 2), not the float64 fall-back of segments shorter than 4 rows (src 1)
        assert plan.can_regenerate_potential("resident") == single
        seed, noise = 0, "resident"
    elif vid == "I":
        seed, noise = 0, gm.oracle_for(vid, shape, dtype, power).noise
    if vid in ("C", "G"):
        assert plan.can_regenerate_potential(noise)
    plan.set_exact_generation(vid == "H")
    try:
        if vid == "H":
            assert plan.generation_path() == "exact"
        route = gm.VARIANTS[vid][2]
        call = {"field": lambda: plan.realise(seed=seed, noise=noise),
                "potential": lambda: plan.realise_potential(seed=seed, noise=noise),
                "scaled": lambda: plan.realise_scaled_potential(seed=seed, noise=noise, scale=gm.SCALE)}[route]
        field, std, pot = twice(call, lambda: (plan.download_real(), np.float64(plan.moments()[1]),
                                               stored_potential(plan) if route == "potential" else np.zeros(0)))
        return field, (pot if route == "potential" else None), float(std)
    finally:
        plan.set_exact_generation(False)


def std_of_sums(sums, shape):
    """moments() of a job from its ranks' partial (sum, sum of squares) -- rf_slab_stats"""
    n = float(shape[0] * shape[1] * shape[2])
    s1, s2 = sum(a for a, b in sums), sum(b for a, b in sums)
    return float(np.sqrt(s2 / n - (s1 / n) ** 2))


def replicated(hip, shape, dtype, power):
    """J: every rank generates all of k space and keeps its x slab"""
    native_seed = gm.seeds(shape[0])[0]
    parts, sums = [], []
    for r in range(gm.NRANKS):
        plan = make_plan(hip, shape, dtype, power, gm.NRANKS, r)
        try:
            plan.set_replicated_generation(True)
            assert plan.generation_path() == "fast"
            part, stats = twice(lambda: plan.realise(seed=native_seed), lambda: (plan.download_real(), np.array(plan.slab_stats())))
            parts.append(part)
            sums.append(tuple(stats))
        finally:
            plan.close()
    return np.concatenate(parts, axis=0), None, std_of_sums(sums, shape)


def kz_slabs(hip, vid, shape, dtype, power):
    """K, K': the x pass of rank 1 starts at kz0 != 0.  (Of the ranks' copies of the Nyquist plane only rank 0's is written -- by the
    repair of the rank that owns kz = 0 -- and slab.assemble_side_array takes that one.)"""
    from randomfield_amd import slab
    native_seed = gm.seeds(shape[0])[0]
    plans = [make_plan(hip, shape, dtype, power, gm.NRANKS, r) for r in range(gm.NRANKS)]
    try:
        for p in plans:
            assert p.generation_path() == "fast"

        def run():
            for p in plans:
                if vid == "K":
                    p.slab_forward(seed=native_seed)
                else:
                    p.slab_forward(seed=native_seed, source="potential")
            hip.DevicePlan.slab_exchange_local(plans)
            for p in plans:
                p.slab_backward()

        def fetch():
            field = np.concatenate([p.download_real() for p in plans], axis=0)
            sums = np.array([p.slab_stats() for p in plans])
            pot = slab.assemble_side_array([stored_potential(p) for p in plans]) if vid == "K'" else np.zeros(0)
            return field, sums, pot

        field, sums, pot = twice(run, fetch)
        return field, (pot if vid == "K'" else None), std_of_sums([tuple(v) for v in sums], shape)
    finally:
        for p in plans:
            p.close()


def transform_on(hip, shape, dtype, power):
    """the c2r of an uploaded half spectrum on a plan of its own: what generation_matrix.window_error measures the scaled route with"""
    def transform(kspace):
        plan = make_plan(hip, shape, dtype, power)
        try:
            plan.upload_k(np.ascontiguousarray(kspace))
            plan.execute_c2r()
            return plan.download_real()
        finally:
            plan.close()
    return transform


def run_cases(hip, nx, dtype, power, on_case):
    """every case of one length and dtype: on_case(vid, shape, result)"""
    plan, plan_shape = None, None
    try:
        for vid, shape in gm.cases(nx, dtype):
            if vid == "J":
                result = replicated(hip, shape, dtype, power)
            elif vid in gm.LONG_ONLY:
                result = kz_slabs(hip, vid, shape, dtype, power)
            else:
                if plan_shape != shape:
                    if plan is not None:
                        plan.close()
                    plan, plan_shape = make_plan(hip, shape, dtype, power), shape
                result = single_rank(plan, vid, shape, dtype, power)
            on_case(vid, shape, result)
    finally:
        if plan is not None:
            plan.close()


@pytest.mark.parametrize("nx", gm.am.COL_LENGTHS, ids=gm.case_id)
def test_generation_pass_mode_by_mode(hip, default_power, nx):
    try:
        for dtype in gm.am.DTYPES:
            fields = {}

            def on_case(vid, shape, result):
                gm.check_case(vid, result, dtype, shape, default_power, emulator=False, transform=transform_on(hip, shape, dtype, default_power))
                if vid in ("A", "K"):
                    fields[vid, shape] = result[0]

            run_cases(hip, nx, dtype, default_power, on_case)
            ks = [key for key in fields if key[0] == "K"]
            assert len(ks) == (1 if gm.fast_supported(dtype, nx) else 0)
            for _, shape in ks:
                gm.check_k_equals_a(fields["K", shape], fields["A", shape], gm.oracle_for("A", shape, dtype, default_power), dtype, shape)
        gm.report_worst()
    finally:
        gm.forget_oracles()
