"""What a plan allocates lives and dies with it (csrc/rf_owned.h: every buffer, event and stream is an owning member of rf_plan).
rf_diag_live_resources counts what the plans of this process hold, so "freed with the plan" is tested without the device-wide free
memory that other processes change: drive every lazy allocation once, compare rf_plan_nbytes with the formula written out here,
destroy the plans, and the three counters are back where they started.  And growing `stats` / `seeds_dev` (which drops the captured
batch graphs) changes no field."""
import ctypes
import gc

import numpy as np
import pytest

from oracle import cpu_ref

pytestmark = pytest.mark.gpu

SPACING = 2.5


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


def live(hip):
    """(device bytes, events, streams) held by the plans of this process"""
    b, e, s = ctypes.c_size_t(0), ctypes.c_int(0), ctypes.c_int(0)
    hip.check(hip.load().rf_diag_live_resources(ctypes.byref(b), ctypes.byref(e), ctypes.byref(s)), "rf_diag_live_resources")
    return b.value, e.value, s.value


def tables(hip, plan, power):
    from randomfield_amd import powertools
    plan.set_kgrid(*powertools.ksq_axes(plan.nx, plan.ny, plan.nz, SPACING))
    plan.set_power(*cpu_ref.sigma_table(power["k"], power["Pk"], plan.nx, plan.ny, plan.nz, SPACING))
    return plan


def want_nbytes(plan, have, noise=False, scratch=0):
    """rf_plan_nbytes from the shape: the field buffer W and whichever of R, W2 + R2, X, K, P, L, Q, A, G, G2 exist (`have`), the
    float64 deviates and the replay's runs"""
    nx, ny, nz, cs = plan.nx, plan.ny, plan.nz, plan.complex_dtype.itemsize
    nzl = nz // 2 // plan.nranks
    w = nx * ny * nz * cs if plan.unpacked else nx * ny * nzl * cs
    k = 0 if plan.unpacked else nx * ny * (nzl + 1) * cs
    ppitch = nzl + 1 if cs == 16 else nzl + (64 if nzl >= 256 else 2)
    p = nx * ny * ppitch * cs
    h = lambda name: 1 if name in have else 0
    total = w * (1 + h("R") + 2 * h("W2") + h("X")) + h("K") * k + h("P") * p + h("L") * max(2 * w, p) + h("Q") * 3 * w + h("A") * nx * ny * nz * 8
    total += (h("G") + h("G2")) * (w if plan.unpacked else k)
    return total + (2 * nx * ny * (nzl + 1) * 8 if noise else 0) + scratch


def mt_runs_bytes(plan, pair_bytes):
    """bytes of the MT19937 replay's runs for this grid: segments x attempts per segment x bytes per accepted pair"""
    from randomfield_amd import mt19937
    cells = plan.nx * plan.ny * (plan.nz // 2 + 1)
    bps = mt19937.segment_blocks_for(cells)
    blocks = -(-4 * mt19937.attempts_needed(cells) // 624)
    return -(-blocks // bps) * bps * 156 * pair_bytes


def test_everything_a_plan_allocates_is_freed_with_it(hip, default_power):
    gc.collect()                                             # (plans other tests dropped without close() go now, not in the middle)
    start = live(hip)
    plans = []

    def step(plan, have, **more):
        plan.sync()
        assert plan.nbytes == want_nbytes(plan, have, **more), sorted(have)
        assert live(hip)[0] - start[0] >= sum(q.nbytes for q in plans)

    # -- a complex64 plan on the tiled kernels: (64, 64, 64), the smallest grid the one-call replay's and the host sink's tests use
    p = hip.DevicePlan(64, 64, 64, np.complex64)
    plans.append(p)
    have = set()
    step(p, have)
    after_create = live(hip)
    assert after_create[0] - start[0] >= p.nbytes and after_create[1] - start[1] == 6 and after_create[2] - start[2] == 1
    tables(hip, p, default_power)
    p.generate(seed=1); have.add("K"); step(p, have)
    edges = np.linspace(0.0, 1.0, 9)
    p.measure_power(edges, hip.RF_POWER_FROM_KSPACE); step(p, have)
    p.realise_potential(seed=2); have.add("P"); step(p, have)
    p.set_transposed_intermediate(True)
    p.realise(seed=3); have.add("X"); step(p, have)
    p.set_transposed_intermediate(False); have.discard("X"); step(p, have)          # (the flag off hands X back)
    dk = [2 * np.pi / (n * SPACING) for n in (p.nx, p.ny, p.nz)]
    p.lpt2_source(dk); have.add("L"); step(p, have)
    p.particles_accumulate(0, 0.5, first=True); have.add("Q"); step(p, have)
    assert p.particles_paint([1.0 / SPACING] * 3) == 0; have.add("A"); step(p, have)
    z = np.arange(p.nz) / p.nz
    p.set_z_tables(np.exp(-0.5 * z), 0.5 + z)
    p.realise_lognormal(seed=4); step(p, have)
    # the MT19937 replay in both forms: float32 pairs stay in the runs; float64 deviates are moved into the noise buffer, after which
    # the runs (now twice as large) stay or -- on a device that is two thirds full -- are handed back
    assert p.can_batch_reference()
    p.reference_noise(5, single=True); step(p, have, scratch=mt_runs_bytes(p, 8))
    p.reference_noise(5)
    p.sync()
    assert p.nbytes in (want_nbytes(p, have, noise=True, scratch=mt_runs_bytes(p, 16)), want_nbytes(p, have, noise=True))
    runs = p.nbytes - want_nbytes(p, have, noise=True)
    p.realise_batch_reference([6, 7]); step(p, have, noise=True, scratch=max(runs, mt_runs_bytes(p, 8)))
    runs = max(runs, mt_runs_bytes(p, 8))
    p.realise_batch([1, 2, 3]); step(p, have, noise=True, scratch=runs)
    p.realise_batch(np.arange(100)); step(p, have, noise=True, scratch=runs)
    host = np.empty((p.nx, p.ny, p.nz), np.float32)
    assert p.arm_host_sink(host)
    p.realise(seed=8)
    assert p.host_sink_delivered(); step(p, have, noise=True, scratch=runs)
    assert live(hip)[2] - start[2] == 3                      # the plan's stream, the replays' and the sink's

    # -- a complex128 plan: the same lazy arrays at the other element size, no padded potential rows
    d = tables(hip, hip.DevicePlan(16, 16, 32, np.complex128), default_power)
    plans.append(d)
    have = set()
    d.generate(seed=1); have.add("K"); step(d, have)
    d.realise_potential(seed=2); have.add("P"); step(d, have)
    d.lpt2_source([2 * np.pi / (n * SPACING) for n in (16, 16, 32)]); have.add("L"); step(d, have)
    d.particles_accumulate(2, 1.0, first=True); have.add("Q"); step(d, have)
    d.particles_paint([1.0 / SPACING] * 3); have.add("A"); step(d, have)
    d.reference_noise(9)                                      # (float64 plans replay float64 deviates)
    d.sync()
    assert d.nbytes in (want_nbytes(d, have, noise=True, scratch=mt_runs_bytes(d, 16)), want_nbytes(d, have, noise=True))

    # -- the slab pipeline on one rank, the exchange whole and in 4 sub-slabs, and its pipelined batch (second buffer pair)
    s = tables(hip, hip.DevicePlan(256, 128, 256, np.complex64), default_power)
    plans.append(s)
    s.set_force_slab_path(True); step(s, {"R"})
    s.realise(seed=1); step(s, {"R"})
    s.set_exchange_chunks(4)
    s.realise(seed=1); step(s, {"R"})
    s.realise_batch([1, 2, 3]); step(s, {"R", "W2"})

    # -- two virtual ranks linked for the direct exchange: receive buffers, second pair, exchange stream, the table of destinations
    ranks = [tables(hip, hip.DevicePlan(32, 16, 128, np.complex128, nranks=2, rank=r), default_power) for r in range(2)]
    plans.extend(ranks)
    for r in ranks:
        r.set_exchange_chunks(2)
    hip.DevicePlan.slab_link_direct(ranks)
    for r in ranks:
        r.slab_forward(seed=3)
    for r in ranks:
        r.slab_backward()
    for r in ranks:
        step(r, {"R", "W2"})

    # -- a plan on the generic kernels and an unpacked c2c plan
    g = tables(hip, hip.DevicePlan(6, 4, 12, np.complex64), default_power)
    plans.append(g)
    g.realise(seed=1); step(g, {"K", "G"})
    c = hip.DevicePlan(16, 16, 16, np.complex64, unpacked=True)
    plans.append(c)
    c.upload_c(np.ones((16, 16, 16), np.complex64))
    c.execute_c2c(True); step(c, set())

    held = live(hip)
    assert held[0] - start[0] >= sum(q.nbytes for q in plans) and held[1] > start[1] + 6 * len(plans) and held[2] >= start[2] + len(plans) + 4
    for q in plans:
        q.close()
    assert live(hip) == start


def test_batches_after_the_seed_and_moment_arrays_grew(hip, default_power):
    """rf_realise_batch with 3 seeds, then 100 (the device arrays of seeds and moments grow, the captured graphs go), then 3 again: every
    call gives the last field and all rms values of the same call on a fresh plan, bit for bit."""
    calls = [np.arange(3) + 11, np.arange(100) + 1000, np.arange(3) + 11]
    shape = (16, 16, 16)
    plan = tables(hip, hip.DevicePlan(*shape, np.complex64), default_power)
    for seeds in calls:
        rms = plan.realise_batch(seeds)
        field = plan.download_real()
        fresh = tables(hip, hip.DevicePlan(*shape, np.complex64), default_power)
        rms_fresh = fresh.realise_batch(seeds)
        assert np.array_equal(rms, rms_fresh) and np.all(rms > 0)
        assert np.array_equal(field, fresh.download_real())
        fresh.close()
    plan.close()
