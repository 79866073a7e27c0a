"""Every exchanging form of a plan's route (randomfield_amd/csrc/rf_route.h) against the plain single-GPU pipeline -- run with -m gpu on
an MI355X.

A single-rank plan forced onto the slab path exchanges its own block: by the grouped copy or by the storing ("direct") y pass, each
whole or in 2 sub-slabs.  Each of the four forms runs rf_realise (native and host deviates), rf_realise_potential and a pipelined batch
of 3 seeds, and must give what a plain plan gives for the same seed.  The grids are the smallest powers of two on which
rf_plan_set_flag takes 2 sub-slabs in direct mode (nz / 4 planes per sub-slab = one y-pass tile: 32 columns complex64, 16 complex128).
Bounds: those of test_gpu_parity.py's test_pipelined_slab_batch_matches_plain_path and
test_direct_exchange_on_one_rank_through_the_whole_call_paths -- 1e-6 std on a field, 1e-7 std on an rms, 2e-6 std on the
transformed potential.  The two stand-ins of a virtual rank end in "not a field": the tail of the same schedules."""
import numpy as np
import pytest

from conftest import golden
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

SPACING = 2.5
SEEDS = [3, 4, 5]
GRIDS = {"c64": ((8, 8, 128), np.complex64), "c128": ((8, 8, 64), np.complex128)}
FORMS = [(direct, chunks) for direct in (False, True) for chunks in (1, 2)]


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


def make_plan(hip, shape, dtype, **kw):
    from randomfield_amd import powertools
    d = golden("default_power.npz")
    nx, ny, nz = shape
    plan = hip.DevicePlan(nx, ny, nz, dtype, **kw)
    plan.set_kgrid(*powertools.ksq_axes(nx, ny, nz, SPACING))
    plan.set_power(*cpu_ref.sigma_table(d["k"], d["Pk"], nx, ny, nz, SPACING))
    return plan


def run_calls(plan, noise):
    """the calls under test on one plan: name -> (field, std) or arrays"""
    out = {}
    plan.realise(seed=11)
    out["native"] = (plan.download_real(), plan.moments()[1])
    plan.realise(noise=noise)
    out["host"] = (plan.download_real(), plan.moments()[1])
    plan.realise_potential(seed=11)
    out["potential"] = (plan.download_real(), plan.moments()[1])
    plan.load_potential(-1.5)
    plan.execute_c2r()
    out["newtonian"] = plan.download_real()
    out["rms"] = plan.realise_batch(SEEDS)
    out["last"] = (plan.download_real(), plan.moments()[1])
    return out


@pytest.fixture(scope="module")
def reference(hip):
    """the plain single-GPU plan's results, computed once per grid and only read afterwards"""
    ref = {}
    for kind, (shape, dtype) in GRIDS.items():
        nx, ny, nz = shape
        noise = np.random.RandomState(5).normal(size=2 * nx * ny * (nz // 2 + 1))
        plain = make_plan(hip, shape, dtype)
        ref[kind] = (noise, run_calls(plain, noise))
        plain.close()
    return ref


@pytest.mark.parametrize("direct,chunks", FORMS, ids=["%s-%d" % ("direct" if d else "rccl", c) for d, c in FORMS])
@pytest.mark.parametrize("kind", sorted(GRIDS))
def test_exchanging_form_matches_the_plain_pipeline(hip, reference, kind, direct, chunks):
    shape, dtype = GRIDS[kind]
    noise, want = reference[kind]
    slab = make_plan(hip, shape, dtype)
    slab.set_force_slab_path(True)
    slab.set_exchange_chunks(chunks)
    assert slab.enable_direct_exchange(direct) == direct and slab.direct_exchange_enabled() == direct
    got = run_calls(slab, noise)
    slab.close()
    for call in ("native", "host", "potential", "last"):
        (a, sa), (b, sb) = got[call], want[call]
        err, derr = float(np.max(np.abs(a - b))), abs(sa - sb)
        print("%s %s chunks=%d %s: max|field - plain| = %.3g std, |std - plain| = %.3g std" % (kind, "direct" if direct else "rccl", chunks, call, err / sb, derr / sb))
        assert sb > 0 and err <= 1e-6 * sb, call
        assert derr <= 1e-7 * sb, call
    std = want["last"][1]
    assert len(got["rms"]) == len(SEEDS) and np.max(np.abs(got["rms"] - want["rms"])) <= 1e-7 * std
    a, b = want["newtonian"], got["newtonian"]
    assert a.std() > 0 and np.max(np.abs(a - b)) <= 2e-6 * a.std()


@pytest.mark.parametrize("standin", ["exchange", "direct-overlap", "direct-one-stream"])
def test_standin_schedules_end_in_not_a_field(hip, standin):
    """One rank of a 2-rank job without a communicator: the single call and the batch run the schedule of a multi-GPU rank and leave local
    moments but no field -- the download refuses, as before either call; the moments are finite and reproducible."""
    shape, dtype = GRIDS["c64"]
    p = make_plan(hip, shape, dtype, nranks=2, rank=1)
    with pytest.raises(RuntimeError):
        p.realise(seed=11)                                   # neither a communicator nor a stand-in
    if standin == "exchange":
        p.set_exchange_standin(8)
    else:
        p.set_direct_standin(True, overlap=(standin == "direct-overlap"))
    p.realise(seed=11)
    m1 = p.moments()
    with pytest.raises(RuntimeError, match="no real-space field"):
        p.download_real()
    rms = p.realise_batch(SEEDS)
    with pytest.raises(RuntimeError, match="no real-space field"):
        p.download_real()
    p.realise(seed=11)
    assert np.isfinite(m1[1]) and m1[1] > 0 and p.moments() == m1 and np.all(np.isfinite(rms)) and np.all(rms > 0) and len(rms) == len(SEEDS)
    p.close()
