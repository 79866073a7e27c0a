"""rf_kernel_ms / rf_elapsed_ms after one timed call of every schedule form (csrc/rf_timing.h: one recorder of tagged intervals behind
all of them): five entries, none negative, the same entries zero and non-zero as before the recorder existed, and the entries tile the
call -- their sum is rf_elapsed_ms.

PATTERN and TILING_MS below were written down from `timed_forms` run against the library of the commit BEFORE the recorder (the parent
of the change that added this file), on one MI355X; profiles/schedule_timing_parity.txt keeps that run.  '+': > 0; '0': exactly 0.0;
'~': in that library the distance between two events recorded back to back with no work between them (a few microseconds or 0 there),
which the recorder may report as exactly 0: only >= 0 is asked of it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SPACING = 2.5
INV_H = [1.0 / SPACING] * 3

# form -> pattern of (x, y, z, reduce, extra), as the parent's library showed it in each of three rounds.  The '~' entries, from the
# schedules' code and that run (where they are 4 to 6 microseconds, the distance between two events recorded back to back): the reduce
# entry of a paint and y, z and reduce of a gather (the calls end where their last launch ends), the y entry of a call that exchanges in
# sub-slabs (its whole forward half is charged to x), and the extra entry at 64^3, whose generation pass is one launch.
PATTERN = {
    "native": "+++++", "exact": "++++0", "native slabs16": "+++++", "exact slabs16": "++++0", "four slabs": "++++~",
    "merged slabs2": "+++++", "merged slabs3": "+++++", "slab path chunks1": "+++++", "slab path chunks2": "+~++0",
    "generic unfused": "+++++", "generic fused": "++++0", "lognormal": "+++++", "paint": "+++~0", "gather": "+~~~0",
}
# |sum(kernel_ms) - elapsed_ms|: the largest value over these calls (three rounds) in the parent's library was 7.0e-07 ms -- float32
# rounding of the sum; the event time stamps tile exactly.  Ten times it is below 2 microseconds, so the bound is 2 microseconds (event
# time stamps are quantised and the sum adds up to a dozen float32 values).
TILING_MS = 0.002


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


def timed_forms(hip):
    """yields (form, kernel_ms, elapsed_ms) after one timed call of each schedule form"""
    from randomfield_amd import powertools
    power = powertools.load_default_power()

    def make(shape):
        plan = hip.DevicePlan(*shape, np.complex64)
        plan.set_kgrid(*powertools.ksq_axes(*shape, SPACING))
        plan.set_power(*powertools.sigma_table(power, shape, SPACING))
        return plan

    def read(plan):
        kern = plan.kernel_ms()
        return list(kern), plan.elapsed_ms()

    plan = make((64, 32, 128))
    for slabs in (None, 16):
        if slabs:
            plan.set_yz_slab_planes(slabs)
        for exact in (False, True):
            plan.set_exact_generation(exact)
            plan.realise(seed=11)
            yield (("exact" if exact else "native") + (" slabs%d" % slabs if slabs else ""),) + tuple(read(plan))
    plan.set_exact_generation(False)
    plan.set_yz_slab_planes(-1)
    nz = plan.nz
    plan.set_z_tables(np.linspace(1.0, 0.5, nz), np.linspace(0.9, 1.1, nz))
    plan.realise_lognormal(seed=11)
    yield ("lognormal",) + tuple(read(plan))
    plan.set_force_slab_path(True)
    for chunks in (1, 2):
        plan.set_exchange_chunks(chunks)
        plan.realise(seed=11)
        yield ("slab path chunks%d" % chunks,) + tuple(read(plan))
    plan.close()

    plan = make((64, 64, 64))                         # (whole z-pass workgroups per plane: the passes do run in four slabs)
    plan.set_yz_slab_planes(16)
    assert plan.yz_slabs() == (4, 16)
    plan.realise(seed=11)
    yield ("four slabs",) + tuple(read(plan))
    plan.close()

    plan = make((8, 1024, 1024))                      # the smallest shape the merged y + z kernel serves
    plan.set_merged_yz(2)
    for planes, launches in ((2, 3), (3, 2)):         # 4 slabs of 2 planes; 2 slabs of 3 and a last one of 2
        plan.set_yz_slab_planes(planes)
        plan.realise(seed=11)
        ms, n = plan.merged_yz_ms()
        kern, total = read(plan)
        assert n == launches and 0.0 < ms <= kern[1]
        yield ("merged slabs%d" % planes, kern, total)
    plan.close()

    plan = make((40, 60, 80))
    for fused in (False, True):
        plan.set_fused_generation(fused)
        plan.realise(seed=11)
        yield ("generic fused" if fused else "generic unfused",) + tuple(read(plan))
    plan.close()

    plan = make((16, 16, 16))
    plan.realise(seed=11)
    plan.particles_accumulate(0, 0.5, first=True)
    plan.particles_paint(INV_H)
    yield ("paint",) + tuple(read(plan))
    plan.particles_gather(INV_H, 0)
    yield ("gather",) + tuple(read(plan))
    plan.close()


def test_every_schedule_form_tiles_its_call(hip):
    seen = []
    for form, kern, total in timed_forms(hip):
        gap = abs(float(np.sum(np.asarray(kern, np.float32), dtype=np.float64)) - total)
        print("%-20s kernel_ms %s elapsed_ms %.6f |sum - elapsed| %.6f" % (form, ["%.6f" % v for v in kern], total, gap))
        seen.append(form)
        assert len(kern) == 5 and all(v >= 0.0 for v in kern), form
        for v, want in zip(kern, PATTERN[form]):
            assert (v > 0.0) if want == "+" else (v == 0.0) if want == "0" else want == "~", (form, kern, PATTERN[form])
        assert gap <= TILING_MS, (form, kern, total)
    assert sorted(seen) == sorted(PATTERN)
