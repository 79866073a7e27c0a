"""The generic mixed-radix kernels (rf_generic.h, rf_k_generic.hip) against numpy at EVERY radix sequence and four-step split:
rf_execute_c2r from an uploaded half spectrum (with its moments), rf_execute_r2c and rf_execute_c2c in both directions, one axis
carrying the length under test, in both dtypes wherever the library accepts the shape -- run with -m gpu on an MI355X.

tests/test_gpu_generic.py visits the launch classes (tile, threads, LDS) at some twenty lengths; this file visits the ARITHMETIC the
length selects: every radix as the first and as a later stage of an in-place and of a two-buffer line, dot-product stages up to the
prime 8191, lines of zero to eight stages, the digit-reversed load (also with the generation inside the x pass: fused realisations
equal the unfused ones bit for bit), four-step splits with prime, odd and not-smooth sub-lines both forced by the cap and taken by
preference, and lines with and without the stage tables in LDS.  Table, coverage guards, inputs, references and the bound
(max error over all cells <= B s(Rmax) rms) are tests/generic_matrix.py's; tests/test_emulator_generic_matrix.py puts the same table
through the CPU emulator, so a case that fails here and passes there is a fault of the GPU build or launch, not of the arithmetic."""
import numpy as np
import pytest

import generic_matrix as gm
from conftest import golden
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

SPACING = 0.5


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


@pytest.fixture(scope="module")
def dpower():
    d = golden("default_power.npz")
    return d["k"], d["Pk"]


class Device:
    """generic_matrix.run_row's engine: one packed and one c2c plan per (shape, dtype), made on first use"""

    def __init__(self, hip):
        self.hip, self.plans = hip, {}

    def plan(self, shape, dtype, unpacked):
        key = (shape, dtype, unpacked)
        if key not in self.plans:
            assert self.hip.shape_supported(*shape, dtype), (shape, gm.dtype_name(dtype))
            self.plans[key] = self.hip.DevicePlan(*shape, dtype, unpacked=unpacked)
            assert not self.plans[key].tiled, (shape, "runs on the tiled kernels")
        return self.plans[key]

    def c2r(self, shape, dtype, ks):
        plan = self.plan(shape, dtype, False)
        plan.upload_k(ks)
        plan.execute_c2r()
        return (plan.download_real(),) + tuple(plan.moments())

    def r2c(self, shape, dtype, field):
        plan = self.plan(shape, dtype, False)
        plan.upload_real(field)
        plan.execute_r2c()
        return plan.download_k()

    def c2c(self, shape, dtype, a, inverse):
        plan = self.plan(shape, dtype, True)
        plan.upload_c(a)
        plan.execute_c2c(inverse=inverse)
        return plan.download_c()

    def close(self):
        for plan in self.plans.values():
            plan.close()
        self.plans = {}


def _fused_equals_unfused(plan, shape, dpower):
    """x rows: the x pass that generates its cells writes them to the same generic_pos positions as the pass that loads them"""
    from randomfield_amd import powertools
    plan.set_kgrid(*powertools.ksq_axes(*shape, SPACING))
    plan.set_power(*cpu_ref.sigma_table(*dpower, *shape, SPACING))
    out = {}
    for on in (False, True):
        plan.set_fused_generation(on)
        assert plan.fused_generation is on
        plan.realise(seed=31337)
        out[on] = (plan.download_real(), plan.moments())
    plan.set_fused_generation(False)
    assert float(np.std(out[False][0])) > 0
    assert np.array_equal(out[True][0], out[False][0]) and out[True][1] == out[False][1], ("fused generation", shape)


@pytest.mark.parametrize("role,n", gm.CASES, ids=gm.case_id)
def test_generic_transforms_at_every_radix_sequence(hip, dpower, role, n):
    dev = Device(hip)
    try:
        for dtype in gm.dtypes_of(role, n):
            gm.run_row(role, n, dtype, dev)
            if role == "x":
                _fused_equals_unfused(dev.plan(gm.shape_of(role, n), dtype, False), gm.shape_of(role, n), dpower)
        for role_, n_ in gm.C64_ONLY:
            if (role_, n_) == (role, n):
                assert not hip.shape_supported(*gm.shape_of(role, n), gm.C128)
    finally:
        dev.close()


def test_the_table_reaches_every_stage_form():
    """(needs no GPU work: the coverage guards of the table this file runs)"""
    gm.guard_coverage()


def test_print_the_worst_figures():
    """(after the table: the worst measured / bound per transform, dtype and role, for CHANGES.md)"""
    for line in gm.worst_lines():
        print(line)
