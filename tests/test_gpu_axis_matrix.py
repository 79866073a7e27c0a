"""rf_execute_r2c, rf_execute_c2r from an uploaded half spectrum and rf_execute_c2c (both directions) against numpy at EVERY tiled
axis length, one axis long at a time, in both dtypes and both addressing regimes of a column tile -- run with -m gpu on an MI355X.

The realisation path is pinned at every length by the reference fixtures; these entry points share its tile code but are GPU
instantiations of their own (direction -1, the two-half-transform form of the long float32 in-place passes, the > 64 KB LDS attribute,
launch shapes), which only a value computed on the GPU can check.  Table, guards, inputs, references and the bound (max error over all
cells <= 1e-5 rms float32, 3e-13 rms float64) are tests/axis_matrix.py's; tests/test_emulator_axis_matrix.py puts the same table through
the CPU emulator, so a case that fails here and passes there is a fault of the GPU build or launch, not of the phase functions."""
import pytest

import axis_matrix as am

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


@pytest.mark.parametrize("axis,n", am.CASES, ids=am.case_id)
def test_r2c_c2r_c2c_one_long_axis(hip, axis, n):
    for shape, dtype in am.plans(axis, n, packed=True):
        plan = hip.DevicePlan(*shape, dtype)
        assert plan.tiled
        # forward: real field -> half spectrum (API layout), Hermitian on the planes kz = 0 and nz/2
        field = am.real_field(shape, dtype, n)
        plan.upload_real(field)
        plan.execute_r2c()
        spec = plan.download_k()
        bound = am.check("r2c", spec, am.rfftn(field), dtype, shape)
        am.check_hermitian(spec, bound, shape)
        # inverse from an uploaded half spectrum: symmetrised, and raw (numpy's irfftn defines the answer there too)
        for what, ks in zip(("c2r", "c2r raw"), am.half_spectra(shape, dtype, n)):
            ref = am.irfftn(ks, shape)
            plan.upload_k(ks)
            plan.execute_c2r()
            am.check(what, plan.download_real(), ref, dtype, shape)
            am.check_moments(what, *plan.moments(), ref, dtype, shape)
        plan.close()
    for shape, dtype in am.plans(axis, n, packed=False):
        plan = hip.DevicePlan(*shape, dtype, unpacked=True)
        a = am.complex_array(shape, dtype, n)
        for inverse, what, ref in ((False, "c2c forward", am.fftn(a)), (True, "c2c inverse", am.ifftn(a))):
            plan.upload_c(a)
            plan.execute_c2c(inverse=inverse)
            am.check(what, plan.download_c(), ref, dtype, shape)
        plan.close()
