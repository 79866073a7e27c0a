"""The predicates of the generation source (randomfield_amd/csrc/rf_source.h) against what the calls they announce then do -- run with
-m gpu on an MI355X.  can_regenerate_potential(mode) is true exactly when realise_scaled_potential(mode) succeeds, and the field then
equals the stored route's (realise_potential, load_potential(scale), execute_c2r); can_batch_reference() is true exactly when
realise_batch_reference of two seeds succeeds.  Both dtypes, the exact flag off and on, no deviates / a float32 replay / a float64 replay
resident -- and the exact flag set AFTER a float32 replay, which leaves pairs resident that no x pass reads any more -- on the smallest
power-of-two plan that reports the fast path.  Every failing branch is a refusal with an error string."""
import numpy as np
import pytest

import generation_matrix as gm
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

SCALE = gm.SCALE
# tests/test_gpu_parity.py test_regenerated_potential_equals_stored_one: the regenerated against the stored route, x the field's std
REGENERATED_VS_STORED = {gm.C64: 2e-6, gm.C128: 1e-9}


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


def make_plan(hip, shape, dtype, power):
    from randomfield_amd import powertools
    plan = hip.DevicePlan(*shape, dtype)
    plan.set_kgrid(*powertools.ksq_axes(*shape, gm.SPACING))
    plan.set_power(*cpu_ref.sigma_table(power["k"], power["Pk"], *shape, gm.SPACING))
    plan.set_mt_segment_blocks(gm.mt_blocks(shape))
    return plan


_SHAPES = {}


def smallest_fast_shape(hip, dtype, power):
    """(nx, 16, 16) with the smallest x length of tests/generation_matrix.py's on which generation_path() reports the fast path"""
    if dtype not in _SHAPES:
        for nx in gm.am.COL_LENGTHS:
            plan = make_plan(hip, (nx, 16, 16), dtype, power)
            try:
                if plan.generation_path() == "fast":
                    _SHAPES[dtype] = (nx, 16, 16)
                    break
            finally:
                plan.close()
    return _SHAPES[dtype]


def refused(call):
    """True: the call was refused with an error string (a RuntimeError carrying rf_last_error)"""
    try:
        call()
    except RuntimeError as e:
        assert str(e)
        return True
    return False


CASES = [(dtype, exact, deviates) for dtype in (gm.C64, gm.C128) for exact in (False, True)
         for deviates in ("none", "float32 replay", "float64 replay")] + [(dtype, True, "float32 replay, then the flag") for dtype in (gm.C64, gm.C128)]


@pytest.mark.parametrize("dtype,exact,deviates", CASES, ids=["%s-%s-%s" % (gm.dtype_name(d), "exact" if e else "fast", v) for d, e, v in CASES])
def test_predicate_iff_behaviour(hip, default_power, dtype, exact, deviates):
    flag_after = deviates.endswith("then the flag")
    shape = smallest_fast_shape(hip, dtype, default_power)
    plan = make_plan(hip, shape, dtype, default_power)
    try:
        if not flag_after:
            plan.set_exact_generation(exact)
        if deviates != "none":
            assert plan.reference_noise(4242, single=deviates.startswith("float32")) >= shape[0] * shape[1] * (shape[2] // 2 + 1)
        if flag_after:
            plan.set_exact_generation(True)
        assert plan.generation_path() == ("exact" if exact else "fast")
        for noise in (None, "resident"):
            can = plan.can_regenerate_potential(noise)
            # the fast kernel on Philox, or on float32 pairs -- which only a complex64 plan on the fast path is given (else float64 ones)
            assert can == (not exact and (noise is None or (dtype == gm.C64 and deviates == "float32 replay"))), noise
            assert can == (not refused(lambda: plan.realise_scaled_potential(seed=77, noise=noise, scale=SCALE))), (noise, can)
            if can:
                got = plan.download_real()
                plan.realise_potential(seed=77, noise=noise)
                plan.load_potential(SCALE)
                plan.execute_c2r()
                want = plan.download_real()
                assert np.max(np.abs(got - want)) <= REGENERATED_VS_STORED[dtype] * want.std(), noise
        # last: a batch that runs leaves the float32 pairs of its last seed as the resident deviates
        can = plan.can_batch_reference()
        assert can == (dtype == gm.C64 and not exact)
        assert can == (not refused(lambda: plan.realise_batch_reference([11, 12]))), can
        if can:
            assert plan.can_regenerate_potential("resident")
    finally:
        plan.close()
