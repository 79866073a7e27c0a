"""What a plan's device buffers hold after each call (randomfield_amd/csrc/rf_contents.h; DESIGN.md "What the buffers hold"), seen
from outside -- run with -m gpu on an MI355X.

Short call sequences through DevicePlan; after EVERY step the six calls that only read are tried -- download_real (a field), moments,
download_k (k space), download_aux (the auxiliary field), particles_download_counts (painted counts), download_noise (float64 deviates)
-- and each must succeed or raise the library's own refusal, as the literal expectation beside the step says.  The expectations are the
documented contract (include/randomfield_hip.h), not values read back from the library.  What the reading calls cannot see is
probed by a call that changes the plan, at the end of a sequence or where its refusal changes nothing: execute_r2c (a field in the
PRIMARY buffer), execute_gradient(RF_GRAD_FROM_POTENTIAL2) (the second-order potential), realise(noise="resident") (any deviates).

Plans: 16 x 16 x 16 complex64 and complex128 on the tiled kernels, 6 x 4 x 12 complex64 on the generic ones, and 16 x 16 x 16 complex64
through the slab pipeline (set_force_slab_path: the gathering z pass, the pipelined batch's two buffers, the exchange chunks).  No value
is compared: the value tests are the other test_gpu_* files.  Nothing but the library's own argument refusals is provoked."""
import numpy as np
import pytest

from conftest import golden
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

SPACING = 0.5
C64, C128 = np.complex64, np.complex128
# kind -> (shape, dtype, forced slab path)
KINDS = {"tiled64": ((16, 16, 16), C64, False), "tiled128": ((16, 16, 16), C128, False), "generic": ((6, 4, 12), C64, False),
         "slab": ((16, 16, 16), C64, True)}
ALL = ["tiled64", "tiled128", "generic", "slab"]
SINGLE = ["tiled64", "tiled128", "generic"]

# the calls that only read: (what they need, the call, its refusal)
READERS = [
    ("field", lambda p: p.download_real(), "no real-space field on the device"),
    ("moments", lambda p: p.moments(), "no realisation has been computed"),
    ("k", lambda p: p.download_k(), "no k-space data"),
    ("aux", lambda p: p.download_aux(), "no auxiliary field on the device"),
    ("counts", lambda p: p.particles_download_counts(), "no painted counts"),
    ("noise64", lambda p: p.download_noise(0, 2), "no float64 deviates resident on the device"),
]
NO_FIELD_IN_W = "no real-space field on the device: call rf_upload_real"
NO_K = "no k-space data"
NO_P2 = "no second-order potential: call rf_lpt2_potential first"
NO_DEVIATES = "no deviates resident on the device"


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


@pytest.fixture(scope="module")
def dpower():
    d = golden("default_power.npz")
    return d["k"], d["Pk"]


@pytest.fixture
def plan(hip, dpower, request):
    from randomfield_amd import powertools
    shape, dtype, slab = KINDS[request.param]
    nx, ny, nz = shape
    assert hip.shape_supported(nx, ny, nz, dtype)
    p = hip.DevicePlan(nx, ny, nz, dtype)
    assert p.tiled == (request.param != "generic")
    p.set_kgrid(*powertools.ksq_axes(nx, ny, nz, SPACING))
    p.set_power(*cpu_ref.sigma_table(dpower[0], dpower[1], nx, ny, nz, SPACING))
    if slab:
        p.set_force_slab_path(True)
    p.kind = request.param
    yield p
    p.close()


def holds(p, what, after):
    """exactly the things named in `what` (blank-separated names of READERS) can be read; every other reader is refused"""
    want = set(what.split())
    assert want <= {r[0] for r in READERS}
    for name, call, refusal in READERS:
        if name in want:
            try:
                call(p)
            except RuntimeError as exc:
                raise AssertionError("after %s (%s): %s should be there, but: %s" % (after, p.kind, name, exc))
        else:
            with pytest.raises(RuntimeError, match=refusal):
                call(p)
                pytest.fail("after %s (%s): %s should be refused" % (after, p.kind, name))


def per_kind(p, **what):
    """the expectation of this plan's kind: tiled = both tiled dtypes, else = every kind not named"""
    if p.kind in what:
        return what[p.kind]
    if p.kind.startswith("tiled") and "tiled" in what:
        return what["tiled"]
    return what["else_"]


def refused(p, call, refusal):
    with pytest.raises(RuntimeError, match=refusal):
        call()


def dk_of(p):
    return [2 * np.pi / (n * SPACING) for n in (p.nx, p.ny, p.nz)]


def real_field(p, seed=4):
    return np.random.RandomState(seed).normal(size=(p.nx, p.ny, p.nz)).astype(p.real_dtype)


def edges_of(p):
    return np.linspace(0.0, 1.1 * np.sqrt(3.0) * np.pi / SPACING, 5)


@pytest.mark.parametrize("plan", ALL, indirect=True)
def test_fresh_plan_holds_nothing(hip, plan):
    p = plan
    holds(p, "", "creation")
    refused(p, lambda: p.realise(noise="resident"), NO_DEVIATES)
    refused(p, p.execute_r2c, NO_FIELD_IN_W)
    refused(p, p.execute_c2r, NO_K)
    refused(p, lambda: p.measure_power(edges_of(p), hip.RF_POWER_FROM_FIELD), NO_FIELD_IN_W)
    refused(p, lambda: p.measure_power(edges_of(p), hip.RF_POWER_FROM_KSPACE), NO_K)
    refused(p, lambda: p.scale_z(np.ones(p.nz)), "no real-space field on the device")
    refused(p, lambda: p.lensing_potential(np.ones(p.nz), SPACING, 1), "no real-space field on the device")
    refused(p, lambda: p.execute_gradient(0, 1.0, dk_of(p)[0], hip.RF_GRAD_FROM_POTENTIAL2), NO_P2)
    refused(p, lambda: p.execute_gradient(0, 1.0, dk_of(p)[0], hip.RF_GRAD_FROM_KSPACE), NO_K)
    holds(p, "", "the refusals")                             # a refusal changes nothing


@pytest.mark.parametrize("plan", ALL, indirect=True)
def test_realisations_and_transforms(hip, plan):
    p = plan
    p.realise(seed=3)                                        # generic plans generate into the k buffer first
    holds(p, per_kind(p, generic="field moments k", else_="field moments"), "realise")
    p.generate(seed=5)
    holds(p, "field moments k", "generate")
    p.execute_c2r()                                          # the k buffer is only read
    holds(p, "field moments k", "generate -> execute_c2r")
    p.upload_real(real_field(p))                             # a field without moments
    holds(p, "field k", "upload_real")
    p.execute_r2c()                                          # tiled kernels transform in place: the field is consumed
    holds(p, per_kind(p, generic="field k", else_="k"), "upload_real -> execute_r2c")
    refused(p, lambda: p.realise(noise="resident"), NO_DEVIATES)
    noise = cpu_ref.reference_noise(11, p.nx * p.ny * (p.nz // 2 + 1))
    p.realise(noise=noise)                                   # host deviates stay resident as float64
    holds(p, "field moments k noise64", "realise(noise=host array)")
    p.realise(noise="resident")
    holds(p, "field moments k noise64", "realise(noise=resident)")
    p.scale_z(np.full(p.nz, 0.5))                            # changed in place: the moments are stale
    holds(p, "field k noise64", "scale_z")
    p.measure_power(edges_of(p), hip.RF_POWER_FROM_KSPACE)   # reads the k buffer
    holds(p, "field k noise64", "measure_power from k space")
    p.measure_power(edges_of(p), hip.RF_POWER_FROM_FIELD)    # tiled: field consumed, k buffer untouched; generic: field kept, delta(k) in the k buffer
    holds(p, per_kind(p, generic="field k noise64", else_="k noise64"), "measure_power from the field")
    if p.kind != "generic":
        refused(p, p.execute_r2c, NO_FIELD_IN_W)


@pytest.mark.parametrize("plan", ALL, indirect=True)
def test_measure_power_from_field_without_k_space(hip, plan):
    p = plan
    p.upload_real(real_field(p))
    holds(p, "field", "upload_real")
    p.measure_power(edges_of(p), hip.RF_POWER_FROM_FIELD)
    holds(p, per_kind(p, generic="field k", else_=""), "measure_power from the field")


@pytest.mark.parametrize("plan", SINGLE, indirect=True)
def test_gradient_and_second_order_potential(hip, plan):
    p = plan
    dk = dk_of(p)
    p2 = lambda axis: p.execute_gradient(axis, 1.0, dk[axis], hip.RF_GRAD_FROM_POTENTIAL2)
    p.generate(seed=1)
    p.realise_potential(seed=2)                              # (after generate the k buffer holds a spectrum whichever way the potential is stored)
    holds(p, "field moments k", "generate -> realise_potential")
    refused(p, lambda: p2(0), NO_P2)
    p.execute_gradient(0, 1.0, dk[0], hip.RF_GRAD_FROM_KSPACE)          # consumes the k buffer on both kinds of plan
    holds(p, "field moments", "execute_gradient from k space")
    refused(p, lambda: p.execute_gradient(0, 1.0, dk[0], hip.RF_GRAD_FROM_KSPACE), NO_K)
    p.execute_gradient(1, 1.0, dk[1], hip.RF_GRAD_FROM_POTENTIAL)       # tiled: the component passes through the k buffer; generic: inside the x pass
    holds(p, per_kind(p, tiled="field moments k", generic="field moments"), "execute_gradient from the potential")
    p.lensing_potential(1.0 / (1.0 + np.arange(p.nz)), SPACING, 2)      # the k buffer's memory becomes the auxiliary field
    holds(p, "field moments aux", "lensing_potential")
    p.lpt2_source(dk)                                        # the k buffer holds nothing afterwards, on either kind of plan
    holds(p, "field", "lpt2_source")
    refused(p, lambda: p2(0), NO_P2)
    p.lpt2_potential(dk)                                     # the k buffer holds S(k), the field buffer is as after execute_r2c
    holds(p, per_kind(p, tiled="k", generic="field k"), "lpt2_potential")
    p2(2)
    holds(p, "field moments k", "execute_gradient from the second-order potential")
    p.realise_potential(seed=3)                              # the stored potential is rewritten: the second-order one is stale
    holds(p, "field moments k", "realise_potential")
    refused(p, lambda: p2(0), NO_P2)
    p.lpt2_potential(dk)
    p.save_potential()                                       # ... and so it is when the potential is stored from the k buffer
    refused(p, lambda: p2(0), NO_P2)
    holds(p, per_kind(p, tiled="k", generic="field k"), "lpt2_potential -> save_potential")


@pytest.mark.parametrize("plan", ["tiled64", "tiled128"], indirect=True)
def test_lognormal_realisation_keeps_the_auxiliary_field(hip, plan):
    p = plan
    p.generate(seed=1)
    p.realise(seed=2)
    holds(p, "field moments k", "generate -> realise")
    p.lensing_potential(1.0 / (1.0 + np.arange(p.nz)), SPACING, 1)
    holds(p, "field moments aux", "lensing_potential")
    p.set_z_tables(np.ones(p.nz))
    p.realise_lognormal(seed=3)                              # claims no k space, and leaves the auxiliary field alone
    holds(p, "field moments aux", "lensing_potential -> realise_lognormal")
    p.lognormal(np.ones(p.nz), np.zeros(p.nz), 1.0)
    holds(p, "field aux", "lognormal")
    p.generate(seed=4)                                       # the k buffer's memory is a spectrum again
    holds(p, "field k", "generate")


@pytest.mark.parametrize("plan", SINGLE, indirect=True)
def test_particles_paint_and_gather(hip, plan):
    p = plan
    inv_h = [1.0 / SPACING] * 3
    for axis in range(3):
        p.particles_upload(axis, (0.1 * SPACING * real_field(p, seed=axis)).astype(p.real_dtype))
    holds(p, "", "particles_upload")
    refused(p, lambda: p.particles_gather(inv_h, 0), "no real-space field on the device")
    assert p.particles_paint(inv_h) == 0                     # the painted density contrast is the current field, without moments
    holds(p, "field counts", "particles_paint")
    assert p.particles_gather(inv_h, 0) == 0                 # changes nothing but the gathered values
    holds(p, "field counts", "particles_gather")
    p.execute_r2c()                                          # the painted field lies in the primary buffer
    holds(p, per_kind(p, tiled="k counts", generic="field k counts"), "particles_paint -> execute_r2c")


@pytest.mark.parametrize("plan", ALL, indirect=True)
def test_batches(hip, plan):
    p = plan
    p.realise_batch([1, 2])                                  # slab pipeline: realisation i lies in buffer i % 2 -- the last of two in the second
    holds(p, per_kind(p, generic="field moments k", else_="field moments"), "realise_batch of 2")
    if p.kind == "slab":
        refused(p, p.execute_r2c, NO_FIELD_IN_W)
        refused(p, lambda: p.measure_power(edges_of(p), hip.RF_POWER_FROM_FIELD), NO_FIELD_IN_W)
        holds(p, "field moments", "the refusals")
    p.realise_batch([1, 2, 3])
    holds(p, per_kind(p, generic="field moments k", else_="field moments"), "realise_batch of 3")
    p.execute_r2c()                                          # generic plans leave the field, and so its moments, untouched
    holds(p, per_kind(p, generic="field moments k", else_="k"), "realise_batch of 3 -> execute_r2c")


@pytest.mark.parametrize("plan", ["slab"], indirect=True)
def test_slab_pipeline_and_exchange_chunks(hip, plan):
    p = plan
    p.realise(seed=3)                                        # forward half, exchange, gathering z pass, moments
    holds(p, "field moments", "realise")
    p.set_exchange_chunks(1)                                 # the layout between the passes may change: no field survives it, the moments do
    holds(p, "moments", "set_exchange_chunks")
    refused(p, p.execute_r2c, NO_FIELD_IN_W)
    p.generate(seed=5)
    p.execute_c2r()
    holds(p, "field moments k", "generate -> execute_c2r")
    p.execute_r2c()
    holds(p, "k", "execute_r2c")
