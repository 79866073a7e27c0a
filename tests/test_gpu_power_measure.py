"""The binned power spectrum on the device (rf_measure_power; rf_k_power.hip bin_sweep_kernel / bin_reduce_kernel) and
Generator.measure_power_spectrum on the hip backend -- run with -m gpu on an MI355X.

Oracle: tests/power_oracle.py, float64 numpy on the array the device itself was given.  Counts must be exact; sum_k and sum_p within
rtol 1e-9 (sums of non-negative float64 terms: n 2^-53 < 1e-10 for the < 1e6 cells here).  FROM_FIELD is compared with a second plan's
execute_r2c + FROM_KSPACE on the same field: tiled plans sweep the packed array of the forward passes and untangle the slot kz = 0 in
the kernel with the unpack kernel's formula and rounding, so only the summation order differs.

Shapes: tiled plans (16, 16, 16) both dtypes and (16, 32, 64); generic plans one workgroup with rows shorter than a wave (4, 6, 8),
(40, 60, 80), a ragged last workgroup (30, 14, 22), (154, 28, 44) complex128, and rows longer than a workgroup (4, 6, 1200).  Rows of
at least 33 cells -- (16, 32, 64), (40, 60, 80), (4, 6, 1200) -- take the run-based reduction of the sweep, shorter ones the loop over bins.
Tiled (16, 16, 512): rows of 257 cells, a second kz step that holds the Nyquist plane alone, which the packed FROM_FIELD sweep untangles
from slot kz = 0 of two rows.  More rows than the sweep's workgroups take in one stride: tests/test_gpu_at_scale.py.  The launch shape
is mirrored here (power_shape) and the mirror is asserted against the block shapes written out, at bin counts on both sides of its
thresholds 128 (workgroup cap) and 512 (waves per workgroup).

Generator, complex64, measure_power_spectrum(field) against the oracle on np.fft.rfftn(field): the float32 FFT's rounding is relative to
the largest amplitude, not to each bin's, so no bound follows from the formats.  Measured once on an MI355X: largest relative bin
difference 1.106e-07 on (32, 32, 32) and 6.338e-08 on (40, 60, 80) (complex128: 2.8e-15 and 6.4e-15); asserted at ten times that, and never looser than 1e-3 (a plumbing error shows as >= 1e-2)."""
import numpy as np
import pytest

import power_oracle as po
from power_oracle import C64, C128

pytestmark = pytest.mark.gpu

SPACING = 2.5
TILED = [((16, 16, 16), C64), ((16, 16, 16), C128), ((16, 32, 64), C64),
         ((16, 16, 512), C64)]        # nz/2 + 1 = 257: a second kz step of one cell, the Nyquist plane the packed sweep untangles
GENERIC = [((4, 6, 8), C64), ((4, 6, 8), C128), ((40, 60, 80), C64), ((30, 14, 22), C64), ((154, 28, 44), C128),
           ((4, 6, 1200), C64)]        # rows of several waves and several steps: the run-based reduction, a ragged last step
# largest relative bin difference of Pk measured for complex64 (see the module docstring), per shape
C64_MEASURED = {(32, 32, 32): 1.106e-07, (40, 60, 80): 6.338e-08}


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


def make_plan(hip, shape, dtype, kgrid=True):
    from randomfield_amd import powertools
    plan = hip.DevicePlan(*shape, dtype)
    if kgrid:
        plan.set_kgrid(*powertools.ksq_axes(*shape, SPACING))
    return plan


def edge_sets(shape):
    """16 linear bins over the whole range, and 12 log-spaced bins strictly inside it (cells fall off both ends)"""
    from randomfield_amd import powertools
    k_min, k_max = powertools.grid_k_range(shape, SPACING)
    return [powertools.default_k_edges(shape, SPACING, 16), np.geomspace(1.7 * k_min, 0.8 * k_max, 13)]


def real_field(shape, dtype, seed=4):
    rt = np.float32 if dtype == C64 else np.float64
    return np.ascontiguousarray(np.random.RandomState(seed).normal(size=shape).astype(rt))


@pytest.mark.parametrize("shape,dtype", TILED + GENERIC, ids=po.ids)
def test_from_kspace_against_the_oracle(hip, shape, dtype):
    plan = make_plan(hip, shape, dtype)
    src = po.spectrum(shape, dtype)
    plan.upload_k(src)
    total = int(po.weights(shape).sum()) - 1
    for edges in edge_sets(shape):
        want = po.oracle(src, shape, SPACING, edges)
        got = plan.measure_power(edges, hip.RF_POWER_FROM_KSPACE)
        po.assert_sums(got, want, "FROM_KSPACE %s" % (shape,))
        assert int(got[0].sum()) + want[3] == total
        again = plan.measure_power(edges, hip.RF_POWER_FROM_KSPACE)
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two calls differ"
        assert plan.elapsed_ms() > 0
    assert int(plan.measure_power(edge_sets(shape)[0])[0].sum()) == total        # the default edges drop nothing but DC
    assert np.array_equal(plan.download_k(), src), "FROM_KSPACE changed the k buffer"
    plan.close()


@pytest.mark.parametrize("shape,dtype", TILED + GENERIC, ids=po.ids)
def test_from_field_equals_r2c_then_from_kspace(hip, shape, dtype):
    field = real_field(shape, dtype)
    two = make_plan(hip, shape, dtype)
    two.upload_real(field)
    two.execute_r2c()
    khat = two.download_k()
    for i, edges in enumerate(edge_sets(shape)):
        want = two.measure_power(edges, hip.RF_POWER_FROM_KSPACE)
        po.assert_sums(want, po.oracle(khat, shape, SPACING, edges), "r2c + FROM_KSPACE %s" % (shape,))
        one = make_plan(hip, shape, dtype)                 # a fresh plan: it never had a k-space array
        one.upload_real(field)
        got = one.measure_power(edges, hip.RF_POWER_FROM_FIELD)
        po.assert_sums(got, want, "FROM_FIELD %s" % (shape,))
        assert one.elapsed_ms() > 0
        if one.tiled:
            with pytest.raises(RuntimeError, match="no k-space data"):
                one.download_k()
            with pytest.raises(RuntimeError, match="no real-space field"):
                one.download_real()
            with pytest.raises(RuntimeError, match="no real-space field"):       # consumed: a second measurement needs a new field
                one.measure_power(edges, hip.RF_POWER_FROM_FIELD)
            one.upload_real(field)
        else:
            assert np.array_equal(one.download_real(), field), "a generic plan keeps its field"
            assert np.array_equal(one.download_k(), khat), "a generic plan leaves delta(k) in the k buffer"
        again = one.measure_power(edges, hip.RF_POWER_FROM_FIELD)
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two calls differ"
        one.close()
    two.close()


def power_shape(shape, nbins):
    """the mirror of bin_launch_shape with rf_measure_power's table (rf_k_power.hip): (tx, ty, workgroups, LDS bytes, workgroup cap)"""
    nx, ny, nz = shape
    nthreads = 256 if nbins <= 512 else 128
    tx = 1
    while tx < nthreads and tx < nz // 2 + 1:
        tx *= 2
    ty = nthreads // tx
    cap = 2048 if nbins <= 128 else 1024
    grid = min(max(-(-(nx * ny) // ty), 1), cap)
    lds = ((nbins + 1) + 3 * (nthreads // 64) * nbins) * 8
    assert lds <= 65536
    return tx, ty, grid, lds, cap


@pytest.mark.parametrize("nbins,block", [(128, 256), (129, 256), (512, 256), (513, 128), (1024, 128)])
def test_bin_count_classes(hip, nbins, block):
    """bin counts on both sides of the thresholds of rf_measure_power's launch shape: 128 (workgroup cap) and 512 (four waves per
    workgroup, then two: three and five kz steps on the 601-cell rows), and 1024"""
    shape, dtype = (4, 6, 1200), C64
    tx, ty, grid, lds, cap = power_shape(shape, nbins)
    assert (tx, ty, grid) == (block, 1, 24) and cap == (2048 if nbins <= 128 else 1024)
    assert -(-601 // tx) == {256: 3, 128: 5}[block]          # kz steps of a row of 601 cells
    from randomfield_amd import powertools
    edges = powertools.default_k_edges(shape, SPACING, nbins)
    plan = make_plan(hip, shape, dtype)
    src = po.spectrum(shape, dtype)
    plan.upload_k(src)
    got = plan.measure_power(edges, hip.RF_POWER_FROM_KSPACE)
    po.assert_sums(got, po.oracle(src, shape, SPACING, edges), "%d bins" % nbins)
    again = plan.measure_power(edges, hip.RF_POWER_FROM_KSPACE)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two calls differ"
    assert np.array_equal(plan.download_k(), src)
    plan.close()


def test_tiled_from_field_leaves_an_existing_k_buffer_alone(hip):
    shape = (16, 16, 16)
    plan = make_plan(hip, shape, C64)
    src = po.spectrum(shape, C64)
    plan.upload_k(src)
    plan.upload_real(real_field(shape, C64))
    plan.measure_power(edge_sets(shape)[0], hip.RF_POWER_FROM_FIELD)
    assert np.array_equal(plan.download_k(), src)
    plan.close()


def test_refusals_leave_the_plan_usable(hip):
    shape = (16, 16, 16)
    K, F = hip.RF_POWER_FROM_KSPACE, hip.RF_POWER_FROM_FIELD
    edges = edge_sets(shape)[0]
    src = po.spectrum(shape, C64)
    plan = make_plan(hip, shape, C64)
    with pytest.raises(RuntimeError, match="no k-space data"):
        plan.measure_power(edges, K)
    with pytest.raises(RuntimeError, match="no real-space field"):
        plan.measure_power(edges, F)
    plan.upload_k(src)
    with pytest.raises(RuntimeError, match="source"):
        plan.measure_power(edges, 7)
    with pytest.raises(RuntimeError, match="increasing"):
        plan.measure_power([0.1, 0.3, 0.3, 0.5], K)
    with pytest.raises(RuntimeError, match="increasing"):
        plan.measure_power([0.5, 0.3], K)
    with pytest.raises(RuntimeError, match="negative"):
        plan.measure_power([-0.1, 0.3], K)
    with pytest.raises(RuntimeError, match="nbins"):
        plan.measure_power(np.linspace(0.0, 5.0, 1026), K)
    with pytest.raises(RuntimeError, match="nbins"):
        plan.measure_power([0.3], K)
    po.assert_sums(plan.measure_power(edges, K), po.oracle(src, shape, SPACING, edges), "after the refusals")
    many = np.linspace(0.0, 5.0, 1025)                       # 1024 bins are accepted (two waves per workgroup)
    po.assert_sums(plan.measure_power(many, K), po.oracle(src, shape, SPACING, many), "1024 bins")
    one = np.array([0.0, 5.0])
    po.assert_sums(plan.measure_power(one, K), po.oracle(src, shape, SPACING, one), "1 bin")
    assert np.array_equal(plan.download_k(), src)
    plan.close()
    nogrid = make_plan(hip, shape, C64, kgrid=False)
    nogrid.upload_k(src)
    with pytest.raises(RuntimeError, match="rf_set_kgrid"):
        nogrid.measure_power(edges, K)
    assert np.array_equal(nogrid.download_k(), src)
    nogrid.close()
    ranked = hip.DevicePlan(*shape, C64, nranks=2, rank=0)
    with pytest.raises(RuntimeError, match="single-rank"):
        ranked.measure_power(edges, K)
    ranked.close()
    c2c = hip.DevicePlan(*shape, C64, unpacked=True)
    with pytest.raises(RuntimeError, match="c2c"):
        c2c.measure_power(edges, K)
    data = (np.arange(16 ** 3) % 7).astype(C64).reshape(shape)
    c2c.upload_c(data)
    c2c.execute_c2c(inverse=False)
    assert np.allclose(c2c.download_c(), np.fft.fftn(data), atol=1e-2)      # still works
    c2c.close()


@pytest.mark.parametrize("dtype", [C64, C128], ids=po.ids)
@pytest.mark.parametrize("shape,seed", [((32, 32, 32), 123), ((40, 60, 80), 7)], ids=["32x32x32", "40x60x80"])
def test_generator_hip_backend(hip, shape, seed, dtype):
    from randomfield_amd import Generator, powertools
    gen = Generator(*shape, SPACING, backend="hip", rng="native", dtype=dtype)
    field = gen.generate_delta_field(seed=seed, save_potential=False).copy()
    edges = powertools.default_k_edges(shape, SPACING, 16)
    res = gen.measure_power_spectrum(nbins=16)
    assert res.dtype.names == ("k", "Pk", "nmodes") and len(res) == 16
    assert int(res["nmodes"].sum()) == int(po.weights(shape).sum()) - 1
    po.assert_matches_table(res, gen.power, shape, SPACING, edges, "hip %s" % (shape,))
    assert np.array_equal(gen.download_field(), field), "the host copy of the field must survive the measurement"
    # an explicit field, against the oracle on numpy's float64 transform of it
    res2 = gen.measure_power_spectrum(field, k_edges=edges)
    khat = np.fft.rfftn(field.astype(np.float64), axes=(0, 1, 2))
    want = powertools.power_estimate(*po.oracle(khat, shape, SPACING, edges)[:3], shape=shape, spacing=SPACING)
    assert np.array_equal(res2["nmodes"], want["nmodes"])
    assert np.max(np.abs(res2["k"] / want["k"] - 1.0)) <= po.RTOL
    err = float(np.max(np.abs(res2["Pk"] / want["Pk"] - 1.0)))
    print("Generator %s %s: largest relative bin difference of Pk %.3e" % (shape, po.ids(dtype), err))
    if dtype == C128:
        assert err <= po.RTOL
    else:
        measured = C64_MEASURED[shape]
        bound = min(10.0 * measured, 1e-3)
        assert err <= bound
    # the current field and the uploaded copy of it are the same bits: the same sums, bit for bit
    assert all(np.array_equal(res[n], res2[n]) for n in res.dtype.names)
