"""The power spectrum multipoles on the device (rf_measure_multipoles; rf_k_power.hip bin_sweep_kernel / bin_sweep_cells_kernel /
bin_reduce_kernel), Generator.measure_power_multipoles and the redshift-space displacements on the hip backend -- run with -m gpu
on an MI355X.

Oracle: tests/multipole_oracle.py, float64 numpy on the array the device itself was given.  Counts must be exact; sum_k, m0, m2, m4
within rtol 1e-9 (sums of non-negative float64 terms, a handful of roundings each: n 2^-53 < 1e-10 for the <= 1e6 cells here).
FROM_FIELD is compared with a second plan's execute_r2c + FROM_KSPACE on the same field (tiled plans sweep the packed array: only the
summation order differs).

Shapes are tests/test_gpu_power_measure.py's: tiled (16, 16, 16) both dtypes, (16, 32, 64), (16, 16, 512) -- rows of 257 cells whose
last, the Nyquist plane, the packed FROM_FIELD sweep untangles from slot kz = 0 of two rows; generic (4, 6, 8) both dtypes (rows shorter than a wave: the loop over bins), (40, 60, 80), (30, 14, 22) (a
ragged last workgroup), (154, 28, 44) complex128, (4, 6, 1200) (rows of several waves and steps).  Rows of at least 256 cells -- nz =
512 and 1200 here -- take the kernel with four cells per lane (runs inside a lane, a lane's first run closing the run before it, the
scan over the last runs), rows of 33 to 255 cells -- (16, 32, 64), (40, 60, 80) -- the scan with one cell per lane.  The launch
shape is mirrored here (multipole_shape) and the mirror is asserted against the block shapes written out: bin counts on both sides
of its thresholds 128 (workgroup cap), 384 and 736 (waves per workgroup: one, two and three kz steps on the 601-cell rows) and 1024;
(64, 64, 512) with 200 bins has 4096 rows for 1024 workgroups of two rows: two strides of the row loop.

Generator, measure_power_multipoles(field) against the oracle on np.fft.rfftn(field.astype(float64)): the moments M0, M2, M4 are
compared, never P2 or P4 (those cancel).  The float32 FFT's rounding is relative to the largest amplitude, not to each bin's, so no
bound follows from the formats.  Measured once on an MI355X (largest relative bin difference over the three moments and the axes
used): 1.352e-07 on (32, 32, 32) and 6.539e-08 on (40, 60, 80) (complex128: 2.9e-15 and 8.9e-15, held to 1e-9): C64_MEASURED below.  Asserted at ten times the measured value, never looser than 1e-3 (a plumbing
error shows as >= 1e-2).

Redshift-space shift: Q after particle_displacements(rsd_axis=a, f1=0.5, f2=0.8, D1=0.7) against the components of
calculate_displacement_field combined with the coefficients rounded to the real type: `first` is one rounded product (exact
comparison), the second-order term one fma on top (within one ulp of the real type at the larger of its two terms)."""
import numpy as np
import pytest

import multipole_oracle as mo
import power_oracle as po
from power_oracle import C64, C128
from test_gpu_power_measure import GENERIC, SPACING, TILED, edge_sets, make_plan, real_field

pytestmark = pytest.mark.gpu

ALL_LOS = [((16, 16, 16), C64), ((16, 16, 16), C128), ((4, 6, 8), C64), ((4, 6, 8), C128)]
# largest relative bin difference of M0, M2, M4 measured for complex64 (see the module docstring), per shape
C64_MEASURED = {(32, 32, 32): 1.352e-07, (40, 60, 80): 6.539e-08}


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


def multipole_shape(shape, nbins):
    """the mirror of bin_launch_shape with rf_measure_multipoles' table (rf_k_power.hip): (tx, ty, workgroups, LDS bytes, workgroup cap, cells per lane)"""
    nx, ny, nz = shape
    nthreads = 256 if nbins <= 384 else (128 if nbins <= 736 else 64)
    nzh = nz // 2 + 1
    cells = 4 if nzh >= 256 else 1
    span = -(-nzh // cells)
    tx = 1
    while tx < nthreads and tx < span:
        tx *= 2
    ty = nthreads // tx
    cap = 2048 if nbins <= 128 else 1024
    grid = min(max(-(-(nx * ny) // ty), 1), cap)
    lds = ((nbins + 1) + 5 * (nthreads // 64) * nbins) * 8
    assert lds <= 65536
    return tx, ty, grid, lds, cap, cells


def buffer_bytes(shape, nbins):
    """the lazy buffer of the call: squared edges, result, the three tables, five planes of per-workgroup partials"""
    nx, ny, nz = shape
    grid = multipole_shape(shape, nbins)[2]
    return (1025 + 5 * 1024 + nx + ny + nz // 2 + 1 + 5 * grid * nbins) * 8


def los_of(shape, dtype):
    return (0, 1, 2) if (shape, dtype) in ALL_LOS else (2, (shape[0] + shape[1]) % 2)


def linear_edges(shape, nbins):
    from randomfield_amd import powertools
    return powertools.default_k_edges(shape, SPACING, nbins)


def from_kspace(hip, plan, src, shape, edges, los, comp, what):
    want = mo.oracle(src, shape, SPACING, edges, los, comp)
    got = plan.measure_multipoles(edges, los, hip.RF_POWER_FROM_KSPACE, comp)
    mo.assert_sums(got, want, what)
    assert plan.elapsed_ms() > 0
    again = plan.measure_multipoles(edges, los, hip.RF_POWER_FROM_KSPACE, comp)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), what + ": two calls differ"
    return got, want


@pytest.mark.parametrize("shape,dtype", TILED + GENERIC, ids=po.ids)
def test_from_kspace_against_the_oracle(hip, shape, dtype):
    plan = make_plan(hip, shape, dtype)
    src = po.spectrum(shape, dtype)
    plan.upload_k(src)
    before = plan.nbytes
    total = int(po.weights(shape).sum()) - 1
    first = True
    for comp in (None, mo.random_tables(shape)):
        for edges in edge_sets(shape):
            for los in los_of(shape, dtype):
                got, want = from_kspace(hip, plan, src, shape, edges, los, comp, "FROM_KSPACE %s los %d" % (shape, los))
                assert int(got[0].sum()) + want[5] == total
                if first:             # the lazy buffer is counted by rf_plan_nbytes
                    assert plan.nbytes == before + buffer_bytes(shape, len(edges) - 1)
                    first = False
    assert np.array_equal(plan.download_k(), src), "FROM_KSPACE changed the k buffer"
    plan.close()


@pytest.mark.parametrize("nbins,block", [(128, 256), (129, 256), (384, 256), (385, 128), (736, 128), (737, 64), (1024, 64)])
def test_bin_count_classes(hip, nbins, block):
    shape, dtype = (4, 6, 1200), C64
    tx, ty, grid, lds, cap, cells = multipole_shape(shape, nbins)
    assert (tx, ty, grid, cells) == (block, 1, 24, 4) and cap == (2048 if nbins <= 128 else 1024)
    assert -(-601 // (tx * cells)) == {256: 1, 128: 2, 64: 3}[block]          # kz steps of a row of 601 cells
    plan = make_plan(hip, shape, dtype)
    src = po.spectrum(shape, dtype)
    plan.upload_k(src)
    from_kspace(hip, plan, src, shape, linear_edges(shape, nbins), 2, mo.random_tables(shape), "%d bins" % nbins)
    from_kspace(hip, plan, src, shape, linear_edges(shape, nbins), 0, None, "%d bins" % nbins)
    assert np.array_equal(plan.download_k(), src)
    plan.close()


def test_more_rows_than_one_stride(hip):
    shape, dtype, nbins = (64, 64, 512), C64, 200
    tx, ty, grid, lds, cap, cells = multipole_shape(shape, nbins)
    assert (tx, ty, grid, cap, cells) == (128, 2, 1024, 1024, 4)  # 257 cells of a row on 128 lanes of four cells
    assert -(-(shape[0] * shape[1]) // (cap * ty)) == 2          # two strides of the row loop
    plan = make_plan(hip, shape, dtype)
    src = po.spectrum(shape, dtype)
    plan.upload_k(src)
    from_kspace(hip, plan, src, shape, linear_edges(shape, nbins), 2, mo.random_tables(shape), "two strides")
    from_kspace(hip, plan, src, shape, linear_edges(shape, nbins), 1, None, "two strides")
    assert np.array_equal(plan.download_k(), src)
    plan.close()


@pytest.mark.parametrize("shape,dtype", TILED + GENERIC, ids=po.ids)
def test_from_field_equals_r2c_then_from_kspace(hip, shape, dtype):
    field = real_field(shape, dtype)
    two = make_plan(hip, shape, dtype)
    two.upload_real(field)
    two.execute_r2c()
    khat = two.download_k()
    K, F = hip.RF_POWER_FROM_KSPACE, hip.RF_POWER_FROM_FIELD
    tables = mo.random_tables(shape)
    for i, edges in enumerate(edge_sets(shape)):
        for los, comp in zip(los_of(shape, dtype), (None, tables, tables)):
            want = two.measure_multipoles(edges, los, K, comp)
            mo.assert_sums(want, mo.oracle(khat, shape, SPACING, edges, los, comp), "r2c + FROM_KSPACE %s" % (shape,))
            one = make_plan(hip, shape, dtype)                 # a fresh plan: it never had a k-space array
            one.upload_real(field)
            got = one.measure_multipoles(edges, los, F, comp)
            mo.assert_sums(got, want, "FROM_FIELD %s" % (shape,))
            assert one.elapsed_ms() > 0
            if one.tiled:
                with pytest.raises(RuntimeError, match="no k-space data"):
                    one.download_k()
                with pytest.raises(RuntimeError, match="no real-space field"):
                    one.download_real()
                with pytest.raises(RuntimeError, match="no real-space field"):       # consumed: a second measurement needs a new field
                    one.measure_multipoles(edges, los, F, comp)
                one.upload_real(field)
            else:
                assert np.array_equal(one.download_real(), field), "a generic plan keeps its field"
                assert np.array_equal(one.download_k(), khat), "a generic plan leaves delta(k) in the k buffer"
            again = one.measure_multipoles(edges, los, F, comp)
            assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two calls differ"
            one.close()
    two.close()


@pytest.mark.parametrize("shape,dtype", [((16, 32, 64), C64), ((40, 60, 80), C64)], ids=po.ids)
def test_null_tables_give_measure_power(hip, shape, dtype):
    K, F = hip.RF_POWER_FROM_KSPACE, hip.RF_POWER_FROM_FIELD
    field = real_field(shape, dtype)
    plan = make_plan(hip, shape, dtype)
    plan.upload_k(po.spectrum(shape, dtype))
    for edges in edge_sets(shape):
        for source in (K, F):
            for los in (0, 2):
                if source == F:
                    plan.upload_real(field)
                count, sum_k, sum_p = plan.measure_power(edges, source)
                if source == F:
                    plan.upload_real(field)
                got = plan.measure_multipoles(edges, los, source)
                assert np.array_equal(got[0], count) and np.array_equal(got[1], sum_k)
                assert np.all(np.abs(got[2] - sum_p) <= 1e-9 * sum_p)
    plan.close()


@pytest.mark.parametrize("dtype", [C64, C128], ids=po.ids)
@pytest.mark.parametrize("shape,seed", [((32, 32, 32), 123), ((40, 60, 80), 7)], ids=["32x32x32", "40x60x80"])
def test_generator_hip_backend(hip, shape, seed, dtype):
    from randomfield_amd import Generator, powertools
    gen = Generator(*shape, SPACING, backend="hip", rng="native", dtype=dtype)
    field = gen.generate_delta_field(seed=seed, save_potential=False).copy()
    edges = powertools.default_k_edges(shape, SPACING, 16)
    khat = np.fft.rfftn(field.astype(np.float64), axes=(0, 1, 2))
    norm = SPACING ** 3 / float(np.prod(shape))
    worst = 0.0
    for los, window in ((2, None), (0, "cic"), (1, None)):
        res = gen.measure_power_multipoles(field, los=los, k_edges=edges, window=window)
        assert res.dtype.names == ("k", "P0", "P2", "P4", "nmodes") and len(res) == 16
        comp = None if window is None else powertools.window_compensation(shape, window)
        count, sum_k, m0, m2, m4, _ = mo.oracle(khat, shape, SPACING, edges, los, comp)
        assert np.array_equal(res["nmodes"], count) and int(count.sum()) == int(po.weights(shape).sum()) - 1
        assert np.max(np.abs(res["k"] * count / sum_k - 1.0)) <= po.RTOL
        # the moments back from the multipoles -- M0 = P0, M2 = (P2 / (5/2) + M0) / 3, M4 = (P4 / (9/8) + 30 M2 - 3 M0) / 35: the inverse
        # of the Legendre combinations adds a few eps of M0 -- against (V / N^2) mj / count of the oracle
        M0 = res["P0"]
        M2 = (res["P2"] / 2.5 + M0) / 3.0
        M4 = (res["P4"] / 1.125 + 30.0 * M2 - 3.0 * M0) / 35.0
        c = count.astype(np.float64)
        for name, g, w in (("M0", M0, norm * m0 / c), ("M2", M2, norm * m2 / c), ("M4", M4, norm * m4 / c)):
            err = float(np.max(np.abs(g / w - 1.0)))
            print("Generator %s %s los %d %s: largest relative bin difference %.3e" % (shape, po.ids(dtype), los, name, err))
            worst = max(worst, err)
    print("Generator %s %s: largest relative bin difference of the moments %.3e" % (shape, po.ids(dtype), worst))
    if dtype == C128:
        assert worst <= po.RTOL
    else:
        assert worst <= min(10.0 * C64_MEASURED[shape], 1e-3)
    # measure_power_spectrum(window=) is the compensated monopole; without a window it is rf_measure_power as before
    comp = gen.measure_power_spectrum(field, k_edges=edges, window="cic")
    same = gen.measure_power_multipoles(field, los=2, k_edges=edges, window="cic")
    assert comp.dtype.names == ("k", "Pk", "nmodes") and np.array_equal(comp["Pk"], same["P0"])
    plain = gen.measure_power_spectrum(field, k_edges=edges)
    assert np.all(comp["Pk"] > plain["Pk"])


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("shape,dtype", [((16, 16, 16), C64), ((16, 16, 16), C128), ((4, 6, 8), C64)], ids=po.ids)
def test_redshift_space_shift(hip, shape, dtype, order):
    from randomfield_amd import Generator
    rt = np.float32 if dtype == C64 else np.float64
    D1, f1, f2 = 0.7, 0.5, 0.8
    gen = Generator(*shape, SPACING, backend="hip", rng="native", dtype=dtype, store_potential=True)
    gen.generate_delta_field(seed=77, save_potential=True, download=False)
    psi1 = [gen.calculate_displacement_field(a, order=1).copy() for a in range(3)]
    psi2 = [gen.calculate_displacement_field(a, order=2).copy() for a in range(3)]
    assert all(p.dtype == rt for p in psi1 + psi2)
    plain = gen.particle_displacements(order=order, D1=D1)
    assert np.array_equal(gen.particle_displacements(order=order, D1=D1, rsd_axis=0, f1=0.0), plain)
    for axis in range(3):
        Q = gen.particle_displacements(order=order, D1=D1, rsd_axis=axis, f1=f1, f2=f2)
        assert Q.dtype == rt and Q.shape == (3,) + shape
        for a in range(3):
            c1 = rt(D1 * (1.0 + f1)) if a == axis else rt(D1)
            c2 = rt(D1 * D1 * (1.0 + f2)) if a == axis else rt(D1 * D1)
            first = (c1 * psi1[a]).astype(rt)
            if order == 1:
                assert np.array_equal(Q[a], first)
            else:
                # the fma before its one rounding, in extended precision (the product of two float64 does not fit a float64).  The
                # rounding is half an ulp of the result, and |result| <= 2 max(|first|, |product|): one ulp of the real type at the
                # larger term covers it whatever cancels
                prod = np.longdouble(c2) * psi2[a].astype(np.longdouble)
                want = first.astype(np.longdouble) + prod
                ulp = np.spacing(np.maximum(np.abs(first), np.abs(prod).astype(rt)))
                assert np.all(np.abs(Q[a].astype(np.longdouble) - want) <= ulp.astype(np.longdouble))
            if a != axis:
                assert np.array_equal(Q[a], plain[a]), "an axis that is not shifted changed"
        assert not np.array_equal(Q[axis], plain[axis])


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_kaiser_quadrupole_hip(hip, axis):
    from randomfield_amd import Generator
    from test_power_multipoles import kaiser_edges, quadrupole_ratio
    gen = Generator(32, 32, 32, 10.0, backend="hip", rng="reference")
    gen.generate_delta_field(seed=1)
    gen.particle_displacements(order=2, D1=0.1, rsd_axis=axis, f1=1.0, f2=1.0, download=False)
    painted = gen.paint_particles().copy()
    for los in range(3):
        res = gen.measure_power_multipoles(painted, los=los, k_edges=kaiser_edges())
        assert int(res["nmodes"].sum()) == 2102
        ratio = quadrupole_ratio(res)
        print("shift along %d, measured along %d: P2 / P0 = %.3f" % (axis, los, ratio))
        if los == axis:
            assert 0.8 <= ratio <= 1.3
        else:
            assert -0.75 <= ratio <= -0.25


def test_refusals_leave_the_plan_usable(hip):
    shape = (16, 16, 16)
    K, F = hip.RF_POWER_FROM_KSPACE, hip.RF_POWER_FROM_FIELD
    edges = edge_sets(shape)[0]
    src = po.spectrum(shape, C64)
    good = mo.random_tables(shape)
    plan = make_plan(hip, shape, C64)
    with pytest.raises(RuntimeError, match="no k-space data"):
        plan.measure_multipoles(edges, 2, K)
    with pytest.raises(RuntimeError, match="no real-space field"):
        plan.measure_multipoles(edges, 2, F)
    plan.upload_k(src)
    held = plan.nbytes
    with pytest.raises(RuntimeError, match="source"):
        plan.measure_multipoles(edges, 2, 7)
    for los in (3, -1):
        with pytest.raises(RuntimeError, match="los_axis"):
            plan.measure_multipoles(edges, los, K)
    with pytest.raises(RuntimeError, match="increasing"):
        plan.measure_multipoles([0.1, 0.3, 0.3, 0.5], 2, K)
    with pytest.raises(RuntimeError, match="negative"):
        plan.measure_multipoles([-0.1, 0.3], 2, K)
    with pytest.raises(RuntimeError, match="nbins"):
        plan.measure_multipoles(np.linspace(0.0, 5.0, 1026), 2, K)
    with pytest.raises(RuntimeError, match="nbins"):
        plan.measure_multipoles([0.3], 2, K)
    for a in range(3):
        for value in (0.0, np.nan, -2.0, np.inf):
            tabs = [t.copy() for t in good]
            tabs[a][-1] = value
            with pytest.raises(RuntimeError, match="compensation"):
                plan.measure_multipoles(edges, 2, K, tabs)
    with pytest.raises(ValueError):
        plan.measure_multipoles(edges, 2, K, (good[0], good[1], good[2][:-1]))
    assert plan.nbytes == held, "a refused call allocated"
    mo.assert_sums(plan.measure_multipoles(edges, 2, K, good), mo.oracle(src, shape, SPACING, edges, 2, good), "after the refusals")
    one = np.array([0.0, 5.0])
    mo.assert_sums(plan.measure_multipoles(one, 1, K), mo.oracle(src, shape, SPACING, one, 1), "1 bin")
    assert np.array_equal(plan.download_k(), src)
    plan.close()
    nogrid = make_plan(hip, shape, C64, kgrid=False)
    nogrid.upload_k(src)
    with pytest.raises(RuntimeError, match="rf_set_kgrid"):
        nogrid.measure_multipoles(edges, 2, K)
    assert np.array_equal(nogrid.download_k(), src)
    nogrid.close()
    ranked = hip.DevicePlan(*shape, C64, nranks=2, rank=0)
    with pytest.raises(RuntimeError, match="single-rank"):
        ranked.measure_multipoles(edges, 2, K)
    ranked.close()
    c2c = hip.DevicePlan(*shape, C64, unpacked=True)
    with pytest.raises(RuntimeError, match="c2c"):
        c2c.measure_multipoles(edges, 2, K)
    data = (np.arange(16 ** 3) % 7).astype(C64).reshape(shape)
    c2c.upload_c(data)
    c2c.execute_c2c(inverse=False)
    assert np.allclose(c2c.download_c(), np.fft.fftn(data), atol=1e-2)      # still works
    c2c.close()
