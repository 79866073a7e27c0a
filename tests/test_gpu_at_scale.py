"""The grid-stride loops, the second kz step and the padded potential pitch of the LPT, paint and P(k) kernels, at the smallest sizes
that reach them -- run with -m gpu on an MI355X.  The four per-feature files (tests/test_gpu_gradient.py, test_gpu_lpt2.py,
test_gpu_power_measure.py, test_gpu_particles.py) stay below every cap in this table; the 512^3 and 1024^3 configurations live above it:

    kernel                                               launch cap (source)                               a second stride needs
    derivative_kernel (gradient and Hessian)             min(nblk, 4096) workgroups of ty = 256 / tx rows, nx ny / ty > 4096
                                                         tx the power of two covering nz/2 + 1, <= 256
                                                         (rf_k_misc.hip launch_derivative)
    save_potential_kernel, scale_copy_kernel             4096 x 256 threads (rf_k_misc.hip grid_for)       > 1 048 576 cells
    cic_convert_kernel, cic_paint_global_kernel          4096 x 256 threads (rf_k_particles.hip sweep_grid) > 1 048 576 cells / particles
    lpt2_accumulate_kernel, particles_accumulate_kernel  4096 x 256 threads of 16 bytes                    > 4 194 304 cells (float32, 4 per
                                                         (grid_for, sweep_grid)                            lane), > 2 097 152 (float64, 2)
    bin_sweep_kernel (rf_measure_power)                  2048 workgroups up to 128 bins, else 1024         nx ny > cap ty
                                                         (rf_k_power.hip bin_launch_shape)

    the kz loop inside a row of derivative_kernel and bin_sweep_kernel takes a second step when nz/2 + 1 > tx.
    float32 plans with nz >= 512 keep the potential in rows of nz/2 + 64 cells (rf_capi.hip rf_plan_create), below that nz/2 + 2.

Every test opens with a regime guard: a plain assert, from the shape and the literal cap, that the launch it is named for strides --
a shape shrunk back under the cap fails there instead of passing for nothing.

Oracles, helpers and tolerances are those of the four files, imported as they are: tests/lpt2_oracle.py, cic_oracle.py and
power_oracle.py on what the device itself holds.  k space within 4 eps with exact zeros; fields within 1e-5 rms (float32) / 1e-11 rms
(float64) per transform; the stored potential within 1e-5 of the largest magnitude (test_gpu_parity.py
test_fused_potential_store_native); counts and painted fields bit for bit; the accumulate step within eps/2 (first) and
2 eps (|Q| + |c W|) (add).  P(k): rtol 1e-9 -- sequential float64 summation of n non-negative terms errs by at most n 2^-53 per side,
the largest half spectrum here has 1.2e6 cells, twice that bound is under 3e-10.  Every check prints measured / bound."""
import numpy as np
import pytest

import cic_oracle as cic
import lpt2_oracle as orc
import power_oracle as po
import test_gpu_gradient as tg
import test_gpu_lpt2 as tl
import test_gpu_particles as tp
import test_gpu_power_measure as tpm

pytestmark = pytest.mark.gpu

C64, C128 = np.complex64, np.complex128
CAP = 4096                       # workgroups of grid_for, sweep_grid and launch_derivative (256 * 16)
THREADS = CAP * 256              # ... of 256 threads: cells, particles or 16-byte vectors per stride
SPACING = tl.SPACING
assert tg.SPACING == SPACING


def _ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else ("c64" if v == C64 else ("c128" if v == C128 else str(v)))


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


def row_block(nz, nthreads=256):
    """(tx, ty) of the row kernels: tx the power of two covering nz/2 + 1, at most nthreads"""
    tx = 1
    while tx < nthreads and tx < nz // 2 + 1:
        tx <<= 1
    return tx, nthreads // tx


def vec_lanes(dtype):
    return 4 if dtype == C64 else 2


# ---- B1: potential, gradient, Hessian, 2LPT ----
# (shape, dtype): tiled, what must stride
LPT = {((128, 128, 512), C64): (True, ("rows", "cells", "accumulate", "kz")),       # rows 4 strides, cells 5 (ragged), vectors 2; pitch 320
       ((64, 128, 512), C128): (True, ("rows", "cells", "accumulate", "kz")),       # rows 2 strides, vectors 2
       ((66, 70, 520), C64): (False, ("rows", "cells", "kz")),                      # rows 4096 + 524; pitch 324 under the generic x pass
       ((66, 70, 520), C128): (False, ("rows", "cells", "accumulate", "kz"))}       # vectors 1 048 576 + 152 624


@pytest.mark.parametrize("shape,dtype", list(LPT), ids=_ids)
def test_potential_gradient_hessian_lpt2(hip, shape, dtype):
    tiled, strides = LPT[shape, dtype]
    nx, ny, nz = shape
    nzh = nz // 2 + 1
    tx, ty = row_block(nz)
    # regime guards
    if "rows" in strides:
        assert nx * ny > CAP * ty
    if "cells" in strides:
        assert nx * ny * nzh > THREADS
    if "accumulate" in strides:
        assert nx * ny * nz > THREADS * vec_lanes(dtype)
    if "kz" in strides:
        assert nzh > tx
    padded = dtype == C64
    assert nz >= 512

    plan = tl.make_plan(hip, shape, dtype)
    assert plan.tiled == tiled
    src = tl.spectrum(shape, dtype)
    dk = orc.dk_of(shape, SPACING)
    K, P, P2 = hip.RF_GRAD_FROM_KSPACE, hip.RF_GRAD_FROM_POTENTIAL, hip.RF_GRAD_FROM_POTENTIAL2

    # 1. the stored potential, in rows of the padded pitch on float32 plans
    plan.upload_k(src)
    before = plan.nbytes
    pot = tl.store_potential(plan, src)
    if padded:
        assert plan.nbytes - before == nx * ny * (nz // 2 + 64) * 8
    else:
        assert plan.nbytes - before == nx * ny * nzh * 16

    # 2. ... is delta(k) / k^2
    k2 = orc.ksq_grid(shape, SPACING)
    k2[0, 0, 0] = 1.0
    ref = src.astype(C128) / k2
    ref[0, 0, 0] = 0.0
    err, big = float(np.max(np.abs(pot - ref))), float(np.max(np.abs(ref)))
    print("potential: max err / (1e-5 max|ref|) = %.3g" % (err / (1e-5 * big)))
    assert pot.dtype == dtype and pot[0, 0, 0] == 0 and err <= 1e-5 * big
    del ref, k2

    # 3. k space, cell by cell
    scale = 1.5
    for a, b in orc.PAIRS:
        plan.load_hessian(a, b, scale, dk[a], dk[b], P)
        tl.assert_elementwise(plan.download_k(), orc.hessian_k(pot, shape, SPACING, a, b, scale, False),
                              orc.hessian_factor(shape, SPACING, a, b, scale), dtype)
    for axis in range(3):
        plan.load_gradient(axis, scale, dk[axis], P)
        tg.assert_elementwise(plan.download_k(), tg.want_k(pot, shape, axis, scale, False), dtype)
    plan.upload_k(src)
    plan.load_hessian(0, 2, scale, dk[0], dk[2], K)
    tl.assert_elementwise(plan.download_k(), orc.hessian_k(src, shape, SPACING, 0, 2, scale, True),
                          orc.hessian_factor(shape, SPACING, 0, 2, scale), dtype)
    plan.upload_k(src)
    plan.load_gradient(2, scale, dk[2], K)
    tg.assert_elementwise(plan.download_k(), tg.want_k(src, shape, 2, scale, True), dtype)

    # 4. fields (scale 1: the Hessian oracles are the ones the source needs below)
    H = orc.hessian_fields(pot, shape, SPACING)
    for a, b in ((1, 1), (0, 2)):
        plan.execute_hessian(a, b, 1.0, dk[a], dk[b], P)
        got = plan.download_real().copy()
        tl.assert_field(got, H[a, b], dtype, "H_%d%d" % (a, b))
        if not tiled:
            plan.load_hessian(a, b, 1.0, dk[a], dk[b], P)
            plan.execute_c2r()
            assert np.array_equal(plan.download_real(), got)
    for axis in (0, 2):
        plan.execute_gradient(axis, 1.0, dk[axis], P)
        got = plan.download_real().copy()
        tg.assert_field(got, tg.irfftn(tg.want_k(pot, shape, axis, 1.0, False), shape), dtype, "axis %d" % axis)
        if not tiled:
            plan.load_gradient(axis, 1.0, dk[axis], P)
            plan.execute_c2r()
            assert np.array_equal(plan.download_real(), got)

    # 5. the second-order source, potential and displacement
    plan.lpt2_source(dk)
    S = plan.download_real().copy()
    tl.assert_source(S, H, dtype, "of the stored potential")
    del H
    plan.lpt2_source(dk)
    assert np.array_equal(plan.download_real(), S)
    plan.lpt2_potential(dk)
    Sk = plan.download_k()
    want_k = orc.rfftn(S)
    err, rms = float(np.max(np.abs(Sk - want_k))), float(np.sqrt(np.mean(np.abs(want_k) ** 2)))
    print("S(k): max err / (TOL rms) = %.3g" % (err / (tl.TOL[dtype] * rms)))
    assert err <= tl.TOL[dtype] * rms
    del Sk, want_k
    for axis in (0, 2):
        plan.execute_gradient(axis, 3.0 / 7.0, dk[axis], P2)
        tl.assert_field(plan.download_real(), orc.displacement2_from_source(S, shape, SPACING, axis), dtype, "psi2 axis %d" % axis, 2)
    plan.load_potential(1.0)
    assert np.array_equal(plan.download_k(), pot)
    plan.close()


# ---- B2: the power spectrum ----
def power_guard(shape, nbins, nstrides, kz_steps=None):
    """the mirror of bin_launch_shape with rf_measure_power's table: more rows than cap * ty, in exactly `nstrides` strides"""
    nx, ny, nz = shape
    tx, ty = row_block(nz, 256 if nbins <= 512 else 128)
    cap = 2048 if nbins <= 128 else 1024
    assert nx * ny > cap * ty
    assert -(-(nx * ny) // (cap * ty)) == nstrides
    if kz_steps is not None:
        assert -(-(nz // 2 + 1) // tx) == kz_steps
    return tx, ty


def linear_edges(shape, nbins):
    from randomfield_amd import powertools
    return powertools.default_k_edges(shape, tpm.SPACING, nbins)


def from_kspace(hip, plan, src, shape, edges, what):
    want = po.oracle(src, shape, tpm.SPACING, edges)
    got = plan.measure_power(edges, hip.RF_POWER_FROM_KSPACE)
    po.assert_sums(got, want, what)
    assert int(got[0].sum()) + want[3] == int(po.weights(shape).sum()) - 1
    again = plan.measure_power(edges, hip.RF_POWER_FROM_KSPACE)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two calls differ"


def from_field(hip, shape, dtype, edge_list):
    """RF_POWER_FROM_FIELD on a fresh plan against a second plan's execute_r2c + FROM_KSPACE, as tests/test_gpu_power_measure.py"""
    field = tpm.real_field(shape, dtype)
    two = tpm.make_plan(hip, shape, dtype)
    two.upload_real(field)
    two.execute_r2c()
    khat = two.download_k()
    one = tpm.make_plan(hip, shape, dtype)
    for edges in edge_list:
        want = two.measure_power(edges, hip.RF_POWER_FROM_KSPACE)
        po.assert_sums(want, po.oracle(khat, shape, tpm.SPACING, edges), "r2c + FROM_KSPACE %s" % (shape,))
        one.upload_real(field)
        got = one.measure_power(edges, hip.RF_POWER_FROM_FIELD)
        po.assert_sums(got, want, "FROM_FIELD %s" % (shape,))
        if one.tiled:
            one.upload_real(field)                  # a tiled plan consumed its field
        again = one.measure_power(edges, hip.RF_POWER_FROM_FIELD)
        assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two calls differ"
    one.close()
    two.close()


def test_power_rows_longer_than_a_workgroup(hip):
    shape, dtype = (64, 64, 512), C64
    assert power_guard(shape, 16, 2, 2) == (256, 1)
    assert power_guard(shape, 200, 4, 2) == (256, 1)
    assert power_guard(shape, 1024, 4, 3) == (128, 1)
    plan = tpm.make_plan(hip, shape, dtype)
    assert plan.tiled
    src = po.spectrum(shape, dtype)
    plan.upload_k(src)
    for nbins in (16, 200, 1024):
        from_kspace(hip, plan, src, shape, linear_edges(shape, nbins), "FROM_KSPACE %s %d bins" % (shape, nbins))
    assert np.array_equal(plan.download_k(), src)
    plan.close()
    from_field(hip, shape, dtype, tpm.edge_sets(shape))       # the packed sweep: two row strides, the Nyquist cell alone in the second kz step


@pytest.mark.parametrize("shape", [(256, 256, 16), (66, 70, 520)], ids=_ids)
def test_power_both_sources(hip, shape):
    """(256, 256, 16): rows shorter than a wave, the loop over bins, two row strides of 2048 workgroups x 16 rows;
    (66, 70, 520): a generic plan, 4620 rows in strides of 2048, 2048 and 524"""
    dtype = C64
    tiled, block, nstrides = (True, (16, 16), 2) if shape[2] == 16 else (False, (256, 1), 3)
    assert power_guard(shape, 16, nstrides) == block and power_guard(shape, 12, nstrides) == block       # (the two edge sets)
    plan = tpm.make_plan(hip, shape, dtype)
    assert plan.tiled == tiled
    src = po.spectrum(shape, dtype)
    plan.upload_k(src)
    for edges in tpm.edge_sets(shape):
        from_kspace(hip, plan, src, shape, edges, "FROM_KSPACE %s" % (shape,))
    assert np.array_equal(plan.download_k(), src)
    plan.close()
    from_field(hip, shape, dtype, tpm.edge_sets(shape))


# ---- B3: particles ----
@pytest.mark.parametrize("shape", [(128, 128, 128), (130, 126, 66)], ids=_ids)
def test_paint_more_particles_than_one_stride(hip, shape):
    """(130, 126, 66): 1 081 080 particles -- the second stride of the global form ends in a partial wave -- and bricks of the tiled
    form that are partial on all three axes"""
    dtype, rt = C64, np.float32
    tiled = shape == (128, 128, 128)
    n = int(np.prod(shape))
    assert n > THREADS                                         # the global paint and the conversion stride
    if not tiled:
        assert (n - THREADS) % 64 != 0 and all(m % b for m, b in zip(shape, (8, 8, 64)))
    plan = hip.DevicePlan(*shape, dtype)
    assert plan.tiled == tiled
    assert plan.paint_geometry()[0] == (8, 8, 64)
    sets = cic.displacement_sets(shape, tp.SPACING)
    sets = {name: sets[name].astype(rt) for name in ("small", "rms3")}
    for name, s in sets.items():
        want, wdrop = cic.paint(s, tp.INV_H)
        assert wdrop == 0 and cic.total(want) == n * cic.ONE
        tp.upload(plan, s)
        tp.paint_all_forms(plan, want, 0, rt, name)
    # a NaN and an inf in the second stride
    s = sets["rms3"].copy()
    l1, l2 = THREADS + 77, n - 1
    assert THREADS < l1 < l2 < n
    p1, p2 = np.unravel_index(l1, shape), np.unravel_index(l2, shape)
    s[1][p1] = np.nan
    s[2][p2] = np.inf
    omit = np.zeros(shape, bool)
    omit[p1] = omit[p2] = True
    want, _ = cic.paint(sets["rms3"], tp.INV_H, omit=omit)
    assert cic.total(want) == (n - 2) * cic.ONE
    tp.upload(plan, s)
    tp.paint_all_forms(plan, want, 2, rt, "non-finite")
    plan.close()


@pytest.mark.parametrize("shape,dtype", [((128, 128, 512), C64), ((130, 126, 260), C64), ((130, 126, 130), C128)], ids=_ids)
def test_accumulate_more_vectors_than_one_stride(hip, shape, dtype):
    rt = tp.real_of(dtype)
    eps = np.finfo(rt).eps
    n = int(np.prod(shape))
    assert n % vec_lanes(dtype) == 0 and n // vec_lanes(dtype) > THREADS
    rng = np.random.RandomState(3)
    W1, W2, Q0 = (rng.normal(size=shape).astype(rt) for _ in range(3))
    c1, c2 = 0.75, 0.25
    plan = hip.DevicePlan(*shape, dtype)
    plan.upload_real(W1)
    plan.particles_accumulate(1, c1, first=True)
    assert np.array_equal(plan.download_real(), W1)
    Q1 = plan.particles_download(1)
    want1 = c1 * W1.astype(np.float64)
    print("first: max err / (eps/2 |c W|) = %.3g" % np.max(np.abs(Q1 - want1) / (0.5 * eps * np.abs(want1))))
    assert np.all(np.abs(Q1 - want1) <= 0.5 * eps * np.abs(want1))
    assert not plan.particles_download(0).any() and not plan.particles_download(2).any()
    plan.particles_upload(2, Q0)
    plan.upload_real(W2)
    plan.particles_accumulate(2, c2, first=False)
    assert np.array_equal(plan.download_real(), W2)
    Q2 = plan.particles_download(2)
    add = c2 * W2.astype(np.float64)
    bound = 2 * eps * (np.abs(Q0) + np.abs(add))
    print("add: max err / (2 eps (|Q| + |c W|)) = %.3g" % np.max(np.abs(Q2 - (Q0.astype(np.float64) + add)) / bound))
    assert np.all(np.abs(Q2 - (Q0.astype(np.float64) + add)) <= bound)
    assert np.array_equal(plan.particles_download(1), Q1)
    assert not plan.particles_download(0).any()
    plan.close()
