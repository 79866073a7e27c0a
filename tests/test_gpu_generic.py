"""The generic mixed-radix path (csrc/rf_generic.h, rf_k_generic.hip) at sizes where every pass has many workgroups and a ragged
last tile, value by value against the float64 oracle -- run with -m gpu on an MI355X.

The launch shape of a pass is chosen by host code (rf_k_generic.hip strided_shape, rf_generic.h generic_strided_tile /
generic_prefers_split, rows_per_block): lines per workgroup tc = 16 / 8 / 4 by axis length, dtype and form (in place for radices
2, 3, 4, 5, 8 -- "smooth" --, two buffers otherwise), 256 ... 1024 threads, the four-step form beyond.  SHAPES puts every
(dtype, form, tc) class on the x axis and on the y axis, each with >= 32 workgroups and a line count that is no multiple of tc
(nz % 4 == 0 makes nzh = nz / 2 + 1 odd, so tiles also straddle the `inner` boundary of the line addressing).

Launch classes reached, from a kernel trace of this module (rocprofv3 --kernel-trace --stats, no counters;
profiles/generic_tests_kernel_trace.csv, summarised by kernel in profiles/generic_tests_kernel_stats.csv).  Workgroup size and
workgroup count are the trace's Workgroup_Size_X and Grid_Size_X / Workgroup_Size_X; the count pins tc = lines / workgroups.  The
trace's LDS_Block_Size column holds static LDS only (0, or 512 for the row kernel's reduction), so the dynamic LDS bytes below are
the launchers' own formula (strided_shape / row_shape) for the class the trace shows.  axis = generic_axis_kernel, lines =
generic_lines_kernel (four-step: step 1 / step 3), row = generic_row_c2r_kernel (generic_row_r2c_kernel: same shape).

  shape, dtype            axis  n     form        kernel  tc  threads  LDS bytes      workgroups (lines)
  (200, 300, 400) c64     x     200   smooth      axis    16  256      27600          3769  (60300)
                          y     300   smooth      axis    16  512      41408          2513  (40200)
                          z     200   smooth      row     8   256      16400          7500  (60000 rows)
  (200, 300, 400) c128    x / y             smooth      axis    16  512 / 1024  54800 / 82208  3769 / 2513
  (250, 126, 1000) c64    y     126   not smooth  axis    16  256      33264          7829  (125250)
                          z     500   smooth      row     8   256      41008          3938  (31500 rows)
  (250, 126, 1000) c128   y     126   not smooth  axis    16  512      66528          7829;   z: 4 rows, 7875 workgroups
  (1000, 12, 1000) c64    x     1000  smooth      axis    16  1024     138000         376   (6012)
  (1000, 12, 1000) c128   x     1000  smooth      axis    8   1024     146000         752   (6012)
  (12, 1000, 1000)        y     1000  as the x axis above: 376 (c64) / 752 (c128) workgroups of 1024 threads
  (1000, 1000, 24)        x, y  1000  smooth      axis    16 / 8  1024  138000 / 146000  813 / 1625 (13000; c128: a multiple of 8)
  (154, 280, 444) c64     x     154   not smooth  axis    16  256      40656          3903  (62440)
                          y     280   not smooth  axis    16  512      73920          2147  (34342)
                          z     222   not smooth  row     8   256      33744          5390  (43120 rows)
  (154, 280, 444) c128    x / y       not smooth  axis    16  512 / 1024  81312 / 147840  3903 / 2147;   z: 4 rows, 10780 workgroups
  (126, 250, 40)          x     126   not smooth  axis    16  256 / 512  33264 / 66528  329   (5250)
  (1200, 30, 40) c64      x     1200  smooth      axis    8   1024     88800          79    (630)
  (1200, 30, 40) c128     x     1200  smooth      axis    4   1024     98400          158   (630)
  (2400, 30, 40) c64      x     2400  smooth      axis    4   1024     100800         158   (630)
  (2400, 30, 40) c128     x     50 x 48           lines   16  256      13712 / 13152  1890 / 1969 (630 x 48 / 630 x 50)
  (350, 30, 40) c64       x     350   not smooth  axis    16  1024     92400          40    (630)
  (350, 30, 40) c128      x     350   not smooth  axis    8   1024     95200          79    (630)
  (700, 30, 40) c64       x     700   not smooth  axis    8   1024     95200          79    (630)
  (700, 30, 40) c128      x     700   not smooth  axis    4   1024     100800         158   (630)
  (1400, 30, 40) c64      x     1400  not smooth  axis    4   1024     100800         158   (630)
  (1400, 30, 40) c128     x     40 x 35           lines   16  256      10960 / 18480  1379 / 1575
  (30, n, 40)             y     the same classes and counts as (n, 30, 40) on the x axis, n = 1200, 2400, 350, 700, 1400
  (4000, 40, 24) c64      x     80 x 50           lines   16  256      11040 / 6912   1625 / 2600 (520 x 50 / 520 x 80)
  (4000, 40, 24) c128     x     80 x 50           lines   16  256      21920 / 13712  1625 / 2600
  (2000, 40, 24) c128     x     50 x 40           lines   16  256      13712 / 10960  1300 / 1625
  (40, 4000, 24)          y     80 x 50           lines   as (4000, 40, 24)
  c2c (200, 300, 400)     z     400   smooth      axis    4   256      16800 / 32800  15000 (60000 lines, inner = 1)
  c2c (12, 1000, 1000)    z     1000  smooth      axis    4   512 / 1024  42000 / 82000  3000
  c2c (154, 280, 444)     z     444   not smooth  axis    4   256 / 512  31968 / 63936  10780
  c2c (12, 10, 7000) c64  z     7000  not smooth  axis    1   256      112000 (no tables: the fallback)  120
  c2c (12, 10, 3500) c128 z     3500  not smooth  axis    1   256      112000 (no tables: the fallback)  120
  (1000, 1000, 1000) c64  x, y  1000  smooth      axis    16  1024     138000         31313 (501000)
                          z     500   smooth      row     8   256      41008          125000

Every band of the class table -- (complex64 | complex128) x (smooth | not smooth) x tc (16 | 8 | 4) -- is reached on the x axis and
on the y axis, with at least 40 workgroups; no shape was left out for memory or time.  One pass has a line count that IS a multiple
of its tc: (1000, 1000, 24) complex128, 13000 lines at tc 8 (a shape the grid set has to contain); its class is also run with ragged
last tiles by (1000, 12, 1000) / (12, 1000, 1000).  The LDS column is the launchers' formula; the trace backs tc and threads.
"""
import numpy as np
import pytest

import partial_dft
from conftest import golden
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

TOL_F32 = 1e-5          # * rms: the project's tolerances (tests/test_gpu_parity.py, BASELINE section 3)
TOL_F64 = 1e-11
SPACING = 0.5           # keeps the k range of every grid here (axes of 12 ... 4000 cells) inside the default power table

BIG = [(200, 300, 400), (250, 126, 1000),                            # smooth; and 126 = 2 3^2 7 on the y axis
       (1000, 1000, 24), (1000, 12, 1000), (12, 1000, 1000),         # the published 1000^3's own axis instantiations in each role
       (2 * 7 * 11, 8 * 5 * 7, 4 * 3 * 37)]                          # (154, 280, 444): large primes behind smooth stages, all three axes
BANDS = [(126, 250, 40),                                             # not smooth, tc 16, on the x axis
         (1200, 30, 40), (30, 1200, 40),                             # smooth: complex64 tc 8, complex128 tc 4
         (2400, 30, 40), (30, 2400, 40),                             # smooth: complex64 tc 4, complex128 four-step by preference
         (350, 30, 40), (30, 350, 40),                               # 2 5^2 7: complex64 tc 16 / 1024 threads, complex128 tc 8
         (700, 30, 40), (30, 700, 40),                               # 4 5^2 7: complex64 tc 8, complex128 tc 4
         (1400, 30, 40), (30, 1400, 40)]                             # 8 5^2 7: complex64 tc 4, complex128 four-step by preference
FOUR_STEP = [(4000, 40, 24), (2000, 40, 24), (40, 4000, 24)]         # just past "prefers four-step": steps 1 / 3 with 520 parent lines x 50 / 80 sub-lines
SHAPES = BIG + BANDS + FOUR_STEP
DTYPES = [(np.complex64, TOL_F32, 5e-7), (np.complex128, TOL_F64, 1e-14)]


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


@pytest.fixture(scope="module")
def dpower():
    d = golden("default_power.npz")
    return d["k"], d["Pk"]


def make_plan(hip, shape, dtype, k, Pk, spacing=SPACING):
    from randomfield_amd import powertools
    nx, ny, nz = shape
    plan = hip.DevicePlan(nx, ny, nz, dtype)
    plan.set_kgrid(*powertools.ksq_axes(nx, ny, nz, spacing))
    xt, st = cpu_ref.sigma_table(k, Pk, nx, ny, nz, spacing)
    plan.set_power(xt, st)
    return plan


def _tag(dtype):
    return "c64" if dtype == np.complex64 else "c128"


@pytest.mark.parametrize("dtype,tol,ktol", DTYPES, ids=["c64", "c128"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_same_noise_field_against_oracle(hip, dpower, shape, dtype, tol, ktol):
    """The whole field, its moments, the materialised k space, its Hermitian planes and the forward transform back to it, against
    the oracle's float64 transform of the same deviates."""
    nx, ny, nz = shape
    assert nz % 4 == 0 and nx * ny * nz <= 35e6
    k, Pk = dpower
    noise = cpu_ref.reference_noise(11, nx * ny * (nz // 2 + 1))
    ref, rms = cpu_ref.generate_delta_field(nx, ny, nz, SPACING, k, Pk, noise=noise, dtype=dtype, double_fft=True)
    rms = float(rms)
    plan = make_plan(hip, shape, dtype, k, Pk)
    try:
        assert not plan.tiled
        plan.realise(noise=noise)
        d = plan.download_real()
        err = float(np.max(np.abs(d - ref))) / rms
        mean, std = plan.moments()
        print("%s %s field err %.3g * rms, |std - rms| %.3g * rms" % (shape, _tag(dtype), err, abs(std - rms) / rms))
        assert d.shape == shape and err <= tol
        assert abs(std - rms) <= tol * rms and abs(mean - float(np.mean(ref, dtype=np.float64))) <= tol * rms
        del d, ref
        ks = plan.download_k()                                   # the generic path materialises k space
        kref = cpu_ref.generate_kspace(nx, ny, nz, SPACING, k, Pk, noise=noise, dtype=dtype)
        kmax = float(np.max(np.abs(kref)))
        kerr = float(np.max(np.abs(ks - kref))) / kmax
        print("%s %s k-space err %.3g * max|K|" % (shape, _tag(dtype), kerr))
        assert kerr <= ktol
        assert cpu_ref.is_hermitian_packed(ks, rtol=0, atol=0)
        del ks
        plan.execute_r2c()                                       # forward transform of the field: back to the same k space
        back = plan.download_k()
        berr = float(np.max(np.abs(back - kref))) / kmax
        print("%s %s r2c err %.3g * max|K|" % (shape, _tag(dtype), berr))
        assert berr <= 20 * tol
    finally:
        plan.close()


NATIVE = [((200, 300, 400), np.complex64), ((200, 300, 400), np.complex128), ((250, 126, 1000), np.complex64),
          ((1000, 12, 1000), np.complex128), ((12, 1000, 1000), np.complex64), ((154, 280, 444), np.complex64),
          ((154, 280, 444), np.complex128), ((1200, 30, 40), np.complex64), ((30, 700, 40), np.complex128),
          ((4000, 40, 24), np.complex64), ((2000, 40, 24), np.complex128)]


@pytest.mark.parametrize("shape,dtype", NATIVE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else _tag(v))
def test_native_generation_value_by_value(hip, dpower, shape, dtype):
    """Native (Philox) generation on generic grids against the oracle's restatement of the same counter-based stream: the default
    fast flavour (float32 hardware log / sin / cos) at 1e-5 * rms, the exact-chain flavour at the dtype's tolerance; the fused
    call equals generate + execute_c2r bit for bit, and so does the last realisation of a batch."""
    nx, ny, nz = shape
    k, Pk = dpower
    seed = 31337
    tol = TOL_F32 if dtype == np.complex64 else TOL_F64
    noise = cpu_ref.native_noise(seed, nx, ny, nz, dtype)
    ref, rms = cpu_ref.generate_delta_field(nx, ny, nz, SPACING, k, Pk, noise=noise, dtype=dtype, double_fft=True)
    del noise
    rms = float(rms)
    plan = make_plan(hip, shape, dtype, k, Pk)
    try:
        plan.realise(seed=seed)
        d = plan.download_real()
        mean, std = plan.moments()
        err = float(np.max(np.abs(d - ref))) / rms
        print("%s %s native fast err %.3g * rms, |std - rms| %.3g * rms" % (shape, _tag(dtype), err, abs(std - rms) / rms))
        assert err <= 1e-5
        assert abs(std - rms) <= 1e-5 * rms
        plan.generate(seed=seed)
        plan.execute_c2r()
        assert np.array_equal(plan.download_real(), d) and plan.moments() == (mean, std)
        rms_b = plan.realise_batch([1, 2, seed])
        assert rms_b[2] == std and np.array_equal(plan.download_real(), d)
        assert rms_b[0] != rms_b[1] and rms_b[1] != rms_b[2]
        del d
        plan.set_exact_generation(True)
        plan.realise(seed=seed)
        e = plan.download_real()
        xerr = float(np.max(np.abs(e - ref))) / rms
        print("%s %s native exact err %.3g * rms" % (shape, _tag(dtype), xerr))
        assert xerr <= tol
        assert abs(plan.moments()[1] - rms) <= tol * rms
    finally:
        plan.close()


@pytest.mark.parametrize("ct,tol", [(np.complex64, 2e-6), (np.complex128, 1e-14)], ids=["c64", "c128"])
@pytest.mark.parametrize("shape", [(200, 300, 400), (12, 1000, 1000), (154, 280, 444), (12, 10, 7000), (12, 10, 3500)],
                         ids=lambda s: "x".join(map(str, s)))
def test_unpacked_c2c_against_numpy(hip, shape, ct, tol):
    """transform.Plan(packed=False) forward and inverse against numpy in complex128.  The contiguous axis of these plans runs
    generic_axis_block with inner = 1 -- lines that are not neighbours in memory, four to a workgroup -- a launch the packed plans
    never make.  7000 = 8 5^3 7 (complex64) and 3500 (complex128) are contiguous lines that are not smooth and whose two buffers
    leave no room for the stage table: strided_shape's one-line fallback with the twiddles read from global memory (tw_lds = 0),
    which only such an axis reaches -- a strided axis of that length takes the four-step form."""
    from randomfield_amd.transform import Plan
    rng = np.random.RandomState(23)
    src = (rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(ct)
    for inverse, fn in ((True, np.fft.ifftn), (False, np.fft.fftn)):
        c = Plan(shape=shape, dtype_in=ct, packed=False, inverse=inverse)
        try:
            assert c.backend == "hip" and not c.device.tiled
            c.data_in[:] = src
            ref = fn(src.astype(np.complex128))
            err = float(np.max(np.abs(c.execute() - ref))) / float(np.abs(ref).std())
            print("%s %s c2c inverse=%s err %.3g * std" % (shape, _tag(ct), inverse, err))
            assert err <= 20 * tol
            del ref
        finally:
            c.device.close()


def test_published_size_1000_cubed_float32(hip, dpower):
    """bench.py --full publishes a 1000^3 float32 time on this path; a float64 oracle of 10^9 cells is out of reach, so the field
    is pinned from its own k space, which the generic path materialises: tests/partial_dft.py gives exact single lines of
    irfftn(K).  Every output depends on every input cell, so a wrong tile of the x or y pass shows on every sampled line; the z
    pass's own rows are covered by the Parseval sum and by the M = 500 shapes above."""
    n = 1000
    shape = (n, n, n)
    k, Pk = dpower
    seed = 2024
    plan = make_plan(hip, shape, np.complex64, k, Pk)
    try:
        assert not plan.tiled
        plan.realise(seed=seed)
        mean, std = plan.moments()
        K = plan.download_k()
        planes = np.ascontiguousarray(K[:, :, [0, 1, n // 2]])           # a packed array of nz = 4: its kz = 0 and nz / 2 planes are K's own
        assert cpu_ref.is_hermitian_packed(planes, rtol=0, atol=0)
        del planes
        pmean, pstd = partial_dft.parseval_moments(K)
        print("1000^3: std %.9g, Parseval %.9g (%.3g * rms), mean %.3g * rms" % (std, pstd, abs(std - pstd) / pstd, abs(mean) / pstd))
        assert abs(std - pstd) <= TOL_F32 * pstd and abs(mean) < 1e-6 * pstd
        rms = pstd
        # first, last and an interior index that is no multiple of 16, in every direction
        zl = [(0, 0), (n - 1, n - 1), (501, 333)]                        # along z at (x0, y0)
        yl = [(0, 0), (n - 1, n - 1), (501, 333)]                        # along y at (x0, z0)
        xl = [(0, 0), (n - 1, n - 1), (333, 501)]                        # along x at (y0, z0)
        wz, wy, wx = partial_dft.field_lines(K, zl, yl, xl)
        del K
        gx = [np.empty(n, np.float32) for _ in xl]
        slab = {}
        step = 50
        for a in range(0, n, step):
            s = plan.download_real(x0=a, x1=a + step)
            for j, (y0, z0) in enumerate(xl):
                gx[j][a:a + step] = s[:, y0, z0]
            for x0 in (0, n - 1, 501):
                if a <= x0 < a + step:
                    slab[x0] = s[x0 - a].copy()
        for (x0, y0), want in zip(zl, wz):
            err = float(np.max(np.abs(slab[x0][y0, :] - want))) / rms
            print("1000^3 line along z at (%d, %d): %.3g * rms" % (x0, y0, err))
            assert err <= TOL_F32
        for (x0, z0), want in zip(yl, wy):
            err = float(np.max(np.abs(slab[x0][:, z0] - want))) / rms
            print("1000^3 line along y at (%d, %d): %.3g * rms" % (x0, z0, err))
            assert err <= TOL_F32
        for j, ((y0, z0), want) in enumerate(zip(xl, wx)):
            err = float(np.max(np.abs(gx[j] - want))) / rms
            print("1000^3 line along x at (%d, %d): %.3g * rms" % (y0, z0, err))
            assert err <= TOL_F32
        # the same seed again, and as the last of a batch: the same bits on a slab
        first = plan.download_real(x0=500, x1=502)
        plan.realise(seed=seed)
        assert np.array_equal(plan.download_real(x0=500, x1=502), first) and plan.moments() == (mean, std)
        rms_b = plan.realise_batch([7, 8, seed])
        assert rms_b[2] == std and np.array_equal(plan.download_real(x0=500, x1=502), first)
    finally:
        plan.close()
