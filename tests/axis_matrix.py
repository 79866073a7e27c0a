"""Shared by tests/test_gpu_axis_matrix.py and tests/test_emulator_axis_matrix.py: the forward (r2c), c2r-from-k and c2c transforms at
every tiled axis length, one axis long and the others short -- the shape table, the regime guards, the inputs, the numpy float64
references and the bound.

Every (axis, length) has two companion shapes so that a column tile is addressed both ways (rf_fft.h ColGeom): with a small `inner`
(the contiguous run of columns: nz/2 of a packed plan, nz of a c2c plan, on the y pass) a tile of TC columns covers several runs and
the lane's column offset selects the run; with a larger one a tile lies inside one run.  On z the first companion has 64 rows -- fewer than one workgroup takes
where rows are short (RowCfg NRT up to 256) -- and the second 512: several workgroups at every row length.

    packed plans (r2c, c2r from k)      x = N: (N, 8, 16), (N, 8, 128)    y = N: (8, N, 16), (8, N, 128)    N in 8 ... 2048
                                        z: (8, 8, nz), (32, 16, nz)       nz in 16 ... 2048
    unpacked c2c plans                  x = N: (N, 8, 8), (N, 8, 64)      y = N: (8, N, 8), (8, N, 64)
                                        z: (8, 8, nz), (32, 16, nz)       nz in 8 ... 2048

Bound: max |got - ref| over ALL cells <= tol rms(ref), tol = 1e-5 (float32: the project's TOL_F32) and 3e-13 (float64:
test_forward_r2c_against_numpy's bound in rms units).  The references are numpy's transforms of the float64 cast of the input; the
phase functions on the CPU emulator reach 1.07e-6 (float32, raw c2r (1024, 8, 128)) and 3.1e-15 (float64) over this whole table and
the GPU 1.11e-6 and 3.1e-15 (CHANGES.md has the figures per transform), so the arithmetic alone stays 9x and 95x inside.  Every check
prints measured / bound and keeps the worst per transform and dtype in WORST."""
import numpy as np

from oracle import cpu_ref

C64, C128 = np.complex64, np.complex128
DTYPES = (C64, C128)
TOL = {C64: 1e-5, C128: 3e-13}

COL_LENGTHS = (8, 16, 32, 64, 128, 256, 512, 1024, 2048)           # rf_configs.h RF_COL_SIZES
PACKED_NZ = (16, 32, 64, 128, 256, 512, 1024, 2048)                # 2 x RF_ROW_SIZES
C2C_NZ = (8, 16, 32, 64, 128, 256, 512, 1024, 2048)                # RF_ROWC_SIZES

# tile widths in columns of the strided passes (rf_configs.h ColSel; float64 has TC32 / 2 except where noted)
TILE_COLS = {
    C64: {8: 32,       # RF_COL(8,    8,  1,  1, 32, 256)
          16: 32,      # RF_COL(16,   16, 1,  1, 32, 256)
          32: 32,      # RF_COL(32,   8,  4,  1, 32, 256)
          64: 32,      # RF_COL(64,   8,  8,  1, 32, 256)
          128: 32,     # RF_COL(128,  16, 8,  1, 32, 256)
          256: 16,     # RF_COL(256,  16, 16, 1, 16, 256)
          512: 16,     # RF_COL(512,  8,  8,  8, 16, 512)
          1024: 8,     # RF_COL32_1024 16, 8, 8, 8, 512
          2048: 8},    # RF_COL32_2048 8, 16, 16, 8, 1024
    C128: {8: 16,      # RF_COL(8, ...): 32 / 2
           16: 16,     # RF_COL(16, ...): 32 / 2
           32: 16,     # RF_COL(32, ...): 32 / 2
           64: 16,     # RF_COL(64, ...): 32 / 2
           128: 16,    # RF_COL(128, ...): 32 / 2
           256: 8,     # RF_COL(256, ...): 16 / 2
           512: 8,     # RF_COL(512, ...): 16 / 2
           1024: 8,    # RF_COL64_1024 16, 8, 8, 8, 1024 (not 8 / 2: whole 128-byte lines)
           2048: 4},   # ColCfg<double, 2048, 8, 16, 16, 4, 1024>
}
# y lengths at which the short companion (inner = 8) is narrower than a tile: the tile covers several runs there
SHORT_REGIME = {C64: (8, 16, 32, 64, 128, 256, 512), C128: (8, 16, 32, 64, 128)}

CASES = [("x", n) for n in COL_LENGTHS] + [("y", n) for n in COL_LENGTHS] + [("z", n) for n in C2C_NZ]

WORST = {}           # (transform, dtype name) -> (largest err / rms seen, where)


def case_id(v):
    return str(v)


def dtype_name(dtype):
    return "c64" if dtype == C64 else "c128"


def real_of(dtype):
    return np.float32 if dtype == C64 else np.float64


def packed_shapes(axis, n):
    """the two companion shapes of a packed plan, () where the length is no packed nz"""
    if axis == "x":
        return ((n, 8, 16), (n, 8, 128))
    if axis == "y":
        return ((8, n, 16), (8, n, 128))
    return ((8, 8, n), (32, 16, n)) if n in PACKED_NZ else ()


def c2c_shapes(axis, n):
    if axis == "x":
        return ((n, 8, 8), (n, 8, 64))
    if axis == "y":
        return ((8, n, 8), (8, n, 64))
    return ((8, 8, n), (32, 16, n))


def tiled(shape, dtype, packed):
    """rf_capi.hip shape_check / rf_plan_create_c2c: the tiled kernels take the shape (it is not generic)"""
    nx, ny, nz = shape
    inner = nz // 2 if packed else nz
    rows = tuple(m // 2 for m in PACKED_NZ) if packed else C2C_NZ
    if nx not in COL_LENGTHS or ny not in COL_LENGTHS or inner not in rows:
        return False
    return (ny * inner) % TILE_COLS[dtype][nx] == 0 and (nx * inner) % TILE_COLS[dtype][ny] == 0


def guard(axis, n, shapes, dtype, packed):
    """regime guards: a shape edited out of what it is in the table for fails here instead of passing for nothing"""
    short, long_ = shapes
    assert short["xyz".index(axis)] == n and long_["xyz".index(axis)] == n
    for shape in shapes:
        assert tiled(shape, dtype, packed), (shape, dtype_name(dtype), "is a generic shape")
    if axis == "y":
        tc = TILE_COLS[dtype][n]
        inner = [s[2] // 2 if packed else s[2] for s in shapes]
        if n in SHORT_REGIME[dtype]:
            assert inner[0] < tc, (short, "a tile no longer covers several runs of `inner` columns")
        # (float32 1024, 2048 and float64 256 ... 2048 have tiles of 8 or 4 columns: no tiled shape is narrower, both companions lie inside a run)
        assert inner[1] >= tc, (long_, "a tile no longer lies inside one run")
    if axis == "z":
        # rf_configs.h RF_ROW: a workgroup takes NRT rows, 256 (float32) / 128 (float64) at the shortest rows down to 1 at the longest
        assert short[0] * short[1] < 128       # a partly filled workgroup where NRT is largest
        assert long_[0] * long_[1] > 256       # several workgroups at every row length


def plans(axis, n, packed):
    """(shape, dtype) of one case, guarded: both companions in both dtypes"""
    shapes = packed_shapes(axis, n) if packed else c2c_shapes(axis, n)
    if not shapes:
        return []
    for dtype in DTYPES:
        guard(axis, n, shapes, dtype, packed)
    return [(shape, dtype) for shape in shapes for dtype in DTYPES]


# ---- inputs (seeded by the length) and references (numpy on the float64 cast of the input) ----
def real_field(shape, dtype, n):
    return np.ascontiguousarray(np.random.RandomState(n).normal(size=shape).astype(real_of(dtype)))


def complex_array(shape, dtype, n):
    rng = np.random.RandomState(n)
    return np.ascontiguousarray((rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(dtype))


def half_spectra(shape, dtype, n):
    """(symmetrised, raw) unit normal half spectra [nx][ny][nz/2 + 1]"""
    nx, ny, nz = shape
    raw = complex_array((nx, ny, nz // 2 + 1), dtype, n)
    return cpu_ref.symmetrize_packed(raw.copy()), raw


def rfftn(field):
    return np.fft.rfftn(field.astype(np.float64), axes=(0, 1, 2))


def irfftn(ks, shape):
    return np.fft.irfftn(ks.astype(C128), s=shape, axes=(0, 1, 2))


def fftn(a):
    return np.fft.fftn(a.astype(C128), axes=(0, 1, 2))


def ifftn(a):
    return np.fft.ifftn(a.astype(C128), axes=(0, 1, 2))


def rms_of(ref):
    return float(np.sqrt(np.mean(np.abs(ref) ** 2)))


def _record(transform, dtype, ratio, where):
    key = (transform, dtype_name(dtype))
    if key not in WORST or not ratio <= WORST[key][0]:
        WORST[key] = (ratio, where)


def check(transform, got, ref, dtype, shape):
    """max |got - ref| over all cells <= TOL rms(ref); returns that bound (absolute)"""
    want_dtype = real_of(dtype) if np.isrealobj(ref) else dtype
    assert got.shape == ref.shape and got.dtype == want_dtype, (transform, shape, got.shape, got.dtype)
    rms = rms_of(ref)
    err, bound = float(np.max(np.abs(got - ref))), TOL[dtype] * rms
    print("%s %s %s: err / rms = %.3e, measured / bound = %.3g" % (transform, shape, dtype_name(dtype), err / rms, err / bound))
    _record(transform, dtype, err / rms, shape)
    assert err <= bound, "%s %s %s: max error %.3e rms, bound %.1e rms" % (transform, shape, dtype_name(dtype), err / rms, TOL[dtype])
    return bound


def check_moments(transform, mean, std, ref, dtype, shape):
    """the (mean, std) the z pass's partials give against the reference's, each within TOL rms(ref)"""
    rms = rms_of(ref)
    bound = TOL[dtype] * rms
    em, es = abs(mean - float(ref.mean())), abs(std - float(ref.std()))
    print("%s moments %s %s: measured / bound = %.3g (mean), %.3g (std)" % (transform, shape, dtype_name(dtype), em / bound, es / bound))
    _record(transform + " moments", dtype, max(em, es) / rms, shape)
    assert em <= bound and es <= bound, "%s moments %s %s: mean off by %.3e rms, std by %.3e rms" % (transform, shape, dtype_name(dtype), em / rms, es / rms)


def check_hermitian(spec, bound, shape):
    assert cpu_ref.is_hermitian_packed(spec, rtol=0, atol=bound), "r2c %s: the planes kz = 0, nz/2 are not Hermitian" % (shape,)
