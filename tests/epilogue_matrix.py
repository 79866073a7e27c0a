"""Shared by tests/test_gpu_epilogue_matrix.py and tests/test_emulator_epilogue_matrix.py: the two z-pass IOs that do arithmetic in their
store -- LognormalRowIO (rf_realise_lognormal) and ScaleZRowIO (rf_realise_scaled_potential(factor_z)), rf_fft_row.h -- at every row
length, and the accumulating y pass that produces sigma for the first (AccColIO, rf_fft_col.h) at every column length in both
tile-addressing regimes.  Shapes and dtypes are tests/axis_matrix.py's (PACKED_NZ, COL_LENGTHS, DTYPES and its guards):

    z cases    (8, 8, nz), (32, 16, nz)      nz in PACKED_NZ: rows of M = nz/2 = 8 ... 1024; 64 rows (part of a workgroup) and 512
    y cases    (8, ny, 16), (8, ny, 128)     ny in COL_LENGTHS: a tile covers several kz runs / lies inside one (axis_matrix.guard)

The lognormal tables sweep the argument of exp.  From the plain field delta of the same input and its float64 std sigma0:
s_z = sqrt(log t_z) log-spaced over 1e-3 ... s_max, permuted with a fixed seed, the largest on the plane that holds max |delta|, and
s_max such that the reference's largest |argument| is TARGET: 40 on float32 plans (MomAcc<float> sums rho^2 in float32 and
e^80 * 32 < FLT_MAX), 60 on float64 plans.  growth_z = sqrt(exp(s_z^2) - 1) / sigma0 and density_z = sqrt(1 + (sigma0 growth_z)^2),
so B_z = density_z / sqrt(t_z) ~ 1 and rho = exp(argument) is a normal number of the dtype.  The run without a density table has
B_z = exp(-s_z^2 / 2): with max |delta| >= 3 sigma0 (1024 cells and more), TARGET_NO_DENSITY = 12 keeps s_max <= 4 and
rho >= e^-20, normal in both dtypes, while |argument| still goes well past the 7 the smooth growth tables of the other tests reach.

Reference: np.longdouble, with the sigma the call returned -- t_z = (sigma growth_z)^2 + 1 formed in float64 as the reference
program forms it, rho = exp(delta sqrt(log t_z) / sigma) density_z / sqrt(t_z) with delta the downloaded field of the plain call.

Per-cell relative bound, x the argument, s_z = sqrt(log t_z), eps of the plan's real dtype:

    float64    1e-13 + 8 eps (1 + |x|) + 1e-14 s_z         float32    4 eps (1 + |x|) + 3.3e-6 s_z

1e-13 is 2.5 x the documented truncation of exp_scaled64's polynomial; the eps terms are the roundings of the argument and of the
two table factors; the s_z term is the transform's own error in delta, in rms units, carried through the map -- 3 x the worst c2r
figure the axis matrix recorded on the GPU (1.11e-6 float32, 3.1e-15 float64: CHANGES.md, "value tests at every axis length").
sigma against the float64 std of delta: 1e-13 (float64); 1e-6 and equal to its own float32 rounding (float32).  The moments of rho
against float64 sums of the downloaded rho, mean and mean square each relatively (sums of positive terms): 2e-6 / 1e-12.

Per-z factor: f_z of both signs, magnitudes log-spaced over 1e-3 ... 1e3, permuted, all different; reference longdouble(plain field)
f_z; per cell eps/2 |ref| + c rms(plain) |f_z| with c = 1e-6 / 1e-13 (what test_regenerated_potential_equals_stored_one allows
between two instantiations of the z pass); moments relative to sum |rho| and sum rho^2, 2e-6 / 1e-12.

Regime guards, plain asserts: the reference's max |argument| >= 0.95 TARGET, every reference output finite and >= finfo.tiny, every
cell in every comparison.  Measured / bound of every check is printed and the worst per IO and dtype kept in WORST; CHANGES.md
("Fused lognormal and per-z epilogues") has the figures of the emulator and the GPU side by side."""
import os
import re

import numpy as np

import axis_matrix as am

C64, C128 = am.C64, am.C128
TARGET = {C64: 40.0, C128: 60.0}
TARGET_NO_DENSITY = 12.0
S_MIN = 1e-3
EPS_TERM = {C64: 4.0, C128: 8.0}               # x eps (1 + |x|)
FFT_TERM = {C64: 3.3e-6, C128: 1e-14}          # x s_z: 3 x (1.11e-6, 3.1e-15)
TRUNCATION = {C64: 0.0, C128: 1e-13}           # exp_scaled64's polynomial: 2.5 x 4e-14
SIGMA_TOL = {C64: 1e-6, C128: 1e-13}
MOMENT_TOL = {C64: 2e-6, C128: 1e-12}
ZSCALE_C = {C64: 1e-6, C128: 1e-13}

Z_CASES = [("z", nz) for nz in am.PACKED_NZ]
Y_CASES = [("y", ny) for ny in am.COL_LENGTHS]
CASES = Z_CASES + Y_CASES
NO_DENSITY_CASE = ("z", 1024)                  # the run without a density table: the short companion of this case, both dtypes

WORST = {}           # (check, dtype name) -> (largest measured / bound seen, where)

case_id = am.case_id
dtype_name = am.dtype_name
real_of = am.real_of


def plans(axis, n):
    """(shape, dtype) of one case: both companions in both dtypes, through axis_matrix's regime guards"""
    return am.plans(axis, n, packed=True)


def header_sizes(macro):
    """the lengths a size list of rf_configs.h names: RF_ROW_SIZES (rows of M complex) or RF_COL_SIZES"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "randomfield_amd", "csrc", "rf_configs.h")
    with open(path) as f:
        line = re.search(r"^#define %s\(X\)(.*)$" % macro, f.read(), re.M).group(1)
    sizes = tuple(int(v) for v in re.findall(r"X\((\d+)\)", line))
    assert sizes and re.sub(r"X\(\d+\)|\s", "", line) == "", line
    return sizes


def coverage_guard(cases):
    """the parameter list visits every (dtype, M) of RF_ROW_SIZES -- both z IOs run on every z case -- and every (dtype, N) of
    RF_COL_SIZES in both tile-addressing regimes of the accumulating y pass"""
    rows, cols = header_sizes("RF_ROW_SIZES"), header_sizes("RF_COL_SIZES")
    seen_rows, inside, several = set(), set(), set()
    for axis, n in cases:
        for shape, dtype in plans(axis, n):
            inner = shape[2] // 2
            if axis == "z":
                seen_rows.add((dtype, inner))
            else:
                (inside if inner >= am.TILE_COLS[dtype][n] else several).add((dtype, n))
    for dtype in am.DTYPES:
        # every row length, with 64 rows and with 512
        assert {m for d, m in seen_rows if d == dtype} == set(rows), (dtype_name(dtype), "row lengths", sorted(m for d, m in seen_rows if d == dtype))
        for axis, n in cases:
            if axis == "z":
                assert {s[0] * s[1] for s, d in plans(axis, n) if d == dtype} == {64, 512}
        assert {n for d, n in inside if d == dtype} == set(cols), (dtype_name(dtype), "column lengths, tile inside one run")
        # (the tiles of the longest passes are 8 or 4 columns wide: no tiled shape has a narrower run -- axis_matrix.SHORT_REGIME)
        assert {n for d, n in several if d == dtype} == set(am.SHORT_REGIME[dtype]), (dtype_name(dtype), "column lengths, tile over several runs")
        assert set(am.SHORT_REGIME[dtype]) == {n for n in cols if am.TILE_COLS[dtype][n] > 8}


def _record(check, dtype, ratio, where):
    key = (check, dtype_name(dtype))
    if key not in WORST or not ratio <= WORST[key][0]:
        WORST[key] = (ratio, where)


def _report(check, dtype, shape, ratio, what="measured / bound"):
    print("%s %s %s: %s = %.3g" % (check, shape, dtype_name(dtype), what, ratio))
    _record(check, dtype, ratio, shape)


# ---- lognormal --------------------------------------------------------------------------------------------------------------------
def sweep_tables(delta, dtype, seed, with_density=True):
    """(growth_z, density_z or None) from the plain field: see the module docstring"""
    d = delta.astype(np.float64)
    nz = d.shape[2]
    sigma0 = float(d.std())
    amax = np.abs(d).max(axis=(0, 1))
    top = int(np.argmax(amax))
    target = TARGET[dtype] if with_density else TARGET_NO_DENSITY
    s = np.random.RandomState(seed).permutation(np.geomspace(S_MIN, target * sigma0 / amax[top], nz))
    i = int(np.argmax(s))
    s[i], s[top] = s[top], s[i]
    growth = np.sqrt(np.expm1(s * s)) / sigma0
    return growth, (np.sqrt(1.0 + (sigma0 * growth) ** 2) if with_density else None)


def lognormal_reference(delta, sigma, growth, density):
    """(rho, argument x, s_z) in np.longdouble from the plain field and the sigma the fused call returned"""
    g = np.float64(sigma) * np.asarray(growth, np.float64)
    t = (g * g + 1.0).astype(np.longdouble)                        # float64, as the reference program forms it
    s = np.sqrt(np.log(t))
    x = delta.astype(np.longdouble) * (s / np.longdouble(sigma))
    b = (np.longdouble(1) if density is None else np.asarray(density, np.float64).astype(np.longdouble)) / np.sqrt(t)
    return np.exp(x) * b, x, s


def check_lognormal(what, rho, sigma, mean, meansq, delta, growth, density, dtype, shape):
    """the fused call's field, sigma and moments against the longdouble map of the plain field"""
    rt = real_of(dtype)
    eps, tiny = float(np.finfo(rt).eps), float(np.finfo(rt).tiny)
    target = TARGET[dtype] if density is not None else TARGET_NO_DENSITY
    assert rho.shape == delta.shape == tuple(shape) and rho.dtype == rt and delta.dtype == rt, (what, shape, rho.shape, rho.dtype)
    # sigma: the Parseval sum of the accumulating y pass against the std of the plain field
    std = float(delta.astype(np.float64).std())
    _report(what + " sigma", dtype, shape, abs(sigma - std) / (SIGMA_TOL[dtype] * std))
    assert abs(sigma - std) <= SIGMA_TOL[dtype] * std, "%s %s %s: sigma %.17g, std of the plain field %.17g" % (what, shape, dtype_name(dtype), sigma, std)
    if dtype == C64:
        assert sigma == float(np.float32(sigma))                   # np.std of float32 data is a float32
    ref, x, s = lognormal_reference(delta, sigma, growth, density)
    # regime guards
    xmax = float(np.max(np.abs(x)))
    assert 0.95 * target <= xmax <= 1.05 * target, (what, shape, "largest |argument| %.3g, target %g" % (xmax, target))
    assert np.all(np.isfinite(ref)) and float(ref.min()) >= tiny and float(ref.max()) <= float(np.finfo(rt).max)
    assert np.all(np.isfinite(rho)) and np.all(rho > 0), (what, shape, "a cell is not a positive finite number")
    bound = TRUNCATION[dtype] + EPS_TERM[dtype] * eps * (1 + np.abs(x)) + FFT_TERM[dtype] * s
    ratio = np.abs(rho.astype(np.longdouble) - ref) / ref / bound
    assert ratio.shape == tuple(shape) and ratio.size == int(np.prod(shape))          # no cell is left out
    worst = float(ratio.max())
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    _report(what, dtype, shape, worst)
    assert worst <= 1.0, "%s %s %s: cell %s (argument %.4g, s_z %.3g) is off by %.3g x its bound" % (
        what, shape, dtype_name(dtype), at, float(x[at]), float(s[at[2]]), worst)
    # moments of rho against float64 sums of the downloaded rho: mean and mean square, each relatively
    r64 = rho.astype(np.float64)
    m1, m2 = float(r64.mean()), float(np.mean(r64 * r64))
    e1, e2 = abs(mean - m1) / m1 / MOMENT_TOL[dtype], abs(meansq - m2) / m2 / MOMENT_TOL[dtype]
    _report(what + " moments", dtype, shape, max(e1, e2))
    assert e1 <= 1.0 and e2 <= 1.0, "%s moments %s %s: mean off by %.3g x its bound, mean square by %.3g x" % (what, shape, dtype_name(dtype), e1, e2)


# ---- per-z factor -----------------------------------------------------------------------------------------------------------------
def factor_z(nz, seed):
    """nz factors of both signs, magnitudes log-spaced over 1e-3 ... 1e3, permuted, every entry different"""
    f = np.geomspace(1e-3, 1e3, nz) * np.where(np.arange(nz) % 2, -1.0, 1.0)
    f = np.random.RandomState(seed).permutation(f)
    assert len(set(f.tolist())) == nz and f.min() < 0 < f.max() and np.abs(f).min() <= 1.001e-3 and np.abs(f).max() >= 999.0
    return f


def check_zscale(what, got, mean, meansq, plain, fz, dtype, shape):
    """the field with the factor in the z pass's store against longdouble(plain field) f_z"""
    rt = real_of(dtype)
    eps = float(np.finfo(rt).eps)
    assert got.shape == plain.shape == tuple(shape) and got.dtype == rt and plain.dtype == rt, (what, shape, got.shape, got.dtype)
    rms = am.rms_of(plain.astype(np.float64))
    assert rms > 0 and np.all(np.isfinite(plain))
    f = np.asarray(fz, np.float64).astype(np.longdouble)
    ref = plain.astype(np.longdouble) * f
    bound = 0.5 * eps * np.abs(ref) + ZSCALE_C[dtype] * rms * np.abs(f)
    ratio = np.abs(got.astype(np.longdouble) - ref) / bound
    assert ratio.shape == tuple(shape) and ratio.size == int(np.prod(shape)) and np.all(np.isfinite(got))
    worst = float(ratio.max())
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    _report(what, dtype, shape, worst)
    assert worst <= 1.0, "%s %s %s: cell %s (factor %.4g) is off by %.3g x its bound" % (what, shape, dtype_name(dtype), at, float(fz[at[2]]), worst)
    g64 = got.astype(np.float64)
    n = g64.size
    e1 = abs(mean * n - float(g64.sum())) / float(np.abs(g64).sum()) / MOMENT_TOL[dtype]
    e2 = abs(meansq * n - float((g64 * g64).sum())) / float((g64 * g64).sum()) / MOMENT_TOL[dtype]
    _report(what + " moments", dtype, shape, max(e1, e2))
    assert e1 <= 1.0 and e2 <= 1.0, "%s moments %s %s: sum off by %.3g x its bound, sum of squares by %.3g x" % (what, shape, dtype_name(dtype), e1, e2)
