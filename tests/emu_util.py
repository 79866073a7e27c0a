"""ctypes binding of the CPU kernel emulator (randomfield_amd/csrc/emu) -- test tooling."""
import ctypes
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "randomfield_amd", "csrc")
SO = os.path.join(CSRC, "emu", "librf_emu.so")

_c_dp = ctypes.POINTER(ctypes.c_double)


def _dp(a):
    return a.ctypes.data_as(_c_dp) if a is not None else None


def build(force=False):
    srcs = [os.path.join(CSRC, f) for f in ("emu/rf_emu.cpp", "rf_core.h", "rf_exp2_tab.h", "rf_fft.h", "rf_fft_col.h", "rf_fft_gen.h", "rf_fft_row.h",
                                            "rf_configs.h", "rf_select.h", "rf_host.h", "rf_generic.h")]
    if force or not os.path.exists(SO) or any(os.path.getmtime(s) > os.path.getmtime(SO) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-pthread", "-o", SO, srcs[0]])
    return SO


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = ctypes.CDLL(build())
    return _lib


def _gen_args(nx, ny, nz, spacing, log10k, sigma, seed, noise):
    from oracle import cpu_ref
    kx2, ky2, kz2 = (np.ascontiguousarray(a) for a in cpu_ref.ksq_axes(nx, ny, nz, spacing))
    log10k = np.ascontiguousarray(log10k, np.float64)
    sigma = np.ascontiguousarray(sigma, np.float64)
    mode = 0 if noise is None else 1
    if noise is not None:
        noise = np.ascontiguousarray(noise, np.float64)
    keep = (kx2, ky2, kz2, log10k, sigma, noise)
    args = (_dp(kx2), _dp(ky2), _dp(kz2), _dp(log10k), _dp(sigma), ctypes.c_int(len(log10k)),
            ctypes.c_int(mode), ctypes.c_uint64(seed or 0), _dp(noise))
    return args, keep


def generate_kspace(nx, ny, nz, spacing, log10k, sigma, seed=0, noise=None, dtype=np.complex64):
    args, keep = _gen_args(nx, ny, nz, spacing, log10k, sigma, seed, noise)
    out = np.empty((nx, ny, nz // 2 + 1), dtype)
    rc = lib().emu_generate_kspace(int(dtype == np.complex128), nx, ny, nz, *args, out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0
    return out


def realise(nx, ny, nz, spacing, log10k, sigma, seed=0, noise=None, dtype=np.complex64):
    args, keep = _gen_args(nx, ny, nz, spacing, log10k, sigma, seed, noise)
    rt = np.float32 if dtype == np.complex64 else np.float64
    out = np.empty((nx, ny, nz), rt)
    s1, s2 = ctypes.c_double(), ctypes.c_double()
    rc = lib().emu_realise(int(dtype == np.complex128), nx, ny, nz, *args, out.ctypes.data_as(ctypes.c_void_p),
                           ctypes.byref(s1), ctypes.byref(s2))
    assert rc == 0, rc
    return out, s1.value, s2.value


def c2r(kspace):
    nx, ny, nzh = kspace.shape
    nz = 2 * (nzh - 1)
    rt = np.float32 if kspace.dtype == np.complex64 else np.float64
    out = np.empty((nx, ny, nz), rt)
    s1, s2 = ctypes.c_double(), ctypes.c_double()
    ks = np.ascontiguousarray(kspace)
    rc = lib().emu_c2r(int(kspace.dtype == np.complex128), nx, ny, nz, ks.ctypes.data_as(ctypes.c_void_p),
                       out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(s1), ctypes.byref(s2))
    assert rc == 0, rc
    return out, s1.value, s2.value


def c2r_lognormal(kspace, growth, density=None):
    """rf_realise_lognormal behind its generation pass: (rho, sigma, sum, sum of squares) -- the accumulating y pass (AccColIO), the
    tables from its sigma, the map in the z pass's store (LognormalRowIO)"""
    nx, ny, nzh = kspace.shape
    nz = 2 * (nzh - 1)
    rt = np.float32 if kspace.dtype == np.complex64 else np.float64
    out = np.empty((nx, ny, nz), rt)
    sig, s1, s2 = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
    ks = np.ascontiguousarray(kspace)
    growth = np.ascontiguousarray(growth, np.float64)
    density = None if density is None else np.ascontiguousarray(density, np.float64)
    assert growth.shape == (nz,) and (density is None or density.shape == (nz,))
    rc = lib().emu_c2r_lognormal(int(kspace.dtype == np.complex128), nx, ny, nz, ks.ctypes.data_as(ctypes.c_void_p), _dp(growth), _dp(density),
                                 out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(sig), ctypes.byref(s1), ctypes.byref(s2))
    assert rc == 0, rc
    return out, sig.value, s1.value, s2.value


def c2r_zscale(kspace, factor_z):
    """c2r with plane z times factor_z[z] in the z pass's store (ScaleZRowIO): (field, sum, sum of squares)"""
    nx, ny, nzh = kspace.shape
    nz = 2 * (nzh - 1)
    rt = np.float32 if kspace.dtype == np.complex64 else np.float64
    out = np.empty((nx, ny, nz), rt)
    s1, s2 = ctypes.c_double(), ctypes.c_double()
    ks = np.ascontiguousarray(kspace)
    fz = np.ascontiguousarray(factor_z, np.float64)
    assert fz.shape == (nz,)
    rc = lib().emu_c2r_zscale(int(kspace.dtype == np.complex128), nx, ny, nz, ks.ctypes.data_as(ctypes.c_void_p), _dp(fz),
                              out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(s1), ctypes.byref(s2))
    assert rc == 0, rc
    return out, s1.value, s2.value


def exp_scaled64(t, stride=1):
    """exp_scaled64 (rf_fft_row.h) of arguments in units of ln2 / 64: stride 1 on rf_exp2_tab, 18 on the copy LognormalRowIO<double, 1>
    stages into the pad slots of its tile"""
    t = np.ascontiguousarray(t, np.float64)
    out = np.empty_like(t)
    f = lib().emu_exp_scaled64
    f.argtypes = [_c_dp, _c_dp, ctypes.c_longlong, ctypes.c_int]
    rc = f(_dp(t), _dp(out), t.size, int(stride))
    assert rc == 0, rc
    return out


def col_fft(data, N, direction, ncols, inner, outer_stride, row_stride):
    f = lib().emu_col_fft
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p] + [ctypes.c_longlong] * 4
    rc = f(int(data.dtype == np.complex128), N, direction, data.ctypes.data_as(ctypes.c_void_p), ncols, inner,
           outer_stride, row_stride)
    return rc


def realise_fast(nx, ny, nz, spacing, log10k, sigma, seed, dtype=np.float32):
    """Fused realisation with the fast native generation path (float32 arithmetic; a float64
    plan widens the generated values and transforms in double precision)."""
    args, keep = _gen_args(nx, ny, nz, spacing, log10k, sigma, seed, None)
    k0 = 2 * np.pi / spacing
    xlo = np.log10(k0 / max(nx, ny, nz)) - 0.01
    xhi = np.log10(k0 * np.sqrt(3) / 2) + 0.01
    out = np.empty((nx, ny, nz), dtype)
    s1, s2 = ctypes.c_double(), ctypes.c_double()
    rc = lib().emu_realise_fast(int(np.dtype(dtype) == np.float64), nx, ny, nz, *args[:6], ctypes.c_uint64(seed),
                                ctypes.c_double(xlo), ctypes.c_double(xhi), ctypes.c_double(k0 / nx),
                                out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(s1), ctypes.byref(s2))
    assert rc == 0, rc
    return out, s1.value, s2.value


def realise_fast_ex(nx, ny, nz, spacing, log10k, sigma, seed, dtype=np.float32, pot=0, pscale=1.0, noise64=None, noise32=None, first=None, cap=0,
                    x0=0, x1=1 << 30, kz0=0, nzl=-1, finish=True, field=None):
    """emu_realise_fast_ex: realise_fast with everything the launcher is told -- pot 0 / 1 (a potential array is returned) / 2 (the
    pass transforms pscale delta(k) / k^2); resident deviates as float64 (noise64, API layout) or as float32 pairs in the replay's
    runs (noise32 [nseg * cap][2], first: exclusive scan of the per-segment counts); rows [x0, x1); planes [kz0, kz0 + nzl).
    The ranks of a job are one call each on the same buffer: finish=False runs the x pass only and returns the buffer, which the
    next call takes as field=...; the last one runs the y and z passes too.  finish="loads": no transform -- the buffer receives
    the packed cells the pass loads, complex [nx][ny][nz / 2] (view it as the plan's complex dtype).  Returns (field, sum, sum of squares, potential of
    this call [nx][ny][nzl + 1] or None)."""
    args, keep = _gen_args(nx, ny, nz, spacing, log10k, sigma, seed, None)
    k0 = 2 * np.pi / spacing
    xlo = np.log10(k0 / max(nx, ny, nz)) - 0.01
    xhi = np.log10(k0 * np.sqrt(3) / 2) + 0.01
    f64 = int(np.dtype(dtype) == np.float64)
    out = np.zeros((nx, ny, nz), dtype) if field is None else field
    assert out.shape == (nx, ny, nz) and out.dtype == np.dtype(dtype) and out.flags.c_contiguous
    nl = nz // 2 if nzl < 0 else nzl
    ppitch = nl + 1 if f64 else nl + (64 if nl >= 256 else 2)
    P = np.zeros((nx, ny, ppitch), np.complex128 if f64 else np.complex64) if pot == 1 else None
    src = 0
    if noise64 is not None:
        src, noise64 = 1, np.ascontiguousarray(noise64, np.float64)
        assert noise64.size == 2 * nx * ny * (nz // 2 + 1)
    nseg = 0
    if noise32 is not None:
        src, noise32, first = 2, np.ascontiguousarray(noise32, np.float32), np.ascontiguousarray(first, np.uint64)
        nseg = len(first) - 1
        assert noise32.size == 2 * nseg * cap
    s1, s2 = ctypes.c_double(), ctypes.c_double()
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p) if a is not None else None
    rc = lib().emu_realise_fast_ex(f64, nx, ny, nz, *args[:6], ctypes.c_uint64(seed), ctypes.c_double(xlo), ctypes.c_double(xhi),
                                   ctypes.c_double(k0 / nx), int(pot), ctypes.c_double(pscale), src, _dp(noise64), vp(noise32), vp(first), nseg,
                                   ctypes.c_ulonglong(cap), int(x0), int(x1), int(kz0), int(nzl), 2 if finish == "loads" else int(bool(finish)), vp(out), vp(P),
                                   ctypes.byref(s1), ctypes.byref(s2))
    assert rc == 0, rc
    return out, s1.value, s2.value, (P[:, :, :nl + 1] if P is not None else None)


def fastgen_variant(f64, N, emit=False, n64=False, n32=False, pot=False, slab=False):
    """rf_select.h fastgen_variant: (slab, pot, src, halves), None where it is invalid"""
    out = (ctypes.c_int * 5)()
    valid = lib().emu_fastgen_variant(int(f64), N, int(emit), int(n64), int(n32), int(pot), int(slab), out)
    return (out[1], out[2], out[3], bool(out[4])) if valid else None


def col_replicate_supported(f64, N, nranks):
    return bool(lib().emu_col_replicate_supported(int(f64), N, nranks))


def fastgen_sequence_ex(nx, ny, nz, f64=False, emit=False, n64=False, n32=False, pot=False, x0=0, x1=1 << 30, kz0=0, nzl=-1):
    """rf_select.h fastgen_sequence for the variant the flags select, rows [x0, x1) and planes [kz0, kz0 + nzl); None where the
    library refuses"""
    buf = (ctypes.c_longlong * 40)()
    n = lib().emu_fastgen_sequence_ex(int(f64), nx, ny, nz, int(emit), int(n64), int(n32), int(pot), int(x0), int(x1), int(kz0), int(nzl), buf, 8)
    if n < 0:
        return None
    return [tuple(buf[5 * i:5 * i + 5]) for i in range(n)]


def _steps(call):
    buf = (ctypes.c_longlong * 40)()
    n = call(buf, 8)
    assert 0 <= n <= 8, n
    return [tuple(buf[5 * i:5 * i + 5]) for i in range(n)]


def fast_steps():
    """The launches the last realise_fast ran for its x pass: (kind, io, count, mul, skip_period) per step (rf_select.h FastStep)."""
    return _steps(lib().emu_fast_steps)


def fastgen_sequence(nx, ny, nz, f64=False):
    """rf_select.h fastgen_sequence for the x pass of that grid, called directly (honours emu_set_xposed / emu_set_pairs)."""
    return _steps(lambda buf, n: lib().emu_fastgen_sequence(int(f64), nx, ny, nz, buf, n))


def fast_visits():
    """How often the last realise_fast transformed each tile of its x pass."""
    f = lib().emu_fast_visits
    f.restype = ctypes.c_longlong
    out = np.zeros(1 << 16, np.int32)
    n = f(out.ctypes.data_as(ctypes.c_void_p), ctypes.c_longlong(out.size))
    assert 0 <= n <= out.size, n
    return out[:n]


def c2c(data, inverse):
    """Unpacked complex-to-complex transform through the emulated kernels (returns a new array)."""
    out = np.ascontiguousarray(data).copy()
    nx, ny, nz = out.shape
    rc = lib().emu_c2c(int(out.dtype == np.complex128), nx, ny, nz, 1 if inverse else -1,
                       out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, rc
    return out


def r2c(field):
    nx, ny, nz = field.shape
    ct = np.complex64 if field.dtype == np.float32 else np.complex128
    out = np.empty((nx, ny, nz // 2 + 1), ct)
    f = np.ascontiguousarray(field)
    rc = lib().emu_r2c(int(ct == np.complex128), nx, ny, nz, f.ctypes.data_as(ctypes.c_void_p),
                       out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, rc
    return out


def fast_sigma(log10k, sigma, xlo, xhi, k2):
    """fast float32 sigma lookup and the exact float64 interpolation for an array of |k|^2 values; also the number
    of per-bin records the fast table needed"""
    log10k = np.ascontiguousarray(log10k, np.float64)
    sigma = np.ascontiguousarray(sigma, np.float64)
    k2 = np.ascontiguousarray(k2, np.float32)
    fast = np.empty(k2.size, np.float32)
    exact = np.empty(k2.size, np.float64)
    f = lib().emu_fast_sigma
    f.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_void_p,
                  ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p]
    nb = f(log10k.ctypes.data, sigma.ctypes.data, len(log10k), xlo, xhi, k2.ctypes.data, k2.size, fast.ctypes.data,
           exact.ctypes.data)
    assert nb > 0, nb
    return fast, exact, nb


# ---- the generic (non-power-of-two) kernels of csrc/rf_generic.h ----------------------------------
def generic_c2r(kspace):
    nx, ny, nzh = kspace.shape
    nz = 2 * (nzh - 1)
    rt = np.float32 if kspace.dtype == np.complex64 else np.float64
    out = np.empty((nx, ny, nz), rt)
    s1, s2 = ctypes.c_double(), ctypes.c_double()
    ks = np.ascontiguousarray(kspace)
    rc = lib().emu_generic_c2r(int(kspace.dtype == np.complex128), nx, ny, nz, ks.ctypes.data_as(ctypes.c_void_p),
                               out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(s1), ctypes.byref(s2))
    assert rc == 0, rc
    return out, s1.value, s2.value


def generic_r2c(field):
    nx, ny, nz = field.shape
    ct = np.complex64 if field.dtype == np.float32 else np.complex128
    out = np.empty((nx, ny, nz // 2 + 1), ct)
    f = np.ascontiguousarray(field)
    rc = lib().emu_generic_r2c(int(ct == np.complex128), nx, ny, nz, f.ctypes.data_as(ctypes.c_void_p),
                               out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, rc
    return out


def generic_c2c(data, inverse):
    out = np.ascontiguousarray(data).copy()
    nx, ny, nz = out.shape
    rc = lib().emu_generic_c2c(int(out.dtype == np.complex128), nx, ny, nz, 1 if inverse else -1,
                               out.ctypes.data_as(ctypes.c_void_p))
    assert rc == 0, rc
    return out


def _form(v):
    """32 ints of emu_form_out -> {"n1", "n2", "lines"}: lines = ({"n", "radices", "smooth", "tables_fit"}, ...), one for an axis that
    is one line, two (n1 then n2) for the four-step form"""
    def line(o):
        radices = tuple(v[o + 3:o + 3 + v[o]])
        return {"n": int(np.prod(radices, dtype=np.int64)), "radices": radices, "smooth": bool(v[o + 1]), "tables_fit": bool(v[o + 2])}
    lines = (line(2), line(17)) if v[0] else (line(2),)
    assert not v[0] or (lines[0]["n"], lines[1]["n"]) == (v[0], v[1])
    return {"n1": v[0], "n2": v[1], "lines": lines}


def generic_axis_form(dtype, n, strided):
    """The form the library runs an axis of length n in (rf_generic.h generic_axis_form; strided: an x or y axis) under the emulator's
    cap and prefer-split switch, whose defaults are the library's; None where the axis is not served."""
    out = (ctypes.c_int * 32)()
    if not lib().emu_generic_axis_form(int(dtype == np.complex128), ctypes.c_longlong(n), int(bool(strided)), out):
        return None
    form = _form(list(out))
    assert np.prod([l["n"] for l in form["lines"]], dtype=np.int64) == n
    return form


def generic_shape_form(dtype, shape, packed):
    """generic_axis_form of the three axes of a packed (z at nz / 2) or c2c plan: (x, y, z); None where the shape is refused"""
    out = (ctypes.c_int * 96)()
    if not lib().emu_generic_shape_form(int(dtype == np.complex128), *map(int, shape), int(bool(packed)), out):
        return None
    return tuple(_form(list(out[32 * i:32 * i + 32])) for i in range(3))


class generic_prefer_split:
    """Context manager: emu_set_generic_prefer_split -- True (the default) is the library's rule, False the one-line form of every axis
    that fits the cap."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = lib().emu_set_generic_prefer_split(int(bool(self.on)))
        return self

    def __exit__(self, *exc):
        lib().emu_set_generic_prefer_split(self.old)
        return False


class generic_threads:
    """Context manager: the generic block functions on `nth` host threads with a real barrier (emu_set_generic_threads) and `tile`
    lines per block (emu_set_generic_tile); nth a multiple of the tile is the kernels' own thread walk."""

    def __init__(self, nth, tile):
        self.nth, self.tile = nth, tile

    def __enter__(self):
        self.old = (lib().emu_set_generic_threads(self.nth), lib().emu_set_generic_tile(self.tile))
        return self

    def __exit__(self, *exc):
        lib().emu_set_generic_threads(self.old[0])
        lib().emu_set_generic_tile(self.old[1])
        return False
