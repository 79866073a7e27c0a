"""Shared by tests/test_gpu_generation_matrix.py and tests/test_emulator_generation_matrix.py: the generation pass fused into the x
FFT -- every FastV<slab, pot, src, halves> of rf_select.h FastList32 / FastList64 at every length of RF_COL_SIZES, in every launch form of
fastgen_sequence, and the exact kernel behind them -- checked MODE BY MODE against cpu_ref's float64 stages.

Shapes (axis_matrix.COL_LENGTHS, both companions of the x cases, tile widths axis_matrix.TILE_COLS -- GenSel keeps ColSel's TC):

    (nx, 8, 16)      a kz row of 8 fits one tile at every length: one launch with the owning lane's repair (unsplit)
    (nx, 8, 128)     64 columns per ky row, more than one tile: FIRST + LEAN; behind FAST_FIX_FILL for nx >= 512; nx = 1024 float32 on
                     tile pairs, 4 pairs per row
    (1024, 8, 32)    float32 only: one pair per row, the FIRST launch covers everything

Variants per (shape, dtype) -- VARIANTS below has the flags each one hands to fastgen_variant:

    A  realise(seed)                            native, pot 0 (halves form at 2048 float32 / 1024 float64)
    B  realise_potential(seed)                  native, pot 1
    C  realise_scaled_potential(seed, scale)    native, pot 2 (halves form too)
    D  resident float64 deviates                complex64 only: src 1
    E  resident float32 pairs                   complex64 only: src 2 (short segments, mt_blocks: rows cut by a segment boundary)
    F  as E, realise_potential                  src 2, pot 1
    G  as E, realise_scaled_potential           src 2, pot 2
    H  exact-generation flag + realise(seed)    the exact kernel (also what float64 plans run at nx = 2048)
    I  realise(noise = host array)              complex128 only: the exact kernel on host deviates
    J  2 ranks, replicated generation           slab 1 (where col_replicate_supported: nx >= 32)
    K  2 kz-slab ranks, native                  (nx, 8, 128): rank 1 has kz0 != 0 -- no repair, LEAN only where it splits
    K' as K with the potential stored           pot 1 on both ranks

Oracle: kref = cpu_ref.generate_kspace(dtype = complex128) on cpu_ref.native_noise (A - C, H, J, K) or cpu_ref.reference_noise
(D - G, I); sigma_m from the same float64 table lookup, n_m = kref_m / sigma_m, k^2 from powertools.ksq_axes.  The fast pass forms its
deviates in float32 on float64 plans too (rf_fft_gen.h FastGenColIO64: BoxMuller<float>, widened), so the fast classes take the
float32 restatement of the native stream (native_noise(..., complex64)) on either plan type; the exact kernel of a complex128 plan
takes the float64 one.  (Against the float64 restatement the float32 stream differs in the tail u1 -> 1, where sqrt(-2 ln u1) loses
the bits that u1's rounding dropped: 6.7e-6 of one mode at (1024, 8, 128) on the emulator -- another definition of the deviate, not
an error of the pass.)

Primary check, every mode of the half spectrum:

    e_m = |got_m - kref_m| / (sigma_m (1 + |n_m|)) <= c[class][dtype]  (+ floor_m on the field route)

    potential route (B, F, K')    got = download_k() after load_potential(1.0), times k^2 in float64: the pass's own k-space values
    field route (A, D, E, H - K)  got = rfftn(float64(field)); floor_m = FFT_TERM sigma_rms / sigma_m, FFT_TERM epilogue_matrix's
                                  (3.3e-6 / 1e-14: 3 x the worst c2r error per cell in rms units), sigma_rms = sqrt(N) rms(field):
                                  white error of that size per cell is sqrt(N) times as much per mode
    C, G                          got = rfftn(float64(field)) k^2 / scale.  The transform's error is relative to the rms of the
                                  POTENTIAL field, whose spectrum is as red as 1 / k^2 makes it, and it is not white, so the
                                  window measures itself: the oracle's own potential spectrum through the backend's c2r of an
                                  uploaded half spectrum and back (window_error: no generation involved); floor_m =
                                  WINDOW_MARGIN = 3 x that worst per-mode error, as a white level, x k^2_m / sigma_m.  On float32
                                  plans this floor is below c on a few per cent of the modes of the smallest grids and on none
                                  from (16, 8, 128) up (every case prints the share): through the transform of a float32 field the
                                  pot = 2 kernels are pinned per mode at the lowest k only, beyond that by the field bound.  On
                                  float64 plans the floor is nothing and every mode is held to c.
    loads (emulator only)         emu_realise_fast_ex(finish = "loads"): the packed cells the variant's IO generates, the kz = 0 slot
                                  repaired, before any transform -- the per-mode window of EVERY single-rank fast variant without a
                                  transform's floor (check_loads), and the one that pins pot = 2 on float32 plans: floor <= c on
                                  more than 99 % of the modes of every case (the rest: the Nyquist plane's share of the packed
                                  kz = 0 slot, rounded once to float32 next to plane 0's).  The GPU has no such window: it never
                                  stores these cells.

`need` = max_m (e_m - floor_m) is what c would have to be for the case to pass: printed next to c for every case, the worst per class
and dtype kept in WORST.  c is 3 x the GPU's worst need of the class rounded up to one digit (CHANGES.md has the emulator's and the
GPU's figures side by side), and never more than its cap: 1e-5 for the fast classes (TOL_F32), 1e-11 for the exact kernel on
complex128 (TOL_F64), 1e-6 for it on complex64.

Structural checks on the potential route, exact: DC = 0; the eight self-conjugate modes are real; on the planes kz = 0 and nz/2 cell
(-ix, -iy) is the conjugate of (ix, iy) value for value (rf_core.h fast_fix_kz0 evaluates a destination cell at its source's
coordinates and flips the sign: no second rounding); modes with sigma_m = 0 are exactly zero on both sides.

Secondary: max |field - irfftn(kref)| <= FIELD_TOL rms; moments() -- of a multi-rank job: from its ranks' partial sums -- against the
float64 std of the downloaded field (MOMENT_TOL by plan dtype) and against the oracle's rms (by the arithmetic of the class); a
second identical call is bit-identical (field, moments, stored potential); K = A within 2e-6 rms."""
import numpy as np

import axis_matrix as am
import epilogue_matrix as em
from replay_matrix import stream_segments          # noqa: F401  (the oracle of the replayed stream lives with the replay's table)
from oracle import cpu_ref

C64, C128 = am.C64, am.C128
SPACING = 2.5
SCALE = -2.5e-3
MT_BLOCKS = 16                                   # segment length of the replayed stream: cap = 156 x 16 = 2496 attempts
FFT_TERM = em.FFT_TERM
MOMENT_TOL = em.MOMENT_TOL
K_VS_A = 2e-6                                    # the kz-slab field against the single-rank one, x rms
WINDOW_MARGIN = 3.0                              # x the scaled route's own measured error (window_error): another spectrum's tail

case_id = am.case_id
dtype_name = am.dtype_name
real_of = am.real_of

FAST_NATIVE, FAST_NOISE64, FAST_NOISE32, EXACT = "fast-native", "fast-noise64", "fast-noise32", "exact"
CAP = {FAST_NATIVE: {"c64": 1e-5, "c128": 1e-5}, FAST_NOISE64: {"c64": 1e-5}, FAST_NOISE32: {"c64": 1e-5},
       EXACT: {"c64": 1e-6, "c128": 1e-11}}
# 3 x the GPU's worst `need` of the class, one digit, rounded up (CHANGES.md, "Generation pass: per-mode value tests")
#   fast-native   c64  6.8e-7 (B (1024, 8, 128))     c128  1.32e-6 (J (1024, 8, 16))       fast-noise32  c64  1.13e-6 (F (2048, 8, 128))
#   exact         c128 6.7e-16 (B (2048, 8, 128): the one potential-route case of the class)
# Two classes have field-route cases only, whose floor covers them on the GPU and on the emulator (need <= 0), so their c is
# reasoned: fast-noise64 differs from fast-noise32 in the deviate alone, which it reads in float64 and rounds once with the product --
# no more error than the float32 pair, the same c (its loads on the emulator need 4.8e-7); the exact chain of a complex64 plan rounds the float64 product sigma n once to
# float32, 2^-24 = 6e-8 of |kref_m|, and 3 x that is 2e-7.
C_BOUND = {FAST_NATIVE: {"c64": 3e-6, "c128": 4e-6}, FAST_NOISE64: {"c64": 4e-6}, FAST_NOISE32: {"c64": 4e-6},
           EXACT: {"c64": 2e-7, "c128": 3e-15}}
for _cls in C_BOUND:
    for _dt in C_BOUND[_cls]:
        assert C_BOUND[_cls][_dt] <= CAP[_cls][_dt], (_cls, _dt)

# id -> (class, noise kind, route, (emit, noise64, noise32, pot, slab) as fastgen_variant takes them or None for the exact kernel)
VARIANTS = {
    "A": (FAST_NATIVE, "native", "field", (0, 0, 0, 0, 0)),
    "B": (FAST_NATIVE, "native", "potential", (0, 0, 0, 1, 0)),
    "C": (FAST_NATIVE, "native", "scaled", (1, 0, 0, 0, 0)),
    "D": (FAST_NOISE64, "reference", "field", (0, 1, 0, 0, 0)),
    "E": (FAST_NOISE32, "reference", "field", (0, 0, 1, 0, 0)),
    "F": (FAST_NOISE32, "reference", "potential", (0, 0, 1, 1, 0)),
    "G": (FAST_NOISE32, "reference", "scaled", (1, 0, 1, 0, 0)),
    "H": (EXACT, "native", "field", None),
    "I": (EXACT, "reference", "field", None),
    "J": (FAST_NATIVE, "native", "field", (0, 0, 0, 0, 1)),
    "K": (FAST_NATIVE, "native", "field", (0, 0, 0, 0, 0)),
    "K'": (FAST_NATIVE, "native", "potential", (0, 0, 0, 1, 0)),
}
C64_ONLY, C128_ONLY, LONG_ONLY = ("D", "E", "F", "G"), ("I",), ("K", "K'")
NRANKS = 2

WORST = {}           # (class, dtype name) -> (largest need seen, where); ("field ...", dtype name) -> the secondary checks


# ---- the shape table and its regime guards ------------------------------------------------------------------------------------
def fast_supported(dtype, nx):
    """rf_select.h fastgen_supported: every length but 2048 on float64 plans (tile + twiddles + records exceed a CU's LDS)"""
    return not (dtype == C128 and nx == 2048)


def replicate_supported(dtype, nx, nranks=NRANKS):
    """rf_select.h col_replicate_supported: the x pass has an LDS stage (two passes and more: nx >= 32) and nx / nranks is a multiple
    of the last pass's row stride -- with two ranks it always is"""
    return fast_supported(dtype, nx) and nx >= 32 and nx % nranks == 0


def variant_of(dtype, nx, flags):
    """rf_select.h fastgen_variant restated for the flag sets of VARIANTS: (slab, pot, src, halves), None where it is invalid.  The
    coverage guard (tests/test_emulator_generation_matrix.py) holds it against the function itself."""
    emit, n64, n32, pot, slab = flags
    if not fast_supported(dtype, nx) or (dtype == C128 and (n64 or n32)):
        return None
    two = nx == (2048 if dtype == C64 else 1024)
    if emit:
        if slab or pot or n64:
            return None
        return (0, 2, 2, False) if n32 else (0, 2, 0, two)
    if n64:
        return None if (slab or pot) else (0, 0, 1, False)
    if n32:
        return None if slab else (0, 1 if pot else 0, 2, False)
    if pot:
        return None if slab else (0, 1, 0, False)
    if slab:
        return (1, 0, 0, False)
    return (0, 0, 0, two)


def shapes(nx, dtype):
    extra = ((1024, 8, 32),) if (nx, dtype) == (1024, C64) else ()
    return ((nx, 8, 16), (nx, 8, 128)) + extra


def expected_form(shape, dtype, vid, kz0=0, nranks=1):
    """(split, side, pairs per ky row or 0) of the fast pass fastgen_sequence plans for this case -- restated from rf_select.h
    (fastgen_sequence, fast_pass_of), checked against the emulator's export by the coverage guard"""
    nx, ny, nz = shape
    nzl, tc = nz // 2 // nranks, am.TILE_COLS[dtype][nx]
    slab, pot, src, halves = variant_of(dtype, nx, VARIANTS[vid][3])
    cn = nx // 2 if halves else nx                      # the configuration's own length
    split = nzl > tc and nzl % tc == 0
    side = split and kz0 == 0 and cn >= 512
    pairs = (dtype == C64 and nx == 1024 and not halves and src in (0, 2) and not slab and split and (nzl // tc) % 2 == 0)
    return split, side, (nzl // tc // 2 if pairs else 0)


def mt_blocks(shape):
    """segment length (blocks of 624 words = 156 polar attempts) of the replayed stream: 16 -- 2496 attempts, about 1960 pairs, a
    few to a few hundred segments per grid -- except on the three smallest grids, whose 576 ... 2304 cells end before or on the
    first boundary of such segments: one block there (156 attempts, 4 x the 9 cells of a row and more)"""
    nx, ny, nz = shape
    return MT_BLOCKS if nx * ny * (nz // 2 + 1) >= 4000 else 1


def guard(nx, dtype):
    """plain asserts on the table: a shape edited out of its regime fails here instead of passing for nothing"""
    short, long_ = shapes(nx, dtype)[:2]
    for shape in shapes(nx, dtype):
        assert shape[0] == nx and am.tiled(shape, dtype, packed=True), (shape, dtype_name(dtype), "is a generic shape")
    if not fast_supported(dtype, nx):                   # the exact kernel runs every tile in one launch
        return
    assert expected_form(short, dtype, "A")[0] is False, (short, "splits")
    split, side, ppi = expected_form(long_, dtype, "A")
    assert split and side == (nx >= 512), (long_, split, side)
    if (nx, dtype) == (1024, C64):
        assert ppi == 4 and expected_form((1024, 8, 32), dtype, "A") == (True, True, 1)
        assert expected_form(long_, dtype, "D")[2] == 0 and expected_form(long_, dtype, "E")[2] == 4      # float64 deviates: no pairs
    else:
        assert ppi == 0
    # E - G keep the float32 form: rf_noise_mt19937_ex falls back to float64 deviates when cap < 4 (nz / 2 + 1)
    assert all(156 * mt_blocks(s) >= 4 * (s[2] // 2 + 1) for s in shapes(nx, dtype))
    # rank 1 of the kz-slab pair
    assert (long_[2] // 2) % NRANKS == 0 and am.tiled((nx, 8, long_[2]), dtype, packed=True)


def cases(nx, dtype):
    """(variant id, shape) of one length and dtype, guarded"""
    guard(nx, dtype)
    out = []
    fast = fast_supported(dtype, nx)
    for shape in shapes(nx, dtype):
        for vid in VARIANTS:
            if (vid in C64_ONLY and dtype != C64) or (vid in C128_ONLY and dtype != C128):
                continue
            if vid in LONG_ONLY and shape != (nx, 8, 128):
                continue
            if not fast and vid in ("C", "J", "K", "K'"):       # no kernel to regenerate, replicate or cut into kz slabs with
                continue
            if vid == "J" and not replicate_supported(dtype, nx):
                continue
            out.append((vid, shape))
    return out


def class_of(vid, dtype, nx):
    """float64 plans at nx = 2048 have no fast kernel: their A and B run the exact chain"""
    return VARIANTS[vid][0] if fast_supported(dtype, nx) else EXACT


def seeds(nx):
    """(native seed, seed of the replayed stream): distinct per length"""
    return 1000 + nx, 2000 + nx


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
class Oracle(object):
    pass


_ORACLES = {}


def forget_oracles():
    _ORACLES.clear()


def oracle(shape, noise_dtype, kind, seed, power):
    """cpu_ref's stages in float64, once per (shape, stream): shared between the variants, read-only"""
    key = (shape, dtype_name(noise_dtype), kind, seed)
    if key in _ORACLES:
        return _ORACLES[key]
    nx, ny, nz = shape
    k, Pk = power["k"], power["Pk"]
    o = Oracle()
    o.noise = (cpu_ref.native_noise(seed, nx, ny, nz, noise_dtype) if kind == "native" else cpu_ref.reference_noise(seed, nx * ny * (nz // 2 + 1)))
    o.kref = cpu_ref.generate_kspace(nx, ny, nz, SPACING, k, Pk, noise=o.noise, dtype=C128)
    o.sigma = cpu_ref.tabulate_sigmas(cpu_ref.fill_log10k(nx, ny, nz, SPACING, C128), k, Pk, SPACING).real.copy()
    from randomfield_amd import powertools
    kx2, ky2, kz2 = powertools.ksq_axes(nx, ny, nz, SPACING)
    o.k2 = kx2[:, None, None] + ky2[None, :, None] + kz2[None, None, :]
    o.live = o.sigma > 0
    assert not o.live[0, 0, 0] and np.all(o.kref[~o.live] == 0)
    n = np.zeros_like(o.kref)
    n[o.live] = o.kref[o.live] / o.sigma[o.live]
    o.den = o.sigma * (1.0 + np.abs(n))
    o.field = am.irfftn(o.kref, shape)
    o.rms = am.rms_of(o.field)
    with np.errstate(divide="ignore", invalid="ignore"):
        pk = np.where(o.k2 > 0, o.kref / o.k2, 0)
    o.phi_rms = am.rms_of(am.irfftn(pk, shape))
    for a in (o.noise, o.kref, o.sigma, o.k2, o.den, o.field):
        a.setflags(write=False)
    _ORACLES[key] = o
    return o


def oracle_for(vid, shape, dtype, power):
    cls, kind = class_of(vid, dtype, shape[0]), VARIANTS[vid][1]
    native_seed, stream_seed = seeds(shape[0])
    noise_dtype = dtype if cls == EXACT else C64           # the fast pass draws the float32 stream on either plan type
    return oracle(shape, noise_dtype, kind, native_seed if kind == "native" else stream_seed, power)


# ---- the replayed stream on the host: per-segment accepted counts ------------------------------------------------------------
def stream_runs(seed, first, blocks):
    """the float32 pairs of the stream where the one-pass replay leaves them: segment s's accepted pairs densely from slot
    s x 156 blocks, [nseg x cap][2]"""
    cap, nseg = 156 * blocks, len(first) - 1
    pairs = cpu_ref.reference_noise(seed, int(first[-1])).astype(np.float32).reshape(-1, 2)
    runs = np.zeros((nseg * cap, 2), np.float32)
    for s in range(nseg):
        a, b = int(first[s]), int(first[s + 1])
        runs[s * cap:s * cap + (b - a)] = pairs[a:b]
    return runs


def rows_cut(first, shape):
    """rows (ix, iy) of the stream that a segment boundary cuts: the row's nz / 2 + 1 cells lie in two segments"""
    nx, ny, nz = shape
    nzh = nz // 2 + 1
    inside = first[1:-1].astype(np.int64)
    inside = inside[inside < nx * ny * nzh]
    return int(np.count_nonzero(inside % nzh))


# ---- checks -------------------------------------------------------------------------------------------------------------------------
def _record(key, dtype, value, where):
    key = (key, dtype_name(dtype))
    if key not in WORST or not value <= WORST[key][0]:
        WORST[key] = (value, where)


def window_error(o, dtype, shape, transform, scale):
    """The scaled route's window measured by itself: the oracle's own potential spectrum, rounded to the plan's dtype, through the
    same c2r (`transform`: half spectrum -> field, no generation involved) and back by rfftn in float64.  Returns the worst error of
    one mode in units of the white level sqrt(N) rms(field) -- 1 would be all modes at the rms a white error of 1 rms per cell has."""
    key = "window " + dtype_name(dtype)
    if not hasattr(o, key):
        nx, ny, nz = shape
        with np.errstate(divide="ignore", invalid="ignore"):
            pref = (np.where(o.k2 > 0, o.kref / o.k2, 0) * scale).astype(dtype)
        back = am.rfftn(transform(pref))
        level = float(np.sqrt(nx * ny * nz)) * abs(scale) * o.phi_rms
        setattr(o, key, float(np.max(np.abs(back - pref.astype(C128)))) / level)
    return getattr(o, key)


def floor_of(vid, o, dtype, shape, window=None):
    """floor_m of the variant's route (module docstring) and the bound on |got| of the modes with sigma = 0"""
    nx, ny, nz = shape
    route, root_n = VARIANTS[vid][2], float(np.sqrt(nx * ny * nz))
    if route == "potential":
        return np.zeros(o.kref.shape), 0.0
    if route == "field":
        unit = FFT_TERM[dtype] * root_n * o.rms
    else:
        unit = WINDOW_MARGIN * window * root_n * o.phi_rms * o.k2
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(o.live, unit / o.sigma, 0.0), FFT_TERM[dtype] * root_n * o.rms


def check_modes(vid, got, o, dtype, shape, floor, dead_bound, what=""):
    """every mode of the half spectrum against the oracle: returns `need`"""
    cls = class_of(vid, dtype, shape[0])
    nx, ny, nz = shape
    assert got.shape == o.kref.shape == (nx, ny, nz // 2 + 1) and got.dtype == C128, (vid, shape, got.shape, got.dtype)
    c = C_BOUND[cls][dtype_name(dtype)]
    assert np.all(np.abs(got[~o.live]) <= dead_bound), "%s %s %s: a mode with sigma = 0 holds %.3e" % (vid, shape, dtype_name(dtype), float(np.abs(got[~o.live]).max()))
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(o.live, np.abs(got - o.kref) / o.den, 0.0)
    assert e.shape == o.kref.shape and e.size == nx * ny * (nz // 2 + 1) and np.all(np.isfinite(got))        # no mode is left out
    need = e - floor
    at = np.unravel_index(int(np.argmax(need)), need.shape)
    worst = float(need[at])
    sharp = float(np.mean(floor[o.live] <= c))             # modes whose floor does not blunt the bound beyond 2 c
    print("%-2s %-14s %-4s %-12s%s need %.3e / c %.1e = %.3g   (max e_m %.3e; floor <= c on %.1f %% of the modes)" % (
        vid, shape, dtype_name(dtype), cls, what, worst, c, worst / c, float(e.max()), 100 * sharp))
    _record(cls + what, dtype, worst, (vid, shape))
    _record("least resolved" + what + " " + VARIANTS[vid][2], dtype, 1.0 - sharp, (vid, shape))
    assert worst <= c, "%s %s %s (%s%s): mode %s is off by %.3e sigma (1 + |n|), floor %.3e, c %.1e" % (
        vid, shape, dtype_name(dtype), cls, what, at, float(e[at]), float(floor[at]), c)
    return worst


def check_loads(vid, packed, o, dtype, shape, scale):
    """Emulator only: the packed cells the pass LOADS (emu_realise_fast_ex(finish="loads"): what the variant's IO generates, the
    kz = 0 slot repaired, no transform behind it; cplx [nx][ny][nz / 2]) -- the pass's own k-space values of EVERY variant, pot = 2
    and the field-route ones included, with no transform's floor.  The kz = 0 slot holds plane 0 + i plane nz / 2, taken apart
    by the planes' Hermitian symmetry; the sum was rounded once to float32 (rf_core.h fast_fix_kz0; float64 where a float64 plan
    scales the potential), so those two planes have the floor 2^-24 (|a| + |b|) / 2 of the two slots a, b that are combined --
    it matters for the Nyquist plane, whose cells are small next to plane 0's.  C, G: times k^2 / scale."""
    nx, ny, nz = shape
    nzc = nz // 2
    assert packed.shape == (nx, ny, nzc) and packed.dtype == dtype
    packed = packed.astype(C128)
    jx, jy = (-np.arange(nx)) % nx, (-np.arange(ny)) % ny
    a, b = packed[:, :, 0], np.conj(packed[jx][:, jy, 0])
    got = np.empty(o.kref.shape, C128)
    got[:, :, 1:nzc] = packed[:, :, 1:]
    got[:, :, 0], got[:, :, nzc] = 0.5 * (a + b), -0.5j * (a - b)
    factor = o.k2 / abs(scale) if VARIANTS[vid][2] == "scaled" else np.ones(o.k2.shape)
    got *= (o.k2 / scale) if VARIANTS[vid][2] == "scaled" else 1.0
    eps = 2.0 ** -53 if (dtype == C128 and VARIANTS[vid][2] == "scaled") else 2.0 ** -24
    slot = np.zeros(o.kref.shape)
    slot[:, :, 0] = slot[:, :, nzc] = 0.5 * eps * (np.abs(a) + np.abs(b))
    with np.errstate(divide="ignore", invalid="ignore"):
        floor = np.where(o.live, slot * factor / o.sigma, 0.0)
    return check_modes(vid, got, o, dtype, shape, floor, float((slot * factor)[0, 0, 0]), " loads")


def got_of(vid, field, pot, o, scale):
    """the pass's k-space values by the variant's route, in float64"""
    route = VARIANTS[vid][2]
    if route == "potential":
        return pot.astype(C128) * o.k2
    got = am.rfftn(field)
    return got * (o.k2 / scale) if route == "scaled" else got


def check_structure(vid, pot, o, dtype, shape):
    """the stored potential: DC, self-conjugate modes, the Hermitian planes, dead modes -- exact"""
    nx, ny, nz = shape
    assert pot.shape == (nx, ny, nz // 2 + 1) and pot.dtype == dtype, (vid, shape, pot.shape, pot.dtype)
    assert pot[0, 0, 0] == 0, (vid, shape, "DC", pot[0, 0, 0])
    jx, jy = (-np.arange(nx)) % nx, (-np.arange(ny)) % ny
    for iz in (0, nz // 2):
        plane = pot[:, :, iz]
        for ix in (0, nx // 2):
            for iy in (0, ny // 2):
                assert plane[ix, iy].imag == 0, (vid, shape, "self-conjugate mode", (ix, iy, iz), plane[ix, iy])
        mirror = np.conj(plane[jx][:, jy])
        bad = np.argwhere(plane != mirror)
        assert len(bad) == 0, "%s %s %s: plane kz = %d, cell %s is not the conjugate of its mirror image: %r / %r" % (
            vid, shape, dtype_name(dtype), iz, tuple(bad[0]), plane[tuple(bad[0])], mirror[tuple(bad[0])])
    assert np.all(pot[~o.live] == 0)


FIELD_TOL_GPU = 1e-5


def field_tol(vid, dtype, shape, emulator):
    """x rms: TOL_F32 on the GPU (TOL_F64 for the exact kernel of a complex128 plan); the emulator's libm-based deviates keep its
    existing 2e-5, 3e-5 from length 1024 (tests/test_emulator.py)"""
    if class_of(vid, dtype, shape[0]) == EXACT and dtype == C128:
        return 1e-11
    if not emulator:
        return FIELD_TOL_GPU
    return 3e-5 if shape[0] >= 1024 else 2e-5


def check_field(vid, field, std, o, dtype, shape, emulator, scale=None):
    """secondary: the field against irfftn(kref) (C, G: against scale x the potential's), moments() against the float64 std of the
    downloaded field and against the oracle's rms"""
    cls = class_of(vid, dtype, shape[0])
    assert field.shape == tuple(shape) and field.dtype == real_of(dtype), (vid, shape, field.shape, field.dtype)
    if VARIANTS[vid][2] == "scaled":
        with np.errstate(divide="ignore", invalid="ignore"):
            ref = am.irfftn(np.where(o.k2 > 0, o.kref / o.k2, 0) * scale, shape)
        rms = am.rms_of(ref)
    else:
        ref, rms = o.field, o.rms
    tol = field_tol(vid, dtype, shape, emulator)
    err = float(np.max(np.abs(field - ref))) / rms
    print("%-2s %-14s %-4s field: err / rms = %.3e, measured / bound = %.3g" % (vid, shape, dtype_name(dtype), err, err / tol))
    _record("field " + cls, dtype, err, (vid, shape))
    assert err <= tol, "%s %s %s: field off by %.3e rms, bound %.1e" % (vid, shape, dtype_name(dtype), err, tol)
    if std is None:
        return
    own = float(field.astype(np.float64).std())
    e1 = abs(std - own) / own / MOMENT_TOL[dtype]
    # against the oracle: the arithmetic of the class decides -- float32 deviates and sigma (2e-6) or the float64 chain (1e-12)
    tol2 = MOMENT_TOL[C128] if (cls == EXACT and dtype == C128) else MOMENT_TOL[C64]
    e2 = abs(std - rms) / rms / tol2
    print("%-2s %-14s %-4s moments: measured / bound = %.3g (downloaded field), %.3g (oracle rms)" % (vid, shape, dtype_name(dtype), e1, e2))
    _record("moments " + cls, dtype, max(e1, e2), (vid, shape))
    assert e1 <= 1.0 and e2 <= 1.0, "%s %s %s: std %.17g, downloaded field %.17g, oracle %.17g" % (vid, shape, dtype_name(dtype), std, own, rms)


def check_case(vid, result, dtype, shape, power, emulator, transform=None, scale=SCALE):
    """result: (field, potential array or None, moments() std or None[, the pass's loads alone]) of one variant; transform: the
    backend's c2r of an uploaded half spectrum (the scaled route's window is measured with it)"""
    field, pot, std = result[:3]
    o = oracle_for(vid, shape, dtype, power)
    route = VARIANTS[vid][2]
    if route == "potential":
        assert pot is not None
        check_structure(vid, pot, o, dtype, shape)
    window = window_error(o, dtype, shape, transform, scale) if route == "scaled" else None
    floor, dead = floor_of(vid, o, dtype, shape, window)
    need = check_modes(vid, got_of(vid, field, pot, o, scale), o, dtype, shape, floor, dead)
    if len(result) > 3 and result[3] is not None:
        need = max(need, check_loads(vid, result[3], o, dtype, shape, scale))
    check_field(vid, field, std, o, dtype, shape, emulator, scale)
    return need


def check_k_equals_a(field_k, field_a, o, dtype, shape):
    err = float(np.max(np.abs(field_k.astype(np.float64) - field_a))) / o.rms
    print("K  %-14s %-4s against A: err / rms = %.3e, measured / bound = %.3g" % (shape, dtype_name(dtype), err, err / K_VS_A))
    assert err <= K_VS_A, (shape, dtype_name(dtype), err)


def report_worst():
    for key in sorted(WORST):
        print("worst %-24s %-4s %.3e at %s" % (key[0], key[1], WORST[key][0], WORST[key][1]))
