"""Shared by tests/test_gpu_generic_matrix.py and tests/test_emulator_generic_matrix.py: the generic mixed-radix transforms
(csrc/rf_generic.h) at every radix sequence and four-step split -- the table, the guards, the inputs, the numpy float64 references and
the bound.  The counterpart of tests/axis_matrix.py for the kernels whose arithmetic is chosen at run time from the axis length.

One axis carries the length under test, the others make the shape generic by construction (an axis of 6 or 10) with line counts that
are no multiple of a tile:

    role   shape                  plan
    x      (n, 6, 4)              packed (r2c, c2r from k; 18 lines) and c2c (24 lines)
    y      (6, n, 4)              packed and c2c; inner = 3 (packed): a tile of lines straddles runs
    zrow   (6, 10, 2 M)           packed: the contiguous pass transforms M = nz / 2 with the untangle / tangle around it (60 rows)
    zc2c   (4, 6, n)              c2c: the contiguous pass at full length (24 lines)

What an axis length runs -- one line or n1 x n2, each line's radices, in place or in two buffers, with or without the stage tables
behind the line image -- is read from the emulator's exports of the library's own decision (emu_util.generic_shape_form: rf_generic.h
generic_axis_form, generic_factor, generic_split), never from a copy of the factoring here.  coverage() turns the table into the set
of features it reaches per dtype and guard_coverage() asserts every feature the kernels can go wrong at; the drivers assert the
table holds at least the lengths it was designed with, so a removed row fails there or here.

Bound: max |got - ref| over ALL cells <= B s(Rmax) rms(ref).  B is the generic emulator tests' own (tests/test_emulator.py): 3e-6
(complex64) and 3e-14 (complex128) for c2r, four times that for r2c and c2c.  s(Rmax) = max(1, sqrt(Rmax / 64)), Rmax the largest radix
any stage of that shape runs: a prime factor R >= 7 is a dot product of length R, whose rounding grows like sqrt(R).  The references
are numpy's transforms of the float64 cast of the input.  Every check prints measured / bound and keeps the worst per transform, dtype
and role in WORST (CHANGES.md has the figures of the emulator and of the GPU)."""
import functools

import numpy as np

import emu_util

C64, C128 = np.complex64, np.complex128
DTYPES = (C64, C128)
B_C2R = {C64: 3e-6, C128: 3e-14}
ROLES = ("x", "y", "zrow", "zc2c")
AXIS = {"x": 0, "y": 1, "zrow": 2, "zc2c": 2}
BIG_RADIX = 1100                        # a one-thread dot-product stage beyond this takes seconds on the CPU: such rows run one configuration

# lengths of the strided roles (x, y) and of the contiguous c2c role
STRIDED = tuple(2 << i for i in range(13)) + (                                  # every power of two 2 ... 8192: 4s, a lone 2, a merged 8
    6, 10, 12, 18, 20, 24, 30, 40, 50, 60, 96, 100, 120, 360, 1000, 1536,       # smooth: 3 and 5 behind 2 / 4 / 8
    4374,                                                                       # 2 3^7: eight stages
    5000, 6000, 6144, 6250, 7776,                                               # smooth beyond the preferred-split threshold (complex64)
    14, 22, 26, 28, 34, 42, 56, 70, 98, 154, 224, 254, 442,                     # a prime >= 7 behind 2, 4, 8, 3, 5; 7 7; 224 = 4 8 7
    2038, 2310, 3408, 3410, 4078, 6816, 6818, 7168, 8186,                       # primes 1019, 2039, 4093; the stage-table boundary (below)
    8194, 9898, 16384, 4098,                                                    # beyond the one-line cap: 241 x 34, 101 x 98, 128 x 128, 683 x 6
    16382)                                                                      # 8191 x 2: complex64 only (8191 is beyond complex128's cap)
# M = nz / 2 of the packed contiguous pass: odd lines (3, 5 or a prime first), M = 1 (no stage at all), and rows beyond the cap
ZROW_M = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 21, 25, 27, 35, 49, 64, 105, 125, 243, 1019, 2048, 2187, 3125, 4093, 4096, 8194, 4098)
C64_ONLY = {("x", 16382), ("y", 16382), ("zc2c", 16382)}
# where the stage table stops fitting behind the two line images of ONE line (generic_extra_bytes against GENERIC_LDS_MAX; the
# contiguous c2c pass is the one that runs such a line whole): 3 n elem_bytes = 163584 at the lower length of each pair
TABLE_BOUNDARY = {C64: (6816, 6818), C128: (3408, 3410)}

CASES = [(role, n) for role in ("x", "y", "zc2c") for n in STRIDED] + [("zrow", m) for m in ZROW_M]

WORST = {}           # (transform, dtype name, role) -> (largest err / bound seen, err / rms there, where)


def case_id(v):
    return str(v)


def dtype_name(dtype):
    return "c64" if dtype == C64 else "c128"


def real_of(dtype):
    return np.float32 if dtype == C64 else np.float64


def dtypes_of(role, n):
    return (C64,) if (role, n) in C64_ONLY else DTYPES


def shape_of(role, n):
    return {"x": (n, 6, 4), "y": (6, n, 4), "zrow": (6, 10, 2 * n), "zc2c": (4, 6, n)}[role]


def plans_of(role):
    """the plan kinds a role runs: packed (r2c, c2r) and / or c2c"""
    return {"x": (True, False), "y": (True, False), "zrow": (True,), "zc2c": (False,)}[role]


def forms(role, n, dtype, packed):
    """the forms of the three axes of the role's shape; the guard: the shape is served (and 16382 is NOT, in complex128)"""
    shape = shape_of(role, n)
    assert shape[AXIS[role]] == (2 * n if role == "zrow" else n)
    assert any(m in (6, 10) for m in shape), (shape, "is not generic by construction")
    f = emu_util.generic_shape_form(dtype, shape, packed)
    assert f is not None, (shape, dtype_name(dtype), "is not served")
    return f


def rmax_of(f):
    """the largest radix any stage of a shape runs"""
    return max([r for axis in f for line in axis["lines"] for r in line["radices"]] + [1])


def s_of(rmax):
    return max(1.0, float(np.sqrt(rmax / 64.0)))


# ---- what the table reaches, from the library's own decisions ---------------------------------------------------------------------
def line_features(line):
    """features of one line transform (rf_generic.h generic_line_fft)"""
    rad, out = line["radices"], set()
    buf = "inplace" if line["smooth"] else "twobuf"
    for s, r in enumerate(rad):
        where = "first" if s == 0 else "later"
        if r in (2, 3, 4, 5, 8):
            out.add((buf, r, where))
        else:
            out.add(("dot", "only" if len(rad) == 1 else where))
            if r > 1000:
                out.add(("dot", "prime > 1000"))
            if rad.count(r) > 1:
                out.add(("dot", "repeated prime"))
    out.add(("stages", min(len(rad), 6)))                         # 0 (M = 1), 1, 2, ... and 6 for six or more
    if 2 in rad:
        out.add(("lone 2",))
    if 8 in rad and rad.index(8) > 0 and set(rad[:rad.index(8)]) == {4}:
        out.add(("8 behind 4s",))
    out.add(("tables fit", buf, line["tables_fit"]))
    return out


def axis_features(form, cap_forced):
    out = set()
    for line in form["lines"]:
        out |= line_features(line)
    if form["n1"]:
        why = "forced" if cap_forced else "preferred"
        l1, l2 = form["lines"]
        out.add(("split", why))
        if len(l1["radices"]) == 1 and l1["radices"][0] >= 7:
            out.add(("split", why, "prime n1"))
        if form["n1"] % 2:
            out.add(("split", why, "odd n1"))
        if form["n2"] == 2:
            out.add(("split", why, "n2 = 2"))
        if not l2["smooth"]:
            out.add(("split", why, "n2 not smooth"))
    return out


def coverage(dtype, cases=None):
    """every feature the rows of `cases` (default: the table) reach in this dtype, in the form the library runs for each role"""
    out = set()
    for role, n in (CASES if cases is None else cases):
        if dtype not in dtypes_of(role, n):
            continue
        for packed in plans_of(role):
            form = forms(role, n, dtype, packed)[AXIS[role]]
            with emu_util.generic_prefer_split(False):             # (split although the one-line form was not asked for: beyond the cap)
                forced = bool(emu_util.generic_shape_form(dtype, shape_of(role, n), packed)[AXIS[role]]["n1"])
            out |= axis_features(form, forced)
        if role == "zrow" and n == 1:
            out.add(("M = 1",))
    return out


REQUIRED = (
    [(buf, r, where) for buf in ("inplace", "twobuf") for r in (3, 4, 5, 8) for where in ("first", "later")]
    # (a radix 2 is never a later stage: the lone 2 behind a 4 is merged with it into the 8)
    + [("inplace", 2, "first"), ("twobuf", 2, "first")]
    + [("dot", w) for w in ("only", "first", "later", "repeated prime", "prime > 1000")]
    + [("stages", 0), ("stages", 1), ("stages", 2), ("stages", 6), ("lone 2",), ("8 behind 4s",), ("M = 1",)]
    + [("split", why) + rest for why in ("forced", "preferred") for rest in ((), ("prime n1",), ("odd n1",), ("n2 = 2",), ("n2 not smooth",))]
    + [("tables fit", "twobuf", True), ("tables fit", "twobuf", False), ("tables fit", "inplace", True)])


def guard_coverage(cases=None):
    """plain asserts on what the table reaches, per dtype"""
    for dtype in DTYPES:
        have = coverage(dtype, cases)
        missing = [f for f in REQUIRED if f not in have]
        assert not missing, (dtype_name(dtype), "the table no longer reaches", missing)
        # both sides of the boundary where the stage table stops fitting, on the role that runs such a line whole
        lo, hi = TABLE_BOUNDARY[dtype]
        rows = CASES if cases is None else cases
        assert ("zc2c", lo) in rows and ("zc2c", hi) in rows, (dtype_name(dtype), "the stage-table boundary rows are gone")
        flo, fhi = (forms("zc2c", n, dtype, False)[2] for n in (lo, hi))
        assert not flo["n1"] and not fhi["n1"] and not flo["lines"][0]["smooth"] and not fhi["lines"][0]["smooth"]
        assert flo["lines"][0]["tables_fit"] and not fhi["lines"][0]["tables_fit"], (dtype_name(dtype), lo, hi)
    for role, n in C64_ONLY:
        assert emu_util.generic_shape_form(C128, shape_of(role, n), role != "zc2c") is None, (role, n, "is served in complex128: run it")


# ---- inputs (seeded by role and length) and references (numpy on the float64 cast of the input), made once per row and dtype --------
def _seed(role, n):
    return 1000003 * ROLES.index(role) + n


def _complex(rng, shape, dtype):
    return np.ascontiguousarray((rng.normal(size=shape) + 1j * rng.normal(size=shape)).astype(dtype))


def rms_of(ref):
    return float(np.sqrt(np.mean(np.abs(ref) ** 2)))


@functools.lru_cache(maxsize=2)
def row_data(role, n, dtype):
    """inputs and references of one row in one dtype (left unchanged by every user): the half spectrum is random and NOT symmetrised
    -- numpy's irfftn ignores the imaginary parts of the DC and Nyquist bins of every row, and so must the contiguous pass"""
    shape = shape_of(role, n)
    nx, ny, nz = shape
    rng = np.random.RandomState(_seed(role, n))
    d = {"shape": shape}
    if True in plans_of(role):
        d["ks"] = _complex(rng, (nx, ny, nz // 2 + 1), dtype)
        d["c2r"] = np.fft.irfftn(d["ks"].astype(C128), s=shape, axes=(0, 1, 2))
        d["field"] = np.ascontiguousarray(rng.normal(size=shape).astype(real_of(dtype)))
        d["r2c"] = np.fft.rfftn(d["field"].astype(np.float64), axes=(0, 1, 2))
    if False in plans_of(role):
        d["a"] = _complex(rng, shape, dtype)
        d["c2c forward"] = np.fft.fftn(d["a"].astype(C128), axes=(0, 1, 2))
        d["c2c inverse"] = np.fft.ifftn(d["a"].astype(C128), axes=(0, 1, 2))
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def _record(transform, dtype, role, ratio, err_rms, where):
    key = (transform, dtype_name(dtype), role)
    if key not in WORST or not ratio <= WORST[key][0]:
        WORST[key] = (ratio, err_rms, where)


def bound_of(transform, dtype, rmax):
    """B s(Rmax), in units of rms(ref)"""
    return B_C2R[dtype] * (1.0 if transform.startswith("c2r") else 4.0) * s_of(rmax)


def check(transform, got, ref, dtype, role, n, rmax, note=""):
    want_dtype = real_of(dtype) if np.isrealobj(ref) else dtype
    assert got.shape == ref.shape and got.dtype == want_dtype, (transform, role, n, got.shape, got.dtype)
    rms = rms_of(ref)
    tol = bound_of(transform, dtype, rmax)
    err = float(np.max(np.abs(got - ref)))
    print("%s %s %d %s%s: err / rms = %.3e, Rmax = %d, measured / bound = %.3g" % (transform, role, n, dtype_name(dtype), note, err / rms, rmax, err / (tol * rms)))
    _record(transform, dtype, role, err / (tol * rms), err / rms, n)
    assert err <= tol * rms, "%s %s %d %s%s: max error %.3e rms, bound %.2e rms" % (transform, role, n, dtype_name(dtype), note, err / rms, tol)


def check_moments(mean, std, ref, dtype, role, n, rmax, note=""):
    """the (mean, std) the contiguous pass's partials give against the reference's, each within the c2r bound"""
    rms = rms_of(ref)
    bound = bound_of("c2r", dtype, rmax) * rms
    em, es = abs(mean - float(ref.mean())), abs(std - float(ref.std()))
    print("c2r moments %s %d %s%s: measured / bound = %.3g (mean), %.3g (std)" % (role, n, dtype_name(dtype), note, em / bound, es / bound))
    _record("c2r moments", dtype, role, max(em, es) / bound, max(em, es) / rms, n)
    assert em <= bound and es <= bound, "c2r moments %s %d %s%s: mean off by %.3e rms, std by %.3e rms" % (role, n, dtype_name(dtype), note, em / rms, es / rms)


def run_row(role, n, dtype, engine, note=""):
    """every transform of one row in one dtype through `engine`:
         engine.c2r(shape, dtype, ks) -> (field, mean, std);  engine.r2c(shape, dtype, field) -> half spectrum;
         engine.c2c(shape, dtype, a, inverse) -> array
    Returns the arrays it got, by transform."""
    d = row_data(role, n, dtype)
    shape, got = d["shape"], {}
    for packed in plans_of(role):
        rmax = rmax_of(forms(role, n, dtype, packed))
        if packed:
            got["c2r"], mean, std = engine.c2r(shape, dtype, d["ks"])
            check("c2r", got["c2r"], d["c2r"], dtype, role, n, rmax, note)
            check_moments(mean, std, d["c2r"], dtype, role, n, rmax, note)
            got["r2c"] = engine.r2c(shape, dtype, d["field"])
            check("r2c", got["r2c"], d["r2c"], dtype, role, n, rmax, note)
        else:
            for inverse, what in ((False, "c2c forward"), (True, "c2c inverse")):
                got[what] = engine.c2c(shape, dtype, d["a"], inverse)
                check(what, got[what], d[what], dtype, role, n, rmax, note)
    return got


def worst_lines():
    return ["%-12s %-4s %-5s measured / bound %.3g (err %.3e rms) at %s" % (k + v) for k, v in sorted(WORST.items())]
