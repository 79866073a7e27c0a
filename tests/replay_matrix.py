"""Shared by tests/test_gpu_replay_matrix.py and tests/test_replay_matrix_host.py: the on-GPU replay of RandomState(seed).normal
(rf_k_mt.hip, rf_capi_mt.hip) held DEVIATE BY DEVIATE against numpy's stream at every stage of the radix-16 jump tree and every form
a segment takes in mt_polar_kernel -- the case table, the geometry rf_capi_mt.hip mt_geom computes for it, the guard that keeps the
table inside its regimes, and the oracle on the host (per-segment accepted counts, r2 of every accepted attempt).

Short segments (set_mt_segment_blocks) make the tree's later stages reachable on grids of a few MB: with one block of 624 words per
segment a 4.2 M-cell stream has 34 585 segments -- stage 3 (rows 45 - 59 of the table, t^(m 16^3 L)) with multipliers 1 ... 8 --
where the default segment length reaches that stage at 2048^3 only.

    CASES          (shape, blocks per segment or None = the default length, seed, second seed on the same plan)
    RANK_SPLITS    (shape, blocks per segment, virtual kz-slab ranks, seed): the shared replay (rf_mt_share_*), whose ranks jump
                   to their first segment with one jump per non-zero radix-16 digit of its index
    REPLICATED     one 2-rank job on which every rank replays the whole stream and keeps its planes (mt_compact_kernel's
                   zpitch != nzh branch, rows cut by segment boundaries)

Bounds are the project's own (tests/test_gpu_parity.py): float64 deviates <= 1e-15 relative on every deviate and > 95 % of them
bit-identical (test_mt19937_replay_matches_numpy); float32 deviates max(dev - 3e-7 |g|) <= 2e-6, rms <= 2e-7 and <= 1e-6 relative
where |g| > 0.5 (test_shared_reference_stream_small).  Accepted counts are integers and compared exactly."""
import numpy as np

import axis_matrix as am
from oracle import cpu_ref

RADIX = 16                                       # mt19937.TREE_RADIX
MT_COMPACT_CHUNK = 16384                         # rf_k_mt.hip: pairs per workgroup of mt_compact_kernel / mt_share_pack_kernel
ATTEMPTS_PER_BLOCK = 156                         # 624 words / 4

REL64, IDENTICAL64 = 1e-15, 0.95                 # test_mt19937_replay_matches_numpy
F32_SLOPE, F32_ABS, F32_RMS, F32_REL_LARGE = 3e-7, 2e-6, 2e-7, 1e-6       # test_shared_reference_stream_small

ARRAY_SEED = (2026, 4, 0xFFFFFFFF, 7)            # init_by_array

# (shape, blocks per segment, seed, second seed)
CASES = [
    ((8, 8, 16), 1, 11, 12),                     # stage 0 only, partial workgroup
    ((8, 8, 16), 2, 21, 22),                     # pair loop, last segment cut to one block
    ((16, 16, 16), 3, 31, 32),                   # pair + odd block + copy back
    ((16, 16, 32), 1, 41, 42),                   # stage 1 with a partial last multiplier
    ((32, 32, 64), 3, 51, ARRAY_SEED),           # odd bps, even cut
    ((32, 32, 64), 1, 61, 62),                   # stage 2: 256 sources, destinations cut at nseg inside m = 1
    ((64, 64, 256), 16, 71, 72),                 # stage 2, odd cut of an even bps
    ((64, 64, 64), 107, 81, 82),                 # cap = 16 692 > MT_COMPACT_CHUNK: second chunk entirely empty
    ((64, 64, 256), 1, 91, 92),                  # stage 3, m = 1 only
    ((256, 128, 256), 1, 101, 102),              # stage 3, multipliers 1 ... 8, every source
    ((32, 32, 64), None, 111, 112),              # the default segment length: one segment, no jump at all
]
LARGEST = ((256, 128, 256), 1, 101, 102)         # the 4.2 M-cell case: the float32 classes are measured on it

# (shape, blocks per segment, ranks, seed, the ranks' first segments)
RANK_SPLITS = [
    ((128, 128, 256), 1, 4, 131, (0, 0x10e8, 0x21d0, 0x32b8)),
    ((64, 64, 256), 1, 2, 141, (0, 0x87d)),
]
REPLICATED = ((32, 32, 64), 3, 2, 151)


def case_id(case):
    shape, bps = case[0], case[1]
    return "%dx%dx%d-bps%s" % (shape + ("default" if bps is None else str(bps),))


# ---- geometry, as rf_capi_mt.hip mt_geom computes it ---------------------------------------------------------------------------
class Geom(object):
    pass


def geom(shape, bps):
    from randomfield_amd import mt19937
    nx, ny, nz = shape
    g = Geom()
    g.ncells = nx * ny * (nz // 2 + 1)
    g.attempts = mt19937.attempts_needed(g.ncells)
    g.total_blocks = -(-4 * g.attempts // 624)
    g.bps = mt19937.segment_blocks_for(g.ncells) if bps is None else bps
    g.nseg = -(-g.total_blocks // g.bps)
    g.stages, reach = 0, 1
    while reach < g.nseg:
        reach *= RADIX
        g.stages += 1
    g.last_nb = g.total_blocks - (g.nseg - 1) * g.bps
    g.cap = ATTEMPTS_PER_BLOCK * g.bps
    return g


def rank_tiled(shape, nranks):
    """rf_capi.hip shape_check for a complex64 plan of `nranks` kz-slab ranks"""
    nx, ny, nz = shape
    nzc = nz // 2
    if not am.tiled(shape, am.C64, packed=True) or nx % nranks or nzc % nranks or (nzc // nranks) % 2:
        return False
    nzl = nzc // nranks
    return (ny * nzl) % am.TILE_COLS[am.C64][nx] == 0 and (nx * nzl) % am.TILE_COLS[am.C64][ny] == 0


def digits(s):
    """radix-16 digits of a segment index, lowest first"""
    out = []
    while s:
        out.append(s % RADIX)
        s //= RADIX
    return out


def guard(cases=None, splits=None, replicated=None):
    """plain asserts: every regime of the jump tree and of the segment loop is in the table -- a row edited out of its regime, or
    removed, fails here instead of leaving the suite passing for nothing"""
    cases = CASES if cases is None else cases
    splits = RANK_SPLITS if splits is None else splits
    replicated = REPLICATED if replicated is None else replicated
    gs = []
    for case in cases:
        shape, bps = case[0], case[1]
        assert am.tiled(shape, am.C64, packed=True), (shape, "is a generic shape")
        g = geom(shape, bps)
        assert 1 <= g.last_nb <= g.bps and g.stages <= 4, (shape, bps)
        gs.append((g, bps))
    short = [g for g, bps in gs if bps is not None]
    # the tree: stage t as the last one, t = 0 ... 3; no jump at all on a default-length case
    assert any(bps is None and g.nseg == 1 and g.stages == 0 for g, bps in gs), "no default-length case without a jump"
    for stages in (1, 2, 3, 4):
        assert any(g.stages == stages for g in short), "no case whose last stage is %d" % (stages - 1)
    # stage 0 alone in a partly filled workgroup (four segments per workgroup of mt_polar_kernel)
    assert any(g.stages == 1 and g.nseg % 4 for g in short)
    # stage 1: the last multiplier's destinations end before all 16 sources have one
    assert any(g.stages == 2 and g.nseg % RADIX for g in short)
    # stage 2 (all 15 multipliers in one workgroup): destinations cut at nseg inside m = 1, and a case with m >= 2
    assert any(g.stages == 3 and RADIX ** 2 < g.nseg < 2 * RADIX ** 2 for g in short), "no stage-2 case cut inside m = 1"
    assert any(g.stages == 3 and g.nseg >= 2 * RADIX ** 2 for g in short) or any(g.stages == 4 for g in short)
    # stage 3: m = 1 only with fewer destinations than sources, and m >= 2 with every source
    assert any(g.stages == 4 and g.nseg < 2 * RADIX ** 3 for g in short), "no stage-3 case cut inside m = 1"
    assert any(g.stages == 4 and g.nseg >= 2 * RADIX ** 3 for g in short), "no stage-3 case with m >= 2"
    # the block-pair loop of mt_polar_kernel: bps = 1 (odd block only), even (pairs only), odd > 1 (pairs, odd block, copy back)
    assert any(g.bps == 1 for g in short), "no case with one block per segment"
    assert any(g.bps % 2 == 0 for g in short), "no case with an even number of blocks per segment"
    assert any(g.bps % 2 == 1 and g.bps > 1 for g in short), "no case with an odd number > 1 of blocks per segment"
    # a last segment cut short, to an odd and to an even number of blocks
    assert any(g.last_nb < g.bps and g.last_nb % 2 == 1 for g in short), "no last segment cut to an odd number of blocks"
    assert any(g.last_nb < g.bps and g.last_nb % 2 == 0 for g in short), "no last segment cut to an even number of blocks"
    assert any(g.bps % 2 == 0 and g.last_nb < g.bps and g.last_nb % 2 == 1 and g.last_nb > 1 for g in short), "no odd cut > 1 of an even bps"
    assert any(g.bps % 2 == 1 and g.last_nb < g.bps and g.last_nb % 2 == 0 for g in short), "no even cut of an odd bps"
    # a last segment of ONE block (no pair at all) behind segments that run pairs: of an even and of an odd bps
    assert any(g.bps % 2 == 0 and g.last_nb == 1 for g in short), "no even bps whose last segment is one block"
    assert any(g.bps % 2 == 1 and g.bps > 1 and g.last_nb == 1 for g in short), "no odd bps > 1 whose last segment is one block"
    # one block per segment (the most segments per deviate, the float64 form) at every depth of the tree
    for stages in (1, 2, 3, 4):
        assert any(g.bps == 1 and g.stages == stages for g in short), "no bps = 1 case whose last stage is %d" % (stages - 1)
    # waves that leave a workgroup early: every residue of nseg mod 4
    for r in range(4):
        assert any(g.nseg % 4 == r for g in short), "no case with nseg %% 4 == %d" % r
    # more pairs per segment than one workgroup of the compaction takes
    assert any(g.cap > MT_COMPACT_CHUNK for g in short), "no case with 156 bps > %d" % MT_COMPACT_CHUNK
    # one array seed (init_by_array) among the second seeds, integers otherwise
    assert any(isinstance(c[3], tuple) for c in cases), "no array seed"
    assert all(isinstance(c[2], int) for c in cases) and all(isinstance(c[3], (int, tuple)) for c in cases)
    assert LARGEST in cases and geom(LARGEST[0], LARGEST[1]).ncells >= 4000000

    # the shared replay: four-digit starts, one with a zero digit between non-zero ones, one with a zero low digit; a three-digit one
    starts = []
    for shape, bps, nranks, seed, first in splits:
        assert rank_tiled(shape, nranks), (shape, nranks)
        g = geom(shape, bps)
        mine = tuple(r * g.nseg // nranks for r in range(nranks))
        assert mine == tuple(first), (shape, bps, [hex(v) for v in mine])
        starts += [(digits(s), (r + 1) * g.nseg // nranks - s) for r, s in enumerate(mine) if s]
    four = [d for d, n in starts if len(d) == 4]
    assert len(four) >= 3, "fewer than three four-digit starts"
    assert any(d[0] == 0 for d in four), "no four-digit start with a zero low digit"
    assert any(0 in d[1:3] and d[0] != 0 for d in four), "no four-digit start with a zero digit between non-zero ones"
    assert any(all(d) for d in four), "no four-digit start without a zero digit"
    assert any(len(d) == 3 for d, n in starts), "no three-digit start"
    assert any(len(d) == 4 and n > RADIX ** 3 for d, n in starts), "no rank with a four-stage local tree behind a four-digit start"

    shape, bps, nranks, seed = replicated
    g = geom(shape, bps)
    assert rank_tiled(shape, nranks) and nranks > 1 and g.nseg > nranks and g.bps % 2 == 1 and g.bps > 1, replicated


# ---- the replayed stream on the host -------------------------------------------------------------------------------------------
def _numpy_seed(seed):
    return list(seed) if isinstance(seed, tuple) else seed


def stream_attempts(seed, ncells, blocks):
    """(accepted?, r2, nseg) of every polar attempt of the segments of `blocks` x 624 words that the replay runs for ncells cells of
    RandomState(seed)'s stream: mt19937.sequence / temper and numpy's acceptance rule (legacy_gauss: 0 < r2 < 1 on 53-bit doubles
    from two words each).  The last segment ends with the stream's last block (rf_capi_mt.hip mt_geom total_blocks): the attempts
    behind it are never made and count as not accepted."""
    from randomfield_amd import mt19937
    total_blocks = -(-4 * mt19937.attempts_needed(ncells) // 624)
    nseg = -(-total_blocks // blocks)
    # (the generator's outputs are the tempered words BEHIND the state it is seeded with: the state's own 624 words are never drawn)
    seq = mt19937.sequence(mt19937.seed_state(_numpy_seed(seed)), (nseg * blocks + 1) * 624)[624:]
    words = mt19937.temper(seq).astype(np.uint64).reshape(-1, 4)
    x = [((words[:, 2 * i] >> np.uint64(5)).astype(np.float64) * 67108864.0 + (words[:, 2 * i + 1] >> np.uint64(6)).astype(np.float64)) / 9007199254740992.0
         for i in (0, 1)]
    x1, x2 = 2.0 * x[0] - 1.0, 2.0 * x[1] - 1.0
    r2 = x1 * x1 + x2 * x2
    ok = (r2 < 1.0) & (r2 != 0.0)
    ok[total_blocks * ATTEMPTS_PER_BLOCK:] = False
    return ok, r2, nseg


def _scan(ok, nseg, blocks):
    first = np.zeros(nseg + 1, np.uint64)
    first[1:] = np.cumsum(ok.reshape(nseg, blocks * ATTEMPTS_PER_BLOCK).sum(axis=1))
    return first


def stream_segments(seed, ncells, blocks):
    """exclusive scan `first` (nseg + 1 entries) of the accepted polar attempts per segment of the replay of ncells cells"""
    ok, r2, nseg = stream_attempts(seed, ncells, blocks)
    return _scan(ok, nseg, blocks)


class Oracle(object):
    pass


_ORACLES = {}


def forget_oracles():
    _ORACLES.clear()


def oracle(shape, bps, seed):
    """numpy's stream for one (shape, segment length, seed), once, read-only: .noise = RandomState(seed).normal(2 ncells), .first =
    the scan of the accepted counts per segment (stream_segments),
    .r2 = numpy's float64 r2 of the attempt each of the first ncells pairs came from"""
    key = (tuple(shape), bps, seed)
    if key in _ORACLES:
        return _ORACLES[key]
    g = geom(shape, bps)
    o = Oracle()
    o.geom = g
    ok, r2, nseg = stream_attempts(seed, g.ncells, g.bps)
    assert nseg == g.nseg
    o.first = _scan(ok, g.nseg, g.bps)
    o.r2 = r2[ok][:g.ncells].copy()
    o.noise = cpu_ref.reference_noise(_numpy_seed(seed), g.ncells)
    assert int(o.first[-1]) >= g.ncells and len(o.r2) == g.ncells
    for a in (o.first, o.r2, o.noise):
        a.setflags(write=False)
    _ORACLES[key] = o
    return o


def locate(o, cell):
    """the segment that stream cell `cell` lies in, the stage of the jump tree that made the segment's start state and the
    multiplier: segment s = i + m 16^t with i < 16^t"""
    seg = int(np.searchsorted(o.first, np.uint64(cell), side="right")) - 1
    if seg == 0:
        return seg, None, None
    t = len(digits(seg)) - 1
    return seg, t, seg // RADIX ** t


def describe(o, got, ref=None):
    """first differing cell of a flat array of 2 ncells deviates against the oracle's, with its segment, stage and multiplier"""
    ref = o.noise if ref is None else ref
    bad = np.nonzero(~(np.abs(got - ref) <= REL64 * np.abs(ref)))[0]
    if not len(bad):
        return "every deviate within %.0e" % REL64
    cell = int(bad[0]) // 2
    seg, t, m = locate(o, cell)
    return "%d deviates differ; the first at cell %d (got %r, numpy %r): segment %d of %d (cells %d ...), made by stage %s with multiplier %s" % (
        len(bad), cell, float(got[bad[0]]), float(ref[bad[0]]), seg, o.geom.nseg, int(o.first[seg]), t, m)


def check64(o, got, what):
    """float64 deviates against numpy's: the bounds of test_mt19937_replay_matches_numpy"""
    assert got.shape == o.noise.shape and got.dtype == np.float64, (what, got.shape, got.dtype)
    rel = np.abs(got - o.noise) / np.maximum(np.abs(o.noise), 1e-300)
    worst, same = float(np.max(rel)), float(np.mean(got == o.noise))
    print("%s: max relative deviation %.3e (bound %.0e), bit-identical %.2f %%" % (what, worst, REL64, 100 * same))
    assert np.all(np.isfinite(got)) and worst <= REL64, "%s: %s" % (what, describe(o, got))
    assert same > IDENTICAL64, (what, same)


def check32(o, got, what):
    """float32 deviates, widened: each in ITS cell within the bounds of test_shared_reference_stream_small, and float32 values"""
    assert got.shape == o.noise.shape and got.dtype == np.float64, (what, got.shape, got.dtype)
    dev = np.abs(got - o.noise)
    mag = np.abs(o.noise)
    a, rms = float(np.max(dev - F32_SLOPE * mag)), float(np.sqrt(np.mean(dev ** 2)))
    large = float(np.max((dev / np.maximum(mag, 1e-30))[mag > 0.5]))
    print("%s: max(dev - 3e-7 |g|) %.3e (bound %.0e), rms %.3e (bound %.0e), relative where |g| > 0.5 %.3e (bound %.0e)" % (
        what, a, F32_ABS, rms, F32_RMS, large, F32_REL_LARGE))
    if not a <= F32_ABS:
        cell = int(np.argmax(dev - F32_SLOPE * mag)) // 2
        raise AssertionError("%s: cell %d is off by %.3e; segment %d, stage %s, multiplier %s" % ((what, cell, a + 0.0) + locate(o, cell)))
    assert rms <= F32_RMS and large <= F32_REL_LARGE, (what, rms, large)
    assert np.array_equal(got, got.astype(np.float32)), (what, "values are not float32 numbers")


# ---- float32 classes of mt_polar_attempt<true> ---------------------------------------------------------------------------------
R2_LOW, R2_HIGH = 2.0 ** -9, 1.0 - 2.0 ** -8
CLASSES = ("r2 < 2^-9", "2^-9 <= r2 <= 1 - 2^-8", "r2 > 1 - 2^-8")


def class_errors(o, got):
    """worst error per class of the float32 form, in units of |g| 2^-24, against np.float32 of numpy's deviate; the classes by
    the oracle's float64 r2 of the pair's attempt.  Returns [(class, pairs, worst)]"""
    want = o.noise.astype(np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        units = np.where(want != 0, np.abs(got - want) / (np.abs(want) * 2.0 ** -24), 0.0).reshape(-1, 2).max(axis=1)
    masks = (o.r2 < R2_LOW, (o.r2 >= R2_LOW) & (o.r2 <= R2_HIGH), o.r2 > R2_HIGH)
    return [(name, int(np.count_nonzero(m)), float(units[m].max()) if m.any() else 0.0) for name, m in zip(CLASSES, masks)]
