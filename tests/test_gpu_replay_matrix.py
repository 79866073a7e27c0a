"""The on-GPU replay of RandomState(seed).normal (rf_k_mt.hip, rf_capi_mt.hip) deviate by deviate against numpy's stream, at every
stage of the radix-16 jump tree and every form a segment takes in mt_polar_kernel -- run with -m gpu on an MI355X.  Table, guard,
oracle and bounds: tests/replay_matrix.py; its host side: tests/test_replay_matrix_host.py.

The other replay tests reach the geometries that workload sizes produce (one, 16 or 1024 blocks per segment, at most three stages
of the tree) and compare deviates or fields.  Here short segments put all four stages, four-digit rank starts, odd and cut
segments and partly filled workgroups on grids of a few MB, and the per-segment accepted counts -- the integers that decide
which cell every later deviate lands in -- are compared with the host's exact ones.

Per table row, on one complex64 plan, for two seeds (the second reuses every buffer; one is an array seed):
    a  reference_noise(seed): accepted == the oracle's total; download_noise() against numpy's deviates, <= 1e-15 relative on
       every deviate and > 95 % bit-identical; a failure names the first differing cell, its segment, the stage and multiplier
    b  share_begin(seed) on the same plan: the per-segment counts equal the oracle's, every segment
    c  share_pack, rf_mt_share_exchange_local with one rank, share_finish: bit-identical to (a) (mt_share_pack_kernel against
       mt_compact_kernel)
Rank splits (virtual kz-slab ranks): the shared replay in float64 (e: numpy's values, bit-identical to the single-rank replay, every
rank's counts, the Nyquist plane on every rank) and float32 (f: every deviate in its cell within the float32 bounds); one replicated
replay on two ranks (h).

g  float32 classes of mt_polar_attempt<true> on the 4.2 M-cell case (the shared route with one rank keeps float32 pairs at one block
per segment, where rf_noise_mt19937_ex falls back to float64), worst error in units of |g| 2^-24 against np.float32 of numpy's
deviate, classes by the oracle's float64 r2.  Measured on an MI355X (seed 101, 4 227 072 pairs):
    r2 < 2^-9                      8 266 pairs    3.983     (the exact float64 path)
    2^-9 <= r2 <= 1 - 2^-8     4 202 340 pairs    3.7e6     (the fast path: small deviates from r2 -> 1 carry the 2e-6 absolute
                                                            allowance of (f), which is what bounds this class; reported only)
    r2 > 1 - 2^-8                 16 466 pairs    3.968     (the exact float64 path)
The two band classes are asserted at twice their measured value (the hardware log2 / rcp / sqrt may round an ulp differently for
another seed): 8 |g| 2^-24 = 4.8e-7 |g|, float32 accuracy without the 2e-6 absolute allowance and inside (f)'s 1e-6 relative.
(f)'s "1e-6 relative where |g| > 0.5" failed on the first run of this file -- 1.013e-6 on (64, 64, 256) x 2 ranks, 1.172e-6 on the
4.2 M-cell case, 9.2e-7 on (128, 128, 256) x 4 ranks: attempts with r2 just above 2^-9 and one component |x| < 2^-6, whose deviate
f x reaches 0.5 ... 1.2 while the fast path's left-out second word is up to 1.3e-6 of x.  mt_polar_attempt sends them to the exact
path now (rf_k_mt.hip small_x); measured since: 5.3e-7, 6.0e-7 and 6.0e-7."""
import ctypes

import numpy as np
import pytest

import replay_matrix as rm
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

SPACING = 2.5
# worst error of the two band classes in units of |g| 2^-24, measured (see the header)
CLASS_MEASURED = {0: 3.983, 2: 3.968}
BAND_MIN_PAIRS = 1000


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


@pytest.fixture(scope="module")
def dpower(default_power):
    return default_power["k"], default_power["Pk"]


@pytest.fixture(scope="module", autouse=True)
def one_block_tree():
    """all four stages of the one-block segments' table, built once (a plan that needs fewer stages takes its rows from it)"""
    from randomfield_amd import mt19937
    mt19937.tree_polynomials(4, segment_blocks=1)
    yield
    rm.forget_oracles()


def make_plan(hip, shape, bps, dpower, nranks=1, rank=0):
    from randomfield_amd import powertools
    k, Pk = dpower
    plan = hip.DevicePlan(*shape, np.complex64, nranks=nranks, rank=rank)
    assert plan.tiled
    plan.set_kgrid(*powertools.ksq_axes(*shape, SPACING))
    plan.set_power(*cpu_ref.sigma_table(k, Pk, *shape, SPACING))
    if bps is not None:
        plan.set_mt_segment_blocks(bps)
    return plan


def numpy_seed(seed):
    return list(seed) if isinstance(seed, tuple) else seed


def second_route(hip, plan, counts):
    """share_pack, the local exchange of a one-rank job (the rank's own block), share_finish"""
    plan.share_pack(counts)
    arr = (ctypes.c_void_p * 1)(plan._h.value)
    hip.check(hip.load().rf_mt_share_exchange_local(arr, 1), "rf_mt_share_exchange_local")
    return plan.share_finish()


def side_array(plans, parts, nzc):
    """the (nx, ny, nz / 2 + 1, 2) deviates from the ranks' side arrays (own planes, then the Nyquist plane), as
    tests/test_gpu_parity.py _slab_side_array assembles them"""
    from randomfield_amd import slab
    assert (parts[0].shape[2] - 1) * len(plans) == nzc
    return slab.assemble_side_array(parts)


@pytest.mark.parametrize("case", rm.CASES, ids=rm.case_id)
def test_replay_case(hip, dpower, case):
    shape, bps, seed_a, seed_b = case
    g = rm.geom(shape, bps)
    plan = make_plan(hip, shape, bps, dpower)
    assert plan.share_segments() == (g.nseg, 0, g.nseg), (plan.share_segments(), g.nseg)
    for seed in (seed_a, seed_b):
        o = rm.oracle(shape, bps, seed)
        what = "%s seed %s" % (rm.case_id(case), seed)
        # a. the replay
        accepted = plan.reference_noise(numpy_seed(seed))
        got = plan.download_noise()
        rm.check64(o, got, what + " (a)")
        assert accepted == int(o.first[-1]), (what, accepted, int(o.first[-1]))
        # b. per-segment counts
        counts = plan.share_begin(numpy_seed(seed))
        want = np.diff(o.first)
        bad = np.nonzero(counts != want)[0]
        print("%s (b): %d segments, %d counts differ" % (what, g.nseg, len(bad)))
        assert counts.shape == want.shape and len(bad) == 0, "%s: segment %d of %d holds %d accepted attempts, numpy's stream %d (%d segments differ)" % (
            what, bad[0], g.nseg, counts[bad[0]], want[bad[0]], len(bad))
        # c. the second route places the same float64 values
        assert second_route(hip, plan, counts) == accepted
        again = plan.download_noise()
        same = np.array_equal(again, got)
        print("%s (c): second route bit-identical: %s" % (what, same))
        assert same, "%s: share_pack route: %s" % (what, rm.describe(o, again, got))
    plan.close()


@pytest.mark.parametrize("split", rm.RANK_SPLITS, ids=lambda s: "%dx%dx%d-bps%d-%dranks" % (s[0] + (s[1], s[2])))
def test_shared_replay_rank_split(hip, dpower, split):
    shape, bps, nranks, seed, firsts = split
    nx, ny, nz = shape
    g = rm.geom(shape, bps)
    o = rm.oracle(shape, bps, seed)
    what = "%s x %d ranks" % (shape, nranks)
    one = make_plan(hip, shape, bps, dpower)
    one.reference_noise(seed)
    single_rank = one.download_noise()
    one.close()
    rm.check64(o, single_rank, what + " single rank")
    plans = [make_plan(hip, shape, bps, dpower, nranks, r) for r in range(nranks)]
    bounds = [p.share_segments() for p in plans]
    assert [b[1] for b in bounds] == list(firsts) and all(b[0] == g.nseg for b in bounds) and sum(b[2] for b in bounds) == g.nseg
    want = np.diff(o.first)
    for single in (False, True):
        # every rank's counts are the oracle's slice [first, first + count)
        counts = [p.share_begin(seed, single) for p in plans]
        for r, (c, (nseg, first, count)) in enumerate(zip(counts, bounds)):
            bad = np.nonzero(c != want[first:first + count])[0]
            print("%s single=%s rank %d: segments [%d, %d), %d counts differ" % (what, single, r, first, first + count, len(bad)))
            assert len(c) == count and len(bad) == 0, "%s rank %d (first segment 0x%x): local segment %d holds %d accepted attempts, numpy's stream %d" % (
                what, r, first, bad[0], c[bad[0]], want[first + bad[0]])
        allc = np.concatenate(counts)
        for p in plans:
            p.share_pack(allc)
        arr = (ctypes.c_void_p * nranks)(*[p._h.value for p in plans])
        hip.check(hip.load().rf_mt_share_exchange_local(arr, nranks), "rf_mt_share_exchange_local")
        acc = [p.share_finish() for p in plans]
        assert acc == [int(o.first[-1])] * nranks
        parts = [p.download_noise().reshape(p.k_shape + (2,)) for p in plans]
        got = side_array(plans, parts, nz // 2).reshape(-1)
        for q in parts[1:]:                                             # every rank carries the Nyquist plane
            assert np.array_equal(q[:, :, -1], parts[0][:, :, -1])
        if single:
            rm.check32(o, got, what + " (f)")
        else:
            rm.check64(o, got, what + " (e)")
            assert np.array_equal(got, single_rank), "%s: shared float64 replay against the single-rank one: %s" % (what, rm.describe(o, got, single_rank))
    for p in plans:
        p.close()


def test_float32_classes(hip, dpower):
    """(g) of the header, and (f)'s bounds on a single-rank share of 34 585 segments"""
    shape, bps, seed, _ = rm.LARGEST
    o = rm.oracle(shape, bps, seed)
    plan = make_plan(hip, shape, bps, dpower)
    counts = plan.share_begin(seed, single=True)
    assert np.array_equal(counts, np.diff(o.first))
    second_route(hip, plan, counts)
    got = plan.download_noise()
    plan.close()
    result = rm.class_errors(o, got)
    for i, (name, pairs, worst) in enumerate(result):
        print("float32 class %-24s %8d pairs, worst error %.3f |g| 2^-24" % (name, pairs, worst))
    rm.check32(o, got, "%s float32" % (shape,))
    for i in (0, 2):
        name, pairs, worst = result[i]
        assert pairs >= BAND_MIN_PAIRS, (name, pairs)
        assert worst <= 2.0 * CLASS_MEASURED[i], (name, worst, CLASS_MEASURED[i])


def test_replicated_replay_on_two_ranks(hip, dpower):
    """(h) every rank replays the whole stream and keeps the deviates of its planes and of the Nyquist plane (mt_compact_kernel with
    zpitch != nzh) in segments of three blocks, whose boundaries cut rows"""
    shape, bps, nranks, seed = rm.REPLICATED
    nx, ny, nz = shape
    o = rm.oracle(shape, bps, seed)
    inside = o.first[1:-1].astype(np.int64)
    assert np.count_nonzero(inside[inside < o.geom.ncells] % (nz // 2 + 1)) >= 1, "no row is cut by a segment boundary"
    plans = [make_plan(hip, shape, bps, dpower, nranks, r) for r in range(nranks)]
    for p in plans:
        assert p.reference_noise(seed) == int(o.first[-1])
    parts = [p.download_noise().reshape(p.k_shape + (2,)) for p in plans]
    for q in parts[1:]:
        assert np.array_equal(q[:, :, -1], parts[0][:, :, -1])
    rm.check64(o, side_array(plans, parts, nz // 2).reshape(-1), "%s replicated on %d ranks" % (shape, nranks))
    for p in plans:
        p.close()
