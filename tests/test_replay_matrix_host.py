"""Host side of tests/replay_matrix.py (no GPU): the guard on the case table, and the jump polynomials of stages 2 and 3 of the radix-16
tree -- the rows tests/test_mt19937_host.py stops short of -- against the generator stepped that far, on one-block segments."""
import numpy as np
import pytest

import replay_matrix as rm
from randomfield_amd import mt19937 as mt


def _same_state(a, b):
    """MT19937 states are equal when all words agree except the unused low 31 bits of word 0."""
    a, b = np.asarray(a, np.uint32), np.asarray(b, np.uint32)
    return np.array_equal(a[1:], b[1:]) and ((int(a[0]) ^ int(b[0])) & 0x80000000) == 0


def test_guard_accepts_the_table():
    rm.guard()


@pytest.mark.parametrize("row", range(len(rm.CASES)), ids=[rm.case_id(c) for c in rm.CASES])
def test_guard_rejects_the_table_without_a_row(row):
    """every row is in the table for a regime no other row covers"""
    with pytest.raises(AssertionError):
        rm.guard(cases=rm.CASES[:row] + rm.CASES[row + 1:])


def test_guard_rejects_a_missing_rank_split():
    for i in range(len(rm.RANK_SPLITS)):
        with pytest.raises(AssertionError):
            rm.guard(splits=rm.RANK_SPLITS[:i] + rm.RANK_SPLITS[i + 1:])
    shape, bps, nranks, seed, first = rm.RANK_SPLITS[0]
    with pytest.raises(AssertionError):                                   # the digit patterns come from r nseg // P
        rm.guard(splits=[(shape, bps, nranks, seed, (0, 0x10e8, 0x21d1, 0x32b8)), rm.RANK_SPLITS[1]])


def test_geometry_of_the_table():
    """the figures the table was chosen by: (nseg, stages, blocks of the last segment)"""
    want = {"8x8x16-bps1": (13, 1, 1), "8x8x16-bps2": (7, 1, 1), "16x16x16-bps3": (10, 1, 1), "16x16x32-bps1": (45, 2, 1),
            "32x32x64-bps3": (97, 2, 2), "32x32x64-bps1": (290, 3, 1), "64x64x256-bps16": (272, 3, 11), "64x64x64-bps107": (11, 1, 54),
            "64x64x256-bps1": (4347, 4, 1), "256x128x256-bps1": (34585, 4, 1), "32x32x64-bpsdefault": (1, 0, 290)}
    got = {}
    for case in rm.CASES:
        g = rm.geom(case[0], case[1])
        got[rm.case_id(case)] = (g.nseg, g.stages, g.last_nb)
    assert got == want


def test_oracle_counts_the_last_segment_as_the_replay_runs_it():
    """the scan ends with the pairs of total_blocks blocks, and its first ncells pairs are numpy's"""
    shape, bps, seed = (8, 8, 16), 2, 21
    o = rm.oracle(shape, bps, seed)
    g = o.geom
    assert g.last_nb < bps and len(o.first) == g.nseg + 1
    whole = rm.stream_segments(seed, g.ncells, 1)                          # the same stream in one-block segments: never cut
    assert int(whole[-1]) == int(o.first[-1]) and np.array_equal(whole[::2][:g.nseg], o.first[:-1])
    # r2 of the accepted attempts gives numpy's deviates: f x2, then f x1 -- |g|^2 summed over the pair is -2 ln r2
    pair = o.noise.reshape(-1, 2)
    assert np.allclose(pair[:, 0] ** 2 + pair[:, 1] ** 2, -2.0 * np.log(o.r2), rtol=1e-13, atol=0)


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """all 60 polynomials of one-block segments, built once"""
    mp = pytest.MonkeyPatch()
    mp.setenv("RANDOMFIELD_CACHE_DIR", str(tmp_path_factory.mktemp("mt_cache")))
    mt._TREE_MEMO.pop(1, None)
    try:
        yield mt.tree_polynomials(4, segment_blocks=1)
    finally:
        mt._TREE_MEMO.pop(1, None)
        mp.undo()


def test_stage_2_and_3_polynomials_jump_as_far_as_stepping(tree):
    """rows 30 ... 44 are t^(m 256 L), rows 45 ... 59 t^(m 4096 L), L = 624 words: a jump with one of them lands where the generator
    stepped m 16^t blocks ahead stands"""
    assert tree.shape == (60, mt.N)
    st = mt.init_genrand(2048)
    seq = mt.sequence(st, (2 * 4096 + 1) * mt.N)
    for t, m in ((2, 1), (2, 3), (2, 15), (3, 1), (3, 2)):
        at = m * 16 ** t * mt.N
        assert _same_state(mt.jump_state(st, tree[t * 15 + m - 1]), seq[at:at + mt.N]), (t, m)
    # and no two rows of these stages are the same polynomial (a table that repeats stage 2 under stage 3 would pass nothing above)
    assert len({tree[r].tobytes() for r in range(30, 60)}) == 30


def test_digitwise_jump_to_four_digit_rank_starts(tree):
    """rf_mt_share_begin's hop to a rank's first segment, one jump per non-zero radix-16 digit, for the starts of
    replay_matrix.RANK_SPLITS: four digits, a zero digit in the middle, a zero low digit"""
    st = mt.init_genrand(77)
    starts = [s for split in rm.RANK_SPLITS for s in split[4] if s]
    seq = mt.sequence(st, (max(starts) + 1) * mt.N)
    for s in starts:
        cur = st
        for t, d in enumerate(rm.digits(s)):
            if d:
                cur = mt.jump_state(cur, tree[t * 15 + d - 1])
        assert _same_state(cur, seq[s * mt.N:(s + 1) * mt.N]), hex(s)
