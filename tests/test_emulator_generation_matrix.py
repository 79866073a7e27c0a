"""tests/generation_matrix.py through the CPU emulator -- the same table, oracle, per-mode bound and structural checks as
tests/test_gpu_generation_matrix.py, on the phase functions the kernels inline, with the variant, the IO set-up and the launches
taken from the launchers' own rules (emu_realise_fast_ex: fastgen_variant, FastGen::at, fastgen_sequence, fast_col_io) -- and the
coverage guard that holds the table against rf_select.h.

What differs from the GPU run: the deviates come from the host's libm instead of v_log_f32 / v_sin_f32 / v_cos_f32, so the field
bound is the emulator's existing 2e-5 rms (3e-5 from length 1024, tests/test_emulator.py) while the per-mode bound c is the same;
the exact kernel is the emulator's GenColIO chain (H, I, and A of a float64 plan at nx = 2048 -- its stored potential, B, is made by
kernels the emulator does not have); the ranks of J and K are one x pass each into the whole grid's buffer, the y and z passes run
once behind the last; and every single-rank fast variant is also checked on its loads alone (generation_matrix.check_loads: the
packed cells its IO generates, no transform) -- the window that holds pot = 2 and the field-route variants of float32 plans to c
on more than 99 % of their modes, which no transform of a float32 field can."""
import numpy as np
import pytest

import emu_util
import generation_matrix as gm
from oracle import cpu_ref

C64, C128 = gm.C64, gm.C128
FIX_FILL, COL, COLPAIR, COL2 = 0, 1, 2, 3            # rf_select.h FastKind
LEAN, REPAIR, FIRST = 0, 1, 2                        # FastIo


def _std(field, s1, s2):
    n = float(field.size)
    return float(np.sqrt(s2 / n - (s1 / n) ** 2))


def flags_of(vid):
    emit, n64, n32, pot, slab = gm.VARIANTS[vid][3]
    return dict(emit=bool(emit), n64=bool(n64), n32=bool(n32), pot=bool(pot))


def rank_ranges(vid, shape):
    """[(x0, x1, kz0, nzl)] of the calls that make up one case: one rank, or the two of J (x slabs) and K (kz slabs)"""
    nx, ny, nz = shape
    if vid == "J":
        return [(r * nx // gm.NRANKS, (r + 1) * nx // gm.NRANKS, 0, -1) for r in range(gm.NRANKS)]
    if vid in gm.LONG_ONLY:
        nzl = nz // 2 // gm.NRANKS
        return [(0, 1 << 30, r * nzl, nzl) for r in range(gm.NRANKS)]
    return [(0, 1 << 30, 0, -1)]


def run_variant(vid, shape, dtype, power):
    """(field, potential or None, std from the z pass's sums, loads or None) of one case on the emulator; None where it has no such chain"""
    nx, ny, nz = shape
    rt = gm.real_of(dtype)
    native_seed, stream_seed = gm.seeds(nx)
    xt, st = cpu_ref.sigma_table(power["k"], power["Pk"], nx, ny, nz, gm.SPACING)
    if gm.class_of(vid, dtype, nx) == gm.EXACT:
        if gm.VARIANTS[vid][2] != "field":
            return None
        noise = gm.oracle_for(vid, shape, dtype, power).noise if vid == "I" else None
        field, s1, s2 = emu_util.realise(nx, ny, nz, gm.SPACING, xt, st, seed=native_seed, noise=noise, dtype=dtype)
        return field, None, _std(field, s1, s2)
    kw = dict(dtype=rt, pot={"field": 0, "potential": 1, "scaled": 2}[gm.VARIANTS[vid][2]], pscale=gm.SCALE)
    if vid == "D":
        kw["noise64"] = gm.oracle_for(vid, shape, dtype, power).noise
    if vid in ("E", "F", "G"):
        blocks = gm.mt_blocks(shape)
        first = gm.stream_segments(stream_seed, nx * ny * (nz // 2 + 1), blocks)
        assert gm.rows_cut(first, shape) >= 1, (shape, "no row of the grid is cut by a segment boundary")
        kw.update(noise32=gm.stream_runs(stream_seed, first, blocks), first=first, cap=156 * blocks)
    ranges = rank_ranges(vid, shape)
    field, pots = None, []
    for i, (x0, x1, kz0, nzl) in enumerate(ranges):
        field, s1, s2, p = emu_util.realise_fast_ex(nx, ny, nz, gm.SPACING, xt, st, native_seed, x0=x0, x1=x1, kz0=kz0, nzl=nzl,
                                                    finish=i == len(ranges) - 1, field=field, **kw)
        pots.append(p)
    pot = None
    if kw["pot"] == 1:
        from randomfield_amd import slab
        pot = slab.assemble_side_array(pots) if len(pots) > 1 else pots[0]
    loads = None
    if len(ranges) == 1:                               # the pass's loads alone, no transform (generation_matrix.check_loads)
        loads = emu_util.realise_fast_ex(nx, ny, nz, gm.SPACING, xt, st, native_seed, finish="loads", **kw)[0].view(dtype).copy()
    return field, pot, _std(field, s1, s2), loads


@pytest.mark.parametrize("nx", gm.am.COL_LENGTHS, ids=gm.case_id)
def test_generation_pass_mode_by_mode(default_power, nx):
    try:
        for dtype in gm.am.DTYPES:
            fields = {}
            for vid, shape in gm.cases(nx, dtype):
                result = run_variant(vid, shape, dtype, default_power)
                if result is None:
                    assert (vid, dtype, nx) == ("B", C128, 2048)
                    continue
                gm.check_case(vid, result, dtype, shape, default_power, emulator=True, transform=lambda ks: emu_util.c2r(ks)[0])
                if vid in ("A", "K"):
                    fields[vid, shape] = result[0]
            for (vid, shape), field in fields.items():
                if vid == "K":
                    gm.check_k_equals_a(field, fields["A", shape], gm.oracle_for("A", shape, dtype, default_power), dtype, shape)
        gm.report_worst()
    finally:
        gm.forget_oracles()


# ---- the coverage guard -----------------------------------------------------------------------------------------------------------
def all_flag_sets():
    return [tuple((i >> b) & 1 for b in range(5)) for i in range(32)]          # (emit, n64, n32, pot, slab)


def test_variant_rule_restated():
    """generation_matrix.variant_of is rf_select.h fastgen_variant, for every flag combination at every length and dtype; and the
    other rules the table restates"""
    assert gm.am.COL_LENGTHS == gm.em.header_sizes("RF_COL_SIZES")
    for dtype in gm.am.DTYPES:
        f64 = dtype == C128
        for nx in gm.am.COL_LENGTHS:
            for flags in all_flag_sets():
                emit, n64, n32, pot, slab = flags
                assert gm.variant_of(dtype, nx, flags) == emu_util.fastgen_variant(f64, nx, emit, n64, n32, pot, slab), (gm.dtype_name(dtype), nx, flags)
            assert gm.replicate_supported(dtype, nx) == emu_util.col_replicate_supported(f64, nx, gm.NRANKS)
            assert gm.fast_supported(dtype, nx) == (emu_util.fastgen_variant(f64, nx) is not None)


def test_every_variant_is_requested():
    """the set of valid (dtype, N, slab, pot, src, halves) -- every flag combination fastgen_variant accepts, the slab ones where a
    rank can keep an x slab (col_replicate_supported) -- is the set the matrix's cases request: a variant added to FastList32 / 64 and
    to fastgen_variant fails here until a case visits it"""
    valid, requested = set(), set()
    for dtype in gm.am.DTYPES:
        f64 = dtype == C128
        for nx in gm.am.COL_LENGTHS:
            for emit, n64, n32, pot, slab in all_flag_sets():
                v = emu_util.fastgen_variant(f64, nx, emit, n64, n32, pot, slab)
                if v is not None and (not v[0] or emu_util.col_replicate_supported(f64, nx, gm.NRANKS)):
                    valid.add((gm.dtype_name(dtype), nx) + v)
            for vid, shape in gm.cases(nx, dtype):
                if gm.class_of(vid, dtype, nx) != gm.EXACT:
                    emit, n64, n32, pot, slab = gm.VARIANTS[vid][3]
                    v = emu_util.fastgen_variant(f64, nx, emit, n64, n32, pot, slab)
                    assert v is not None, (vid, shape, gm.dtype_name(dtype))
                    requested.add((gm.dtype_name(dtype), nx) + v)
    assert valid == requested, (sorted(valid - requested), sorted(requested - valid))
    # ten float32 and six float64 list entries (rf_select.h FastList32 / FastList64), each at every length it has a kernel at
    assert len({v[2:] for v in valid if v[0] == "c64"}) == 10 and len({v[2:] for v in valid if v[0] == "c128"}) == 6


def test_every_launch_form_is_emitted():
    """every (FastKind, FastIo) step and every sequence form fastgen_sequence can emit is emitted by some case of the table, and the
    table's own statement of each case's form (generation_matrix.expected_form) is what the library plans"""
    steps, forms = set(), set()
    for dtype in gm.am.DTYPES:
        f64 = dtype == C128
        for nx in gm.am.COL_LENGTHS:
            for vid, shape in gm.cases(nx, dtype):
                if gm.class_of(vid, dtype, nx) == gm.EXACT:
                    continue
                for x0, x1, kz0, nzl in rank_ranges(vid, shape):
                    q = emu_util.fastgen_sequence_ex(*shape, f64=f64, x0=x0, x1=x1, kz0=kz0, nzl=nzl, **flags_of(vid))
                    assert q, (vid, shape, gm.dtype_name(dtype), "the library refuses the pass")
                    steps.update((s[0], s[1]) for s in q)
                    kinds = [(s[0], s[1]) for s in q]
                    split, side, ppi = gm.expected_form(shape, dtype, vid, kz0, gm.NRANKS if vid in gm.LONG_ONLY else 1)
                    body = kinds[1:] if kinds[0][0] == FIX_FILL else kinds
                    assert (kinds[0][0] == FIX_FILL) == side, (vid, shape, kinds)
                    assert (len(body) > 1 or body[0][1] != REPAIR) == split, (vid, shape, kinds)
                    assert (body[0][0] == COLPAIR) == (ppi > 0), (vid, shape, kinds)
                    if not split:
                        forms.add("unsplit")
                    elif kz0 != 0:
                        assert len(q) == 1 and q[0][1] == LEAN
                        forms.add("lean only, kz0 != 0")
                    elif ppi:
                        assert body[0] == (COLPAIR, FIRST) and q[-len(body)][3] == ppi and len(body) == (1 if ppi == 1 else 2)
                        forms.add("pairs, ppi = 1" if ppi == 1 else "pairs, ppi > 1")
                    else:
                        assert [b[1] for b in body] == [FIRST, LEAN]
                        forms.add("fix fill, first + lean" if side else "first + lean")
    assert forms == {"unsplit", "first + lean", "fix fill, first + lean", "pairs, ppi = 1", "pairs, ppi > 1", "lean only, kz0 != 0"}, forms
    one = (COL, COL2)
    assert steps == ({(FIX_FILL, REPAIR), (COLPAIR, FIRST), (COLPAIR, LEAN)} | {(k, io) for k in one for io in (LEAN, REPAIR, FIRST)}), sorted(steps)
