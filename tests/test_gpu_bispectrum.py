"""The binned bispectrum on the device (rf_measure_bispectrum, rf_bispectrum_release and the diagnostics rf_bispectrum_download_shell,
rf_bispectrum_set_max_workgroups, rf_bispectrum_geometry; rf_k_bispectrum.hip shell_filter_kernel / bispectrum_sum_kernel /
bispectrum_reduce_kernel) and Generator(backend='hip').measure_bispectrum -- run with -m gpu on an MI355X.

Oracle: tests/bispectrum_oracle.py, float64 numpy on the array the device itself was given.

Shapes: tiled (8, 8, 16) both dtypes (the smallest tiled grid: fewer cells than one chunk), (16, 16, 16), (16, 32, 64), (16, 16, 512)
(the padded potential pitch, long rows); generic (4, 6, 8) both dtypes, (6, 10, 14) (a ragged last chunk), (40, 60, 80).

a. Shell fields, downloaded with the diagnostic, against irfftn of the oracle's masked spectrum.  complex128: 1e-12 of the field's
largest value.  complex64: the float32 transform's rounding is relative to the field's largest value and no bound follows from the
formats, so the largest difference over the shells (data and unit runs, in units of each field's largest value) was measured once on
an MI355X against this oracle -- C64_MEASURED below, per shape: the largest of the data run, the unit run and, where test f. runs, the
runs with tables -- and is asserted at ten times that value, never looser than 1e-3.
b. The sums against the exact sum (math.fsum / np.longdouble) of the same terms over the DOWNLOADED device shell fields, within
4 cells 2^-53 sum|term|: this pins the reduction alone, free of the transforms' rounding, so the bound follows from the formats
(a float64 sum of `cells` terms in any order is within (cells - 1) 2^-53 sum|term| of the exact one).

The reduction's caps and where they are set (rf_k_bispectrum.hip bispectrum_launch_shape, rf_launch.h):

    what                      value                                                   reached here by
    LDS tile                  [nbins][chunk + 2] values in 40960 bytes, chunk a       5 bins complex64: 1984 cells; 32 bins: 256
                              multiple of 64 cells                                    (complex64), 128 (complex128)
    workgroups                min(chunks, 1024); rf_bispectrum_set_max_workgroups     set to 2 on (16, 32, 64): 17 chunks, 8 or 9 per
                                                                                      workgroup (the grid-stride loop)
    triples per workgroup     256 x 1, 2, 3 or 4 (<= 256, <= 512, <= 768, more)       35 and 364 triples: one tile; 680 (15 bins): three
                                                                                      per thread; 5984: six tiles of 1024 (blockIdx.y)
    cell groups               4, 2, 1 for <= 64, <= 128, more triples                 35 triples: four groups share a chunk's cells
    shell filter              min(row blocks, 4096) workgroups, the same setter       2 on (16, 32, 64): 64 row blocks per workgroup
"""
import numpy as np
import pytest

import bispectrum_oracle as bo
import power_oracle as po
from power_oracle import C64, C128

pytestmark = pytest.mark.gpu

SPACING = 2.5
SHAPES = [((8, 8, 16), C64), ((8, 8, 16), C128), ((16, 16, 16), C64), ((16, 32, 64), C64), ((16, 16, 512), C64),
          ((4, 6, 8), C64), ((4, 6, 8), C128), ((6, 10, 14), C64), ((40, 60, 80), C64)]
NBINS = 5
# largest difference of a complex64 shell field from the oracle's, in units of the field's largest value (see the module docstring)
C64_MEASURED = {(8, 8, 16): 1.872e-07, (16, 16, 16): 1.896e-07, (16, 32, 64): 2.098e-07, (16, 16, 512): 1.779e-07, (4, 6, 8): 1.123e-07,
                (6, 10, 14): 1.485e-07, (40, 60, 80): 2.149e-07}


@pytest.fixture(scope="module")
def hip():
    from randomfield_amd import _hip
    _hip.require_gpu()
    return _hip


def make_plan(hip, shape, dtype, kgrid=True):
    from randomfield_amd import powertools
    plan = hip.DevicePlan(*shape, dtype)
    if kgrid:
        plan.set_kgrid(*powertools.ksq_axes(*shape, SPACING))
    return plan


def edges_of(shape, nbins=NBINS):
    """linear edges from just below the fundamental mode of the longest axis to 0.9 of the Nyquist frequency: every shell is populated
    on every shape here, cells fall off both ends"""
    return np.linspace(0.9 * 2 * np.pi / (max(shape) * SPACING), 0.9 * np.pi / SPACING, nbins + 1)


def all_triples(nbins):
    from randomfield_amd import powertools
    return powertools.bispectrum_triples(np.arange(nbins + 1.0), "all")


def field_bound(shape, dtype):
    if dtype == C128:
        return 1e-12
    return min(10.0 * C64_MEASURED[shape], 1e-3)


def check_fields(plan, want, shape, dtype, what):
    """every shell field of the last call against the oracle's; returns the downloaded fields"""
    got = [plan.bispectrum_download_shell(b) for b in range(len(want))]
    worst = 0.0
    for b, (g, w) in enumerate(zip(got, want)):
        top = float(np.max(np.abs(w)))
        assert top > 0, "an empty shell tests nothing"
        worst = max(worst, float(np.max(np.abs(g.astype(np.float64) - w))) / top)
    print("%s %s %s: shell fields differ by at most %.3e of their largest value" % (what, shape, po.ids(dtype), worst))
    assert worst <= field_bound(shape, dtype), what
    return got


def check_sums(got, fields, triples, what):
    want, absum = bo.triple_sums(fields, triples)
    bound = bo.reduction_bound(fields[0].size, absum)
    diff = np.abs(got - want)
    print("%s: %d triples over %d cells, worst difference %.3f of the bound" % (what, len(triples), fields[0].size, float(np.max(diff / np.maximum(bound, 1e-300)))))
    assert np.all(diff <= bound), what


@pytest.mark.parametrize("shape,dtype", SHAPES, ids=po.ids)
def test_shell_fields_and_sums(hip, shape, dtype):
    """a. and b. on every shape, data and unit runs; two calls give the same bits"""
    plan = make_plan(hip, shape, dtype)
    src = po.spectrum(shape, dtype)
    plan.upload_k(src)
    edges, triples = edges_of(shape), all_triples(NBINS)
    for unit in (False, True):
        got = plan.measure_bispectrum(edges, triples, unit=unit)
        assert plan.elapsed_ms() > 0
        fields = check_fields(plan, bo.shell_fields(src, shape, SPACING, edges, unit=unit), shape, dtype, "unit" if unit else "data")
        check_sums(got, fields, triples, "%s %s %s" % ("unit" if unit else "data", shape, po.ids(dtype)))
        assert np.array_equal(plan.measure_bispectrum(edges, triples, unit=unit), got), "two calls differ"
        if unit:
            n = float(np.prod(shape))
            counts = np.rint(n * n * got)
            assert np.all(counts >= 0) and counts.sum() > 0
    assert np.array_equal(plan.download_k(), src), "the k buffer changed"
    plan.close()


@pytest.mark.parametrize("dtype", [C64, C128], ids=po.ids)
@pytest.mark.parametrize("nbins,ntriples", [(12, 364), (15, 680), (32, 5984)])
def test_sums_of_many_triples(hip, nbins, ntriples, dtype):
    """b. with the host test's bin and triple counts at (8, 8, 16): one tile of triples with two per thread, six tiles with four; and
    15 bins, whose 680 triples take three per thread"""
    shape = (8, 8, 16)
    plan = make_plan(hip, shape, dtype)
    plan.upload_k(po.spectrum(shape, dtype))
    k_min, k_max = 0.9 * 2 * np.pi / (16 * SPACING), np.sqrt(3.0) * np.pi / SPACING
    edges, triples = np.linspace(k_min, k_max, nbins + 1), all_triples(nbins)
    assert len(triples) == ntriples
    got = plan.measure_bispectrum(edges, triples)
    fields = [plan.bispectrum_download_shell(b) for b in range(nbins)]
    assert sum(1 for f in fields if np.any(f != 0)) >= nbins // 2
    check_sums(got, fields, triples, "%d bins %s" % (nbins, po.ids(dtype)))
    dup = plan.measure_bispectrum(edges, np.concatenate([triples[-2:], triples[-2:]]))
    assert np.array_equal(dup[:2], dup[2:]), "duplicates are allowed and give the same bits"
    plan.close()


def test_sums_with_two_workgroups(hip):
    """b. again with the workgroup cap at 2 on (16, 32, 64): every workgroup takes several chunks, every filter workgroup many rows"""
    shape, dtype = (16, 32, 64), C64
    plan = make_plan(hip, shape, dtype)
    src = po.spectrum(shape, dtype)
    plan.upload_k(src)
    edges, triples = edges_of(shape), all_triples(NBINS)
    free = plan.measure_bispectrum(edges, triples)
    chunk, wgs, rows = plan.bispectrum_geometry(NBINS, len(triples))
    assert chunk == 1984 and wgs == -(-int(np.prod(shape)) // chunk) == 17 and rows == 4 * wgs
    plan.bispectrum_set_max_workgroups(2)
    assert plan.bispectrum_geometry(NBINS, len(triples)) == (chunk, 2, 8)
    got = plan.measure_bispectrum(edges, triples)
    fields = check_fields(plan, bo.shell_fields(src, shape, SPACING, edges), shape, dtype, "two workgroups")
    check_sums(got, fields, triples, "two workgroups")
    check_sums(free, fields, triples, "default cap")          # (the same fields: the filter and the transforms do not depend on the cap)
    plan.bispectrum_set_max_workgroups(0)
    assert np.array_equal(plan.measure_bispectrum(edges, triples), free)
    with pytest.raises(RuntimeError, match="workgroup cap"):
        plan.bispectrum_set_max_workgroups(-1)
    plan.close()


def lazy_bytes(plan, shape, dtype, nbins, ntriples):
    """the documented lazy memory of a call: a masked half spectrum, nbins shell fields, tables and per-workgroup partials"""
    nx, ny, nz = shape
    csize = 8 if dtype == C64 else 16
    rows = plan.bispectrum_geometry(nbins, ntriples)[2]
    return nx * ny * (nz // 2 + 1) * csize + nbins * nx * ny * nz * (csize // 2) + 8 * (12321 + nx + ny + nz // 2 + 1 + rows * ntriples)


@pytest.mark.parametrize("shape,dtype", [((8, 8, 16), C64), ((6, 10, 14), C64), ((16, 16, 16), C128)], ids=po.ids)
def test_reproducible_and_memory(hip, shape, dtype):
    """c. two calls and a call after the release give the same bits; rf_plan_nbytes grows by the documented amount and comes back"""
    plan = make_plan(hip, shape, dtype)
    src = po.spectrum(shape, dtype)
    plan.upload_k(src)
    plan.execute_c2r()                        # (the transforms' own lazy scratch exists before the baseline is read)
    before = plan.nbytes
    edges, triples = edges_of(shape), all_triples(NBINS)
    with pytest.raises(RuntimeError, match="no shell fields"):
        plan.bispectrum_download_shell(0)
    first = plan.measure_bispectrum(edges, triples)
    assert plan.nbytes == before + lazy_bytes(plan, shape, dtype, NBINS, len(triples))
    assert np.array_equal(plan.measure_bispectrum(edges, triples), first)
    with pytest.raises(RuntimeError, match="last call's bins"):
        plan.bispectrum_download_shell(NBINS)
    plan.bispectrum_release()
    assert plan.nbytes == before
    with pytest.raises(RuntimeError, match="no shell fields"):
        plan.bispectrum_download_shell(0)
    assert np.array_equal(plan.measure_bispectrum(edges, triples), first)
    plan.bispectrum_release()
    plan.bispectrum_release()                 # (nothing to free: not an error)
    assert plan.nbytes == before
    plan.close()


@pytest.mark.parametrize("shape,dtype", [((16, 16, 16), C64), ((6, 10, 14), C128)], ids=po.ids)
def test_state_is_untouched(hip, shape, dtype):
    """d. K and the stash bit for bit, no real-space field afterwards, rf_measure_power(FROM_KSPACE) the same bits before and after"""
    import interlace_oracle as orc
    plan = make_plan(hip, shape, dtype)
    stashed, src = po.spectrum(shape, dtype, seed=5), po.spectrum(shape, dtype)
    plan.upload_k(stashed)
    plan.kspace_stash()
    plan.upload_k(src)
    plan.execute_c2r()
    assert plan.download_real().shape == shape
    edges = edges_of(shape)
    power = plan.measure_power(edges, hip.RF_POWER_FROM_KSPACE)
    plan.measure_bispectrum(edges, all_triples(NBINS))
    assert np.array_equal(plan.download_k(), src)
    with pytest.raises(RuntimeError, match="no real-space field"):
        plan.download_real()
    again = plan.measure_power(edges, hip.RF_POWER_FROM_KSPACE)
    assert all(np.array_equal(a, b) for a, b in zip(power, again))
    plan.kspace_interlace(None)               # K <- (S + K) / 2: the stash is what was put aside
    assert np.array_equal(plan.download_k(), orc.combine(stashed, src, None))
    plan.close()


def test_refusals_allocate_nothing(hip):
    """e. every refusal leaves rf_plan_nbytes as it was"""
    shape = (16, 16, 16)
    edges, triples = edges_of(shape), all_triples(NBINS)
    plan = make_plan(hip, shape, C64)
    before = plan.nbytes
    with pytest.raises(RuntimeError, match="no k-space data"):
        plan.measure_bispectrum(edges, triples)
    assert plan.nbytes == before
    plan.upload_k(po.spectrum(shape, C64))
    before = plan.nbytes
    bad_tab = np.ones(16)
    bad_tab[3] = 0.0
    nan_tab = np.ones(9)
    nan_tab[8] = np.nan
    cases = [("increasing", dict(edges=[0.1, 0.3, 0.3, 0.5], triples=[(0, 1, 2)])),
             ("negative", dict(edges=[-0.1, 0.3], triples=[(0, 0, 0)])),
             ("nbins", dict(edges=np.linspace(0.1, 1.0, 34), triples=[(0, 0, 0)])),
             ("nbins", dict(edges=[0.3], triples=[(0, 0, 0)])),
             ("ntriples", dict(edges=edges, triples=np.zeros((0, 3), np.intc))),
             ("ntriples", dict(edges=edges, triples=np.zeros((8193, 3), np.intc))),
             ("bad triple", dict(edges=edges, triples=[(0, 1, NBINS)])),
             ("bad triple", dict(edges=edges, triples=[(1, 0, 2)])),
             ("bad triple", dict(edges=edges, triples=[(-1, 0, 2)])),
             ("amplitude table", dict(edges=edges, triples=triples, amp=(bad_tab, None, None))),
             ("amplitude table", dict(edges=edges, triples=triples, amp=(None, None, nan_tab)))]
    for match, kw in cases:
        with pytest.raises(RuntimeError, match=match):
            plan.measure_bispectrum(kw["edges"], kw["triples"], kw.get("amp"))
        assert plan.nbytes == before, match
    with pytest.raises(RuntimeError, match="no shell fields"):
        plan.bispectrum_download_shell(0)
    plan.close()
    nogrid = make_plan(hip, shape, C64, kgrid=False)
    nogrid.upload_k(po.spectrum(shape, C64))
    before = nogrid.nbytes
    with pytest.raises(RuntimeError, match="rf_set_kgrid"):
        nogrid.measure_bispectrum(edges, triples)
    assert nogrid.nbytes == before
    nogrid.close()
    ranked = hip.DevicePlan(*shape, C64, nranks=2, rank=0)
    before = ranked.nbytes
    with pytest.raises(RuntimeError, match="single-rank"):
        ranked.measure_bispectrum(edges, triples)
    with pytest.raises(RuntimeError, match="single-rank"):
        ranked.bispectrum_release()
    assert ranked.nbytes == before
    ranked.close()
    c2c = hip.DevicePlan(*shape, C64, unpacked=True)
    before = c2c.nbytes
    with pytest.raises(RuntimeError, match="c2c"):
        c2c.measure_bispectrum(edges, triples)
    assert c2c.nbytes == before
    c2c.close()


@pytest.mark.parametrize("shape,dtype", [((16, 16, 16), C64), ((4, 6, 8), C128), ((40, 60, 80), C64)], ids=po.ids)
def test_amplitude_tables(hip, shape, dtype):
    """f. the tables against the oracle with the same tables; the unit run ignores them bit for bit"""
    plan = make_plan(hip, shape, dtype)
    src = po.spectrum(shape, dtype)
    plan.upload_k(src)
    edges, triples = edges_of(shape), all_triples(NBINS)
    amp = bo.symmetric_tables(shape)
    for tabs in (amp, (amp[0], None, amp[2])):
        got = plan.measure_bispectrum(edges, triples, tabs)
        fields = check_fields(plan, bo.shell_fields(src, shape, SPACING, edges, tabs), shape, dtype, "tables")
        check_sums(got, fields, triples, "tables %s" % (shape,))
    plain = plan.measure_bispectrum(edges, triples, unit=True)
    bad = [np.full_like(t, -1.0) for t in amp]                 # (not even checked in a unit run)
    assert np.array_equal(plan.measure_bispectrum(edges, triples, amp, unit=True), plain)
    assert np.array_equal(plan.measure_bispectrum(edges, triples, bad, unit=True), plain)
    plan.close()


# ---- g. Generator(backend='hip') --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,rtol", [(C128, 1e-9), (C64, 1e-4)], ids=po.ids)
def test_generator_plane_waves(hip, dtype, rtol):
    """the host test's three plane waves, all three cases (n_perm = 1, 2, 6).  1e-9 of the closed form in float64; 1e-4 in float32
    (the transforms are held to 1e-5 rms of the field by tests/axis_matrix.py; three factors and two transforms)"""
    from randomfield_amd import Generator
    from test_bispectrum_host import WAVE_AMPS, WAVE_CASES, WAVE_MODES, WAVE_PHASES, WAVE_SHAPE, check_waves, kf
    rt = np.float32 if dtype == C64 else np.float64
    field = bo.plane_waves(WAVE_SHAPE, WAVE_MODES, WAVE_AMPS, WAVE_PHASES).astype(rt)
    gen = Generator(*WAVE_SHAPE, SPACING, backend="hip", rng="native", dtype=dtype)
    n = float(np.prod(WAVE_SHAPE))
    for edges, holder, nperm in WAVE_CASES:
        res = gen.measure_bispectrum(field, k_edges=np.array(edges) * kf(8), triangles="all")
        ok = res["ntriangles"] > 0
        assert np.all(np.isnan(res["B"][~ok])) and np.all(np.isnan(res["Q"][~ok]))
        n2s = np.where(ok, res["B"] * res["ntriangles"] * n / SPACING ** 6, 0.0)
        check_waves(n2s, res["bins"], holder, nperm, rtol, "hip backend")
    with pytest.raises(RuntimeError, match="no real-space field"):
        gen._backend.dev.download_real()


def test_generator_triangle_counts(hip):
    """'ntriangles' is the explicit oracle's integer, triple by triple, at (8, 8, 16); 'k' and 'Q' are measure_power_spectrum's"""
    from randomfield_amd import Generator, powertools
    shape = (8, 8, 16)
    gen = Generator(*shape, SPACING, backend="hip", rng="native", dtype=C64)
    field = np.random.RandomState(2).normal(size=shape).astype(np.float32)
    edges = powertools.default_bispectrum_edges(shape, SPACING, 4)
    res = gen.measure_bispectrum(field, k_edges=edges, triangles="all")
    counts = bo.explicit_oracle(None, shape, SPACING, edges, res["bins"], unit=True)[1]
    assert res["ntriangles"].dtype == np.float64 and np.array_equal(res["ntriangles"], counts.astype(np.float64)) and counts.sum() > 0
    closed = gen.measure_bispectrum(field, k_edges=edges)              # 'closed': the second field costs one run, the counts are kept
    assert np.all(closed["ntriangles"] > 0) and len(closed) == int((counts > 0).sum())
    keep = counts > 0
    assert np.array_equal(closed["B"], res["B"][keep]) and np.array_equal(closed["ntriangles"], res["ntriangles"][keep])
    power = gen.measure_power_spectrum(field, k_edges=edges)
    assert np.array_equal(closed["k1"], power["k"][closed["bins"][:, 0]]) and np.array_equal(closed["k3"], power["k"][closed["bins"][:, 2]])
    p = [power["Pk"][closed["bins"][:, i]] for i in range(3)]
    assert np.array_equal(closed["Q"], closed["B"] / (p[0] * p[1] + p[1] * p[2] + p[2] * p[0]))
    # against the FFT oracle on the float64 spectrum of the same field: 1e-3 of the largest |B| (the float32 transforms' rounding is
    # relative to the largest amplitude; a plumbing error shows as >= 1e-1)
    want = powertools.bin_bispectrum(np.fft.rfftn(field.astype(np.float64)), SPACING, edges, closed["bins"])
    unit = powertools.bin_bispectrum(np.fft.rfftn(field.astype(np.float64)), SPACING, edges, closed["bins"], unit=True)
    wantB = SPACING ** 6 / float(np.prod(shape)) * want / unit
    err = np.max(np.abs(closed["B"] - wantB)) / np.max(np.abs(wantB))
    print("Generator B against numpy: %.3e of the largest" % err)
    assert err <= 1e-3


def test_generator_kspace_source_leaves_the_spectrum(hip):
    """measure_bispectrum(source='kspace', window='cic') after an interlaced paint: measure_power_spectrum(source='kspace') still
    works and gives the same bits"""
    from randomfield_amd import Generator, powertools
    shape = (16, 16, 16)
    gen = Generator(*shape, SPACING, backend="hip", rng="native", dtype=C64)
    s = (0.6 * SPACING * np.random.RandomState(8).normal(size=(3,) + shape)).astype(np.float32)
    gen.set_particle_displacements(s)
    with pytest.raises(RuntimeError, match="interlaced"):
        gen.measure_bispectrum(source="kspace")
    gen.paint_particles(interlaced=True, download=False)
    pedges = powertools.default_k_edges(shape, SPACING, 6)
    before = gen.measure_power_spectrum(source="kspace", window="cic", k_edges=pedges)
    edges = powertools.default_bispectrum_edges(shape, SPACING, 4)       # (shells a fundamental mode wide: every closed triple holds a triangle)
    res = gen.measure_bispectrum(source="kspace", window="cic", k_edges=edges)
    assert len(res) > 0 and np.all(res["ntriangles"] > 0) and np.all(np.isfinite(res["B"])) and np.all(np.isfinite(res["Q"]))
    after = gen.measure_power_spectrum(source="kspace", window="cic", k_edges=pedges)
    for name in ("k", "Pk", "nmodes"):
        assert np.array_equal(before[name], after[name])
    plain = gen.measure_bispectrum(source="kspace", k_edges=edges)
    assert not np.array_equal(plain["B"], res["B"]) and np.array_equal(plain["ntriangles"], res["ntriangles"])
    with pytest.raises(ValueError, match="field"):
        gen.measure_bispectrum(s[0], source="kspace")
    gen.measure_bispectrum(s[0])                                       # a measurement of a field: the interlaced spectrum is gone
    with pytest.raises(RuntimeError, match="interlaced"):
        gen.measure_bispectrum(source="kspace")
