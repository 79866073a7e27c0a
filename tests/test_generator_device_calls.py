"""The device calls behind every public method of ``Generator(backend='hip')``, pinned as text: no GPU, no library.

``_hip.DevicePlan`` is replaced by the recording stand-in of tests/recording_plan.py; one fixed script of Generator calls (refused
ones included: the exception's type and text enter the trace) runs for the cross product of rng x dtype x save_potential x
store_potential x download x the answers the Generator branches on, on a tiled 16^3 grid and on (10, 6, 12), which is not tiled
(such a plan arms no sink and serves no reference batch, so those two answers are not varied there).  After every Generator call the
state a caller can see is recorded too.  The expected traces are in tests/generator_device_calls.txt, written from the tree before
the Generator's backends were split (``python tests/test_generator_device_calls.py --write`` regenerates it): one line per distinct
text (the device calls and refusal of one Generator call; the state after it), the distinct sequences of their numbers over the
script, and per case the number of its sequence.

The failed-realisation cases at the end are literals: they pin that a host sink armed by a call that raises is disarmed."""
import itertools
import os
import sys

import numpy as np
import pytest

import recording_plan

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "generator_device_calls.txt")
SHAPES = [(16, 16, 16), (10, 6, 12)]
RNGS = ["reference", "native"]
DTYPES = [np.complex64, np.complex128]
BOOL = (True, False)


def make_generator(shape, log, **kwargs):
    from randomfield_amd import Generator
    nz = shape[2]
    tables = dict(growth_function=np.linspace(1.0, 0.5, nz), mean_matter_density=np.linspace(0.9, 1.1, nz),
                  redshifts=np.linspace(0.0, 1.0, nz), transverse_distance=np.arange(nz) * 2.5)
    tables.update(kwargs)
    return Generator(*shape, 2.5, num_plot_sections=2, backend="hip", **tables)


class Trace(object):
    """the log cut into one (calls, state) pair per Generator call: the device calls and a refusal (!) as one line of text, and what a
    caller can see afterwards; and the calls' labels"""

    def __init__(self, log):
        self.log, self.blocks, self.labels, self.gen = log, [], ["Generator"], None

    def cut(self):
        g = self.gen
        state = "potential=%s rms=%s dropped=%r on_host=%r" % (type(g.potential).__name__, recording_plan.text(g.delta_field_rms),
                                                               g.particles_dropped, g._field_on_host)
        self.blocks.append((" ; ".join(self.log), state))
        del self.log[:]

    def step(self, label, fn):
        self.labels.append(label)
        try:
            fn(self.gen)
        except Exception as exc:          # (the type and text of a refusal are part of the trace)
            self.log.append("! %s: %s" % (type(exc).__name__, " ".join(str(exc).split())))
        self.cut()


def run_script(shape, rng, dtype, save_potential, store_potential, download, monkeypatch, answers):
    log = []
    recording_plan.install(monkeypatch, log, answers)
    t = Trace(log)
    t.gen = make_generator(shape, log, rng=rng, dtype=dtype, store_potential=store_potential)
    t.cut()
    nz = shape[2]
    zeros = np.zeros(shape)
    sp, dl = save_potential, download
    s = t.step
    s("generate_delta_field(seed=3)", lambda g: g.generate_delta_field(seed=3, save_potential=sp, download=dl))
    s("generate_density_field(seed=4)", lambda g: g.generate_density_field(seed=4, download=dl))
    s("generate_delta_field(seed=3) again", lambda g: g.generate_delta_field(seed=3, save_potential=sp, download=dl))
    s("generate_delta_field(smoothing)", lambda g: g.generate_delta_field(2.0, seed=6, save_potential=sp, download=dl))
    s("generate_delta_field(show_plot)", lambda g: g.generate_delta_field(seed=3, show_plot=True))
    s("download_field", lambda g: g.download_field())
    s("download_field again", lambda g: g.download_field())
    s("measure_power_spectrum(kspace) refused", lambda g: g.measure_power_spectrum(source="kspace"))
    s("measure_power_spectrum(source) refused", lambda g: g.measure_power_spectrum(source="k"))
    s("measure_power_spectrum(nbins=4)", lambda g: g.measure_power_spectrum(nbins=4))
    s("measure_power_spectrum(field, cic)", lambda g: g.measure_power_spectrum(zeros, nbins=3, window="cic"))
    s("measure_power_spectrum(field shape) refused", lambda g: g.measure_power_spectrum(zeros[1:]))
    s("measure_power_multipoles(los=0, tsc)", lambda g: g.measure_power_multipoles(los=0, k_edges=[0.1, 0.2, 0.4], window="tsc"))
    s("measure_power_multipoles(los=3) refused", lambda g: g.measure_power_multipoles(los=3))
    s("convert_delta_to_density(lognormal)", lambda g: g.convert_delta_to_density(download=dl))
    s("convert_delta_to_density(linear)", lambda g: g.convert_delta_to_density(apply_lognormal_transform=False, download=dl))
    s("calculate_newtonian_potential(light cone)", lambda g: g.calculate_newtonian_potential(scale=-1.5, download=dl))
    s("calculate_newtonian_potential(flat)", lambda g: g.calculate_newtonian_potential(light_cone=False, scale=2.0, download=dl))
    s("calculate_newtonian_potential(no scale) refused", lambda g: g.calculate_newtonian_potential())
    s("device deviates replaced", lambda g: g.plan_c2r.device.reference_noise(9))
    s("calculate_newtonian_potential after that", lambda g: g.calculate_newtonian_potential(scale=1.0, download=dl))
    s("device power replaced", lambda g: g.plan_c2r.device.set_power(np.zeros(2), np.ones(2)))
    s("calculate_displacement_field after that", lambda g: g.calculate_displacement_field(0, download=dl))
    s("potential.download after that", lambda g: g.potential.download())
    s("generate_delta_field(seed=3) once more", lambda g: g.generate_delta_field(seed=3, save_potential=sp, download=dl))
    s("calculate_newtonian_potential of the new field", lambda g: g.calculate_newtonian_potential(scale=-1.5, download=dl))
    s("calculate_lensing_potential", lambda g: g.calculate_lensing_potential())
    s("calculate_lensing_potential(i_min) refused", lambda g: g.calculate_lensing_potential(i_min=nz))
    s("calculate_displacement_field(0)", lambda g: g.calculate_displacement_field(0, download=dl))
    s("calculate_displacement_field('y', light_cone)", lambda g: g.calculate_displacement_field("y", light_cone=True, scale=0.5, download=dl))
    s("calculate_displacement_field(2, order=2, factor_z)",
      lambda g: g.calculate_displacement_field(2, order=2, factor_z=np.linspace(1, 2, nz), download=dl))
    s("calculate_displacement_field(1, order=2, light_cone)", lambda g: g.calculate_displacement_field(1, True, order=2, download=dl))
    s("calculate_displacement_field(3) refused", lambda g: g.calculate_displacement_field(3))
    s("calculate_displacement_field('w') refused", lambda g: g.calculate_displacement_field("w"))
    s("calculate_displacement_field(order=3) refused", lambda g: g.calculate_displacement_field(0, order=3))
    s("lpt2_source", lambda g: g.lpt2_source(download=dl))
    s("calculate_displacement_field(0, order=2) after the source", lambda g: g.calculate_displacement_field(0, order=2, download=dl))
    s("potential.download", lambda g: g.potential.download())
    s("paint_particles refused", lambda g: g.paint_particles())
    s("interpolate_at_particles refused", lambda g: g.interpolate_at_particles())
    s("shift_particles refused", lambda g: g.shift_particles(0))
    s("particle_positions refused", lambda g: g.particle_positions())
    s("particle_displacements(order=3) refused", lambda g: g.particle_displacements(order=3))
    s("particle_displacements(rsd_axis=5) refused", lambda g: g.particle_displacements(rsd_axis=5))
    s("particle_displacements(order=2, rsd)", lambda g: g.particle_displacements(order=2, D1=0.5, download=dl, rsd_axis=2, f1=0.5))
    s("particle_displacements(order=1)", lambda g: g.particle_displacements(order=1, download=dl, rsd_axis=0, f1=0.5, f2=0.25))
    s("set_particle_displacements(shape) refused", lambda g: g.set_particle_displacements(zeros))
    s("set_particle_displacements", lambda g: g.set_particle_displacements(np.zeros((3,) + shape)))
    s("shift_particles(no gather) refused", lambda g: g.shift_particles(0))
    s("paint_particles(assignment) refused", lambda g: g.paint_particles(assignment="ngp"))
    s("paint_particles", lambda g: g.paint_particles(download=dl))
    s("paint_particles(tsc, interlaced)", lambda g: g.paint_particles(download=dl, assignment="tsc", interlaced=True))
    s("measure_power_spectrum(kspace)", lambda g: g.measure_power_spectrum(nbins=4, source="kspace"))
    s("measure_power_spectrum(kspace, field) refused", lambda g: g.measure_power_spectrum(zeros, source="kspace"))
    s("measure_power_multipoles(kspace)", lambda g: g.measure_power_multipoles(los=1, nbins=4, window="tsc", source="kspace"))
    s("measure_power_multipoles(field)", lambda g: g.measure_power_multipoles(nbins=4))
    s("measure_power_multipoles(kspace) refused", lambda g: g.measure_power_multipoles(source="kspace"))
    s("interpolate_at_particles(slot=1, tsc)",
      lambda g: g.interpolate_at_particles(slot=1, coeff=2.0, first=False, download=dl, assignment="tsc"))
    s("interpolate_at_particles(field)", lambda g: g.interpolate_at_particles(zeros, download=dl))
    s("interpolate_at_particles(slot=5) refused", lambda g: g.interpolate_at_particles(slot=5))
    s("shift_particles(1)", lambda g: g.shift_particles(1, coeff=0.5))
    s("shift_particles(0, slot=1)", lambda g: g.shift_particles(0, slot=1))
    s("shift_particles(axis=4) refused", lambda g: g.shift_particles(4))
    s("shift_particles(slot=4) refused", lambda g: g.shift_particles(0, slot=4))
    s("particle_positions", lambda g: g.particle_positions())
    s("paint_particles(interlaced) before a new field", lambda g: g.paint_particles(download=dl, interlaced=True))
    s("calculate_newtonian_potential replaces the spectrum", lambda g: g.calculate_newtonian_potential(scale=1.0, download=dl))
    s("measure_power_spectrum(kspace) after it refused", lambda g: g.measure_power_spectrum(source="kspace"))
    s("generate_density_field(seed=8)", lambda g: g.generate_density_field(1.0, seed=8, download=dl))
    s("paint_particles after a new field refused", lambda g: g.paint_particles())
    s("shift_particles after a new field refused", lambda g: g.shift_particles(0))
    s("calculate_newtonian_potential after a density field refused", lambda g: g.calculate_newtonian_potential(scale=1.0))
    s("plot_slice refused", lambda g: g.plot_slice())
    return t.blocks, t.labels


def cases(shape):
    """(key, keyword arguments of run_script) of every case of one shape"""
    tiled = shape == SHAPES[0]
    for rng, dtype, sp, store, dl, arm, delivered, batch, regen in itertools.product(
            RNGS, DTYPES, BOOL, BOOL, BOOL, BOOL if tiled else (True,), BOOL if tiled else (True,), BOOL if tiled else (True,), BOOL):
        key = "%dx%dx%d %s %s save=%d store=%d download=%d arm=%d delivered=%d batch=%d regenerate=%d" % (
            shape + (rng, np.dtype(dtype).name, sp, store, dl, arm, delivered, batch, regen))
        answers = dict(recording_plan.ANSWERS, arm_host_sink=arm, host_sink_delivered=delivered, can_batch_reference=batch,
                       can_regenerate_potential=regen)
        yield key, dict(shape=shape, rng=rng, dtype=dtype, save_potential=sp, store_potential=store, download=dl, answers=answers)


def group_of(kw):
    return "%dx%dx%d %s %s" % (kw["shape"] + (kw["rng"], np.dtype(kw["dtype"]).name))


def read_fixture():
    """(sequences, groups): ``calls`` and ``state`` lines are the distinct texts of :class:`Trace`, ``seq`` lines the distinct sequences
    of calls/state numbers (one pair per Generator call of the script), ``cases`` lines the sequence number of every case of a
    (shape, rng, dtype) group in the order of :func:`cases`"""
    tables, groups = {"calls": [], "state": [], "seq": []}, {}
    with open(FIXTURE) as f:
        for line in f.read().split("\n"):
            head, _, rest = line.partition(": ")
            kind, _, name = head.partition(" ")
            if kind in tables:
                assert int(name) == len(tables[kind])
                tables[kind].append(rest)
            elif kind == "cases":
                groups[name] = [int(i) for i in rest.split()]
    sequences = [[(tables["calls"][int(c)], tables["state"][int(s)]) for c, s in (pair.split("/") for pair in seq.split())]
                 for seq in tables["seq"]]
    return sequences, groups


@pytest.fixture(scope="module")
def expected():
    return read_fixture()


@pytest.mark.parametrize("rng", RNGS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["complex64", "complex128"])
@pytest.mark.parametrize("shape", SHAPES, ids=["16x16x16", "10x6x12"])
def test_device_calls_are_those_of_the_fixture(shape, dtype, rng, expected, monkeypatch):
    sequences, groups = expected
    mine = [(key, kw) for key, kw in cases(shape) if kw["rng"] == rng and kw["dtype"] == dtype]
    numbers = groups[group_of(mine[0][1])]
    assert len(mine) == len(numbers) == (128 if shape == SHAPES[0] else 16)
    for (key, kw), number in zip(mine, numbers):
        got, labels = run_script(monkeypatch=monkeypatch, **kw)
        want = sequences[number]
        for n, (g, w) in enumerate(zip(got, want)):
            assert g == w, "%s, Generator call %d (%s)" % (key, n, labels[n])
        assert len(got) == len(want), key


def test_fixture_holds_these_groups_and_no_others(expected):
    assert sorted(expected[1]) == sorted(set(group_of(kw) for shape in SHAPES for _, kw in cases(shape)))


def test_first_traces_of_the_default_plan(monkeypatch):
    """the two traces the refactor's issue quotes: complex64, rng='reference', 16^3"""
    log = []
    recording_plan.install(monkeypatch, log, dict(recording_plan.ANSWERS))
    gen = make_generator(SHAPES[0], log)
    del log[:]
    gen.generate_delta_field(seed=3)
    assert [line.split("(")[0] for line in log] == ["set_power", "arm_host_sink", "can_batch_reference", "realise_batch_reference",
                                                    "can_regenerate_potential", "moments", "host_sink_delivered"]
    assert log[3] == "realise_batch_reference([3], want_rms=False)" and log[4] == "can_regenerate_potential('resident')"
    del log[:]
    gen.generate_density_field(seed=4)
    assert [line.split("(")[0] for line in log][:4] == ["set_power", "set_z_tables", "reference_noise", "realise_lognormal"]
    assert log[2] == "reference_noise(4, single=True)" and log[3] == "realise_lognormal(0, 'resident')"


def test_dropped_generator_frees_its_plan_without_the_collector(monkeypatch):
    """a Generator that saved no potential is part of no reference cycle: dropping it releases the device plan (and its device
    memory) at once, not whenever the cyclic collector runs -- in the middle of somebody's timed loop"""
    import gc
    import weakref
    recording_plan.install(monkeypatch, [], dict(recording_plan.ANSWERS))
    gen = make_generator(SHAPES[0], [], rng="native")
    gen.generate_delta_field(seed=3, save_potential=False, download=False)
    plan = weakref.ref(gen.plan_c2r.device)
    gc.disable()
    try:
        del gen
        assert plan() is None
    finally:
        gc.enable()


# ---- a realisation that raises: the armed sink is disarmed ----------------------------------------------------------------------
@pytest.mark.parametrize("rng,dtype,store,failing,first", [
    ("native", np.complex64, False, "realise", ["can_regenerate_potential(None)", "realise(3, None)"]),
    ("native", np.complex64, True, "realise_potential", ["realise_potential(3, None)"]),
    ("reference", np.complex128, False, "reference_noise", ["reference_noise(3, single=False)"]),
    ("reference", np.complex64, False, "realise_batch_reference", ["can_batch_reference()", "realise_batch_reference([3], want_rms=False)"]),
])
def test_failed_realisation_disarms_the_sink(rng, dtype, store, failing, first, monkeypatch):
    log, raising = [], set()
    recording_plan.install(monkeypatch, log, dict(recording_plan.ANSWERS), raising)
    gen = make_generator(SHAPES[0], log, rng=rng, dtype=dtype, store_potential=store)
    gen.generate_delta_field(seed=1, download=False)
    del log[:]
    raising.add(failing)
    with pytest.raises(RuntimeError, match="stand-in: %s failed" % failing):
        gen.generate_delta_field(seed=3)
    rtype = "float32" if dtype == np.complex64 else "float64"
    assert log[0].startswith("set_power(") and log[0].endswith("if_changed=True)")
    assert log[1:] == ["arm_host_sink(%s(16, 16, 18), padded=True)" % rtype] + first + ["host_sink_delivered()"]
    raising.clear()
    del log[:]
    # the next call that keeps its field on the device arms nothing, and the native generator replays its captured graph again
    assert gen.generate_delta_field(seed=3, save_potential=False, download=False) is None and not gen._field_on_host
    assert not [line for line in log if line.startswith(("arm_host_sink", "host_sink_delivered"))]
    assert ("realise_batch(uint64(1,), want_rms=False)" in log) == (rng == "native")


def test_failed_graph_replay_leaves_nothing_armed(monkeypatch):
    """download=False arms nothing: a raising realise_batch ends the trace, no sink call before or after"""
    log, raising = [], {"realise_batch"}
    recording_plan.install(monkeypatch, log, dict(recording_plan.ANSWERS), raising)
    gen = make_generator(SHAPES[0], log, rng="native")
    del log[:]
    with pytest.raises(RuntimeError, match="stand-in: realise_batch failed"):
        gen.generate_delta_field(seed=3, save_potential=False, download=False)
    assert [line.split("(")[0] for line in log] == ["set_power", "realise_batch"]


def write_fixture():
    def number(table, item):
        return table.setdefault(item, len(table))

    calls, states, sequences, groups = {}, {}, {}, {}
    for shape in SHAPES:
        for key, kw in cases(shape):
            with pytest.MonkeyPatch.context() as mp:
                got, _ = run_script(monkeypatch=mp, **kw)
            ids = " ".join("%d/%d" % (number(calls, c), number(states, s)) for c, s in got)
            groups.setdefault(group_of(kw), []).append(number(sequences, ids))
    with open(FIXTURE, "w") as f:
        for table, kind in ((calls, "calls"), (states, "state"), (sequences, "seq")):
            for item, n in table.items():
                f.write("%s %d: %s\n" % (kind, n, item))
        for group, numbers in groups.items():
            f.write("cases %s: %s\n" % (group, " ".join(str(n) for n in numbers)))
    print("%d cases, %d distinct sequences, %d calls and %d state lines" % (sum(len(v) for v in groups.values()), len(sequences), len(calls), len(states)))


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1:] == ["--write"]:
        write_fixture()
