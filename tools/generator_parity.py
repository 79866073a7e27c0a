#!/usr/bin/env python3
"""Does a tree's ``Generator`` compute what another tree's does, call by call, through the public API?

    python tools/generator_parity.py --backend numpy|hip > digests.txt

Runs one fixed script of Generator calls -- every public method, every keyword of the particle and measurement calls, the refused
calls too -- on 16^3 and (10, 6, 12) with ``num_plot_sections=2``, complex64 and complex128; the hip backend with both ``rng`` values
and both ``store_potential`` values as well.  Prints one line per call: sha256 of the returned array and of ``plan_c2r.data_out``,
``delta_field_rms``, ``particles_dropped`` and the type name of ``potential`` -- or the exception's type and text.  Run it in each
of the two trees (same library for ``--backend hip``) and diff: every line must be equal, the library being reproducible bit for bit
from call to call.  Each call takes milliseconds; this is a comparison tool, not a test of values."""
import argparse
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from randomfield_amd import Generator  # noqa: E402

SPACING = 2.5
SHAPES = [(16, 16, 16), (10, 6, 12)]
LINES = []


def sha(value):
    if value is None:
        return "None"
    if isinstance(value, (tuple, list)):
        return "+".join(sha(v) for v in value)
    return hashlib.sha256(np.ascontiguousarray(value).tobytes()).hexdigest()[:24]


def run(key, backend, shape, dtype, rng, store):
    nz = shape[2]
    z = np.arange(nz) / float(nz)
    gen = Generator(*shape, SPACING, num_plot_sections=2, backend=backend, dtype=dtype, rng=rng, store_potential=store,
                    growth_function=1.0 / (1.0 + z), mean_matter_density=1.0 + 0.5 * z, redshifts=z,
                    transverse_distance=np.arange(nz) * SPACING, curvature_K=1e-4)
    gen.plan_c2r.data_out_padded[...] = 0          # (the host buffer starts uninitialised; calls that leave the field on the device do not write it)
    rs = np.random.RandomState(17)
    field = rs.normal(size=shape)
    disp = rs.normal(scale=1.5, size=(3,) + shape)
    disp[1, 2, 3, 4] = np.nan                        # (one particle dropped)
    fz = np.linspace(0.5, 1.5, nz)

    def call(label, fn):
        try:
            val = sha(fn(gen))
        except Exception as exc:
            val = "%s %s" % (type(exc).__name__, " ".join(str(exc).split()))
        LINES.append("%s %s: %s out=%s rms=%r dropped=%r potential=%s" % (
            key, label, val, sha(gen.plan_c2r.data_out), None if gen.delta_field_rms is None else float(gen.delta_field_rms),
            gen.particles_dropped, type(gen.potential).__name__))
        print(LINES[-1], flush=True)

    for dl in ((True, False) if backend == "hip" else (True,)):
        d = " download=%d" % dl
        call("delta" + d, lambda g: g.generate_delta_field(seed=3, download=dl))
        call("delta again" + d, lambda g: g.generate_delta_field(seed=3, download=dl))
        call("download_field" + d, lambda g: g.download_field())
        call("delta array seed, smoothing" + d, lambda g: g.generate_delta_field(3.0, seed=[1, 2], save_potential=False, download=dl))
        call("density" + d, lambda g: g.generate_density_field(seed=4, download=dl))
        call("density again, smoothing" + d, lambda g: g.generate_density_field(1.0, seed=5, download=dl))
        call("newtonian without potential" + d, lambda g: g.calculate_newtonian_potential(scale=1.0))
        call("delta for the rest" + d, lambda g: g.generate_delta_field(seed=7, download=dl))
        call("density lognormal" + d, lambda g: g.convert_delta_to_density(download=dl))
        call("delta once more" + d, lambda g: g.generate_delta_field(seed=7, download=dl))
        call("density linear" + d, lambda g: g.convert_delta_to_density(apply_lognormal_transform=False, download=dl))
        call("newtonian light cone" + d, lambda g: g.calculate_newtonian_potential(scale=-1.5, download=dl))
        call("lensing" + d, lambda g: g.calculate_lensing_potential())
        call("lensing i_min=2" + d, lambda g: g.calculate_lensing_potential(i_min=2))
        call("lensing i_min refused" + d, lambda g: g.calculate_lensing_potential(i_min=-1))
        call("newtonian flat" + d, lambda g: g.calculate_newtonian_potential(light_cone=False, scale=2.0, download=dl))
        call("newtonian no scale" + d, lambda g: g.calculate_newtonian_potential())
        call("potential download" + d, lambda g: g.potential.download())
        call("download_field after it" + d, lambda g: g.download_field())
        call("psi x" + d, lambda g: g.calculate_displacement_field("x", download=dl))
        call("psi 1 light cone" + d, lambda g: g.calculate_displacement_field(1, light_cone=True, scale=0.5, download=dl))
        call("psi 2 factor_z" + d, lambda g: g.calculate_displacement_field(2, factor_z=fz, download=dl))
        call("psi2 z" + d, lambda g: g.calculate_displacement_field("z", order=2, download=dl))
        call("psi2 0 light cone" + d, lambda g: g.calculate_displacement_field(0, True, order=2, scale=2.0, download=dl))
        call("psi2 1 factor_z" + d, lambda g: g.calculate_displacement_field(1, order=2, factor_z=fz, download=dl))
        call("psi axis refused" + d, lambda g: g.calculate_displacement_field(3))
        call("psi order refused" + d, lambda g: g.calculate_displacement_field(0, order=0))
        call("lpt2 source" + d, lambda g: g.lpt2_source(download=dl))
        call("psi2 after the source" + d, lambda g: g.calculate_displacement_field(2, order=2, download=dl))
        call("paint without particles" + d, lambda g: g.paint_particles())
        call("gather without particles" + d, lambda g: g.interpolate_at_particles())
        call("positions without particles" + d, lambda g: g.particle_positions())
        call("particles order=2" + d, lambda g: g.particle_displacements(download=dl))
        call("particles order=1 rsd" + d, lambda g: g.particle_displacements(order=1, D1=0.7, download=dl, rsd_axis=2, f1=0.5))
        call("particles order=2 rsd f2" + d, lambda g: g.particle_displacements(order=2, D1=0.7, download=dl, rsd_axis=0, f1=0.5, f2=0.8))
        call("particles refused" + d, lambda g: g.particle_displacements(order=0))
        call("positions" + d, lambda g: g.particle_positions())
        call("paint cic" + d, lambda g: g.paint_particles(download=dl))
        call("paint tsc" + d, lambda g: g.paint_particles(download=dl, assignment="tsc"))
        call("P(k) of the paint, tsc window" + d, lambda g: g.measure_power_spectrum(nbins=4, window="tsc"))
        call("set displacements" + d, lambda g: g.set_particle_displacements(disp))
        call("set displacements refused" + d, lambda g: g.set_particle_displacements(disp[:2]))
        call("shift without gather" + d, lambda g: g.shift_particles(0))
        call("paint interlaced cic" + d, lambda g: g.paint_particles(download=dl, interlaced=True))
        call("P(k) kspace" + d, lambda g: g.measure_power_spectrum(source="kspace"))
        call("P(k) kspace cic window" + d, lambda g: g.measure_power_spectrum(nbins=5, window="cic", source="kspace"))
        call("multipoles kspace" + d, lambda g: g.measure_power_multipoles(los=0, nbins=4, window="cic", source="kspace"))
        call("download_field of the paint" + d, lambda g: g.download_field())
        call("P(k) field" + d, lambda g: g.measure_power_spectrum(k_edges=[0.05, 0.2, 0.4, 0.9]))
        call("P(k) kspace gone" + d, lambda g: g.measure_power_spectrum(source="kspace"))
        call("paint interlaced tsc" + d, lambda g: g.paint_particles(download=dl, assignment="tsc", interlaced=True))
        call("multipoles kspace tables" + d, lambda g: g.measure_power_multipoles(
            los=1, nbins=3, window=[np.full(shape[0], 1.5), None, np.linspace(1.0, 2.0, nz // 2 + 1)], source="kspace"))
        call("multipoles of a field" + d, lambda g: g.measure_power_multipoles(field, los=2, nbins=4, window="ngp"))
        call("multipoles kspace with a field" + d, lambda g: g.measure_power_multipoles(field, source="kspace"))
        call("multipoles los refused" + d, lambda g: g.measure_power_multipoles(los=-1))
        call("P(k) source refused" + d, lambda g: g.measure_power_spectrum(source="x"))
        call("P(k) nbins refused" + d, lambda g: g.measure_power_spectrum(k_edges=[0.1, 0.2], nbins=3))
        call("paint assignment refused" + d, lambda g: g.paint_particles(assignment="pcs"))
        call("gather slot 0" + d, lambda g: g.interpolate_at_particles(download=dl))
        call("gather field slot 1 tsc" + d, lambda g: g.interpolate_at_particles(field, slot=1, coeff=-0.5, download=dl, assignment="tsc"))
        call("gather slot 1 add" + d, lambda g: g.interpolate_at_particles(slot=1, coeff=2.0, first=False, download=dl))
        call("gather slot refused" + d, lambda g: g.interpolate_at_particles(slot=3))
        call("shift 0" + d, lambda g: g.shift_particles(0))
        call("shift 2 by slot 1" + d, lambda g: g.shift_particles(2, slot=1, coeff=0.25))
        call("shift axis refused" + d, lambda g: g.shift_particles(-1))
        call("shift slot refused" + d, lambda g: g.shift_particles(0, slot=7))
        call("displacements after the shifts" + d, lambda g: g._download_particles())
        call("paint after the shifts" + d, lambda g: g.paint_particles(download=dl))
        call("new field" + d, lambda g: g.generate_delta_field(seed=9, save_potential=False, download=dl))
        call("paint after a new field" + d, lambda g: g.paint_particles())
        call("shift after a new field" + d, lambda g: g.shift_particles(0))
        call("psi without potential" + d, lambda g: g.calculate_displacement_field(0))
        call("lpt2 source without potential" + d, lambda g: g.lpt2_source())
        call("plot" + d, lambda g: g.plot_slice())
        call("delta show_plot" + d, lambda g: g.generate_delta_field(seed=1, show_plot=True))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--backend", choices=["numpy", "hip"], required=True)
    backend = ap.parse_args().backend
    for shape in SHAPES:
        for dtype in (np.complex64, np.complex128):
            # (rng='native' needs backend='hip'; store_potential is a hip keyword)
            for rng, store in ([(r, s) for r in ("reference", "native") for s in (False, True)] if backend == "hip" else [("reference", False)]):
                key = "%dx%dx%d %s %s store=%d" % (shape + (np.dtype(dtype).name, rng, store))
                run(key, backend, shape, dtype, rng, store)
    print("# %d lines, sha256 of all: %s" % (len(LINES), hashlib.sha256("\n".join(LINES).encode()).hexdigest()), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
