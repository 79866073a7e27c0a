#!/usr/bin/env python3
"""Timing of the cloud-in-cell gather, rf_particles_gather, under its two kernels (rf_particles_set_gather_form): form 1, eight loads of
the field per particle from memory, against form 2, the paint's tile of brick + halo staged in LDS.  One process, one plan per (grid,
displacement scale), one case after the other; every round gathers once under each form (first = 1, slot 0) and then paints the same
displacements with the paint's own choice of scatter kernel -- unchanged code, the yardstick.  Median, minimum and maximum over the
rounds after one warm-up round, all from rf_kernel_ms: [0] after a gather, [1] (the scatter alone) after a paint.

The displacements are white Gaussian noise of a given rms in cells, made on the device as tools/paint_bench.py makes them: three
realisations of a flat spectrum, each scaled into one component by rf_particles_accumulate.  The field gathered is whatever the plan
holds: the last realisation in the first round, the painted density afterwards.  Both forms must leave the same bits in G: an
xor-folded checksum of the downloaded slot is compared once per case.

Algorithmic bytes of a gather: the three displacement components and the field read, the slot written = 5 arrays of the plan's real
type (21.5 GB at 1024^3 complex64); printed per form as a rate and as a fraction of 8 TB/s.

--scheme cic|tsc|cic,tsc: the assignment scheme(s), rf_particles_gather_ex; with several, every round gathers under each scheme and form
in turn, so the unchanged cloud-in-cell kernels are the yardstick of the same run (the paint that closes a round stays cloud in cell).

usage: gather_bench.py [--f64] [--rounds N] [--rms A,B] [--scheme S[,S]] [edge | NXxNYxNZ ...]
       (default: 1024 and 1000, complex64, rms 0.1 and 2, 7 rounds, cic)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from randomfield_amd import _hip, powertools      # noqa: E402

SPACING = 2.5
INV_H = [1.0 / SPACING] * 3
FORMS = ((1, "global"), (2, "tiled "))
SCHEMES = {"cic": 2, "tsc": 3}                      # name -> RF_ASSIGN_*: the cells per axis
PEAK_TBS = 8.0


def white_plan(shape, ct, rms_cells):
    """a plan whose displacement buffer holds white Gaussian noise of rms `rms_cells` cells per component"""
    nx, ny, nz = shape
    plan = _hip.DevicePlan(nx, ny, nz, ct)
    plan.set_kgrid(*powertools.ksq_axes(nx, ny, nz, SPACING))
    xt, st = powertools.sigma_table(powertools.load_default_power(), shape, SPACING)
    plan.set_power(xt, np.ones_like(st))           # a flat spectrum: independent cells
    for axis in range(3):
        plan.realise(seed=100 + axis)
        std = plan.moments()[1]
        plan.particles_accumulate(axis, rms_cells * SPACING / std, first=True)
    return plan


def run_case(shape, ct, rms, rounds, schemes):
    plan = white_plan(shape, ct, rms)
    gather = {(s, f): [] for s in schemes for f, name in FORMS}
    scatter = []
    dropped = 0
    for r in range(rounds + 1):                    # (the first round warms up: lazy allocations, LDS attributes)
        for scheme in schemes:
            for form, name in FORMS:
                plan.set_gather_form(form)
                dropped = plan.particles_gather(INV_H, 0, 1.0, True, SCHEMES[scheme])
                gather[scheme, form].append(plan.kernel_ms()[0])
        plan.particles_paint(INV_H)
        scatter.append(plan.kernel_ms()[1])
    head0 = "%-20s %-10s rms %-4g " % (shape, np.dtype(ct).name, rms)
    cells = float(np.prod(shape))
    nbytes = 5 * cells * (8 if ct == np.complex128 else 4)
    paint = scatter[1:]
    print(head0 + "paint's scatter (its own choice of form)   %8.3f ms (min %.3f max %.3f, %d rounds)"
          % (np.median(paint), min(paint), max(paint), len(paint)), flush=True)
    med = {}
    for scheme in schemes:
        head = head0 + scheme + " "
        for form, name in FORMS:
            g = gather[scheme, form][1:]
            med[scheme, form] = float(np.median(g))
            rate = nbytes / max(med[scheme, form], 1e-9) / 1e9
            print(head + "gather form %d %s                      %8.3f ms (min %.3f max %.3f, %d rounds) = %.3f x the scatter; "
                  "%.2f GB algorithmic = %.2f TB/s = %.1f %% of %g TB/s"
                  % (form, name, med[scheme, form], min(g), max(g), len(g), med[scheme, form] / np.median(paint), nbytes / 1e9, rate,
                     100 * rate / PEAK_TBS, PEAK_TBS), flush=True)
        spread = max(max(gather[scheme, f][1:]) - min(gather[scheme, f][1:]) for f, name in FORMS)
        print(head + "tiled / global = %.3f; global - tiled = %.3f ms against a spread between rounds of %.3f ms; dropped %d; plan holds %.2f GB"
              % (med[scheme, 2] / med[scheme, 1], med[scheme, 1] - med[scheme, 2], spread, dropped, plan.nbytes / 1e9), flush=True)
        sums = []
        for form, name in FORMS:
            plan.set_gather_form(form)
            plan.particles_gather(INV_H, 0, 1.0, True, SCHEMES[scheme])
            G = plan.particles_gather_download(0)
            bits = G.view(np.uint64 if G.dtype == np.float64 else np.uint32).ravel()
            sums.append((int(np.bitwise_xor.reduce(bits)), int(bits.sum(dtype=np.uint64))))
            del G, bits
        print(head + "gathered values of the two forms %s (xor %x)" % ("EQUAL" if sums[0] == sums[1] else "DIFFER", sums[0][0]), flush=True)
    if "cic" in schemes and "tsc" in schemes:
        print(head0 + "tsc / cic gather: global %.3f, tiled %.3f" % (med["tsc", 1] / med["cic", 1], med["tsc", 2] / med["cic", 2]), flush=True)
    plan.close()


def main(argv):
    ct = np.complex128 if "--f64" in argv else np.complex64
    opts = {"--rounds": "7", "--rms": "0.1,2", "--scheme": "cic"}
    skip = set()
    for name in opts:
        if name in argv:
            opts[name] = argv[argv.index(name) + 1]
            skip.add(argv.index(name) + 1)
    shapes = []
    for i, a in enumerate(argv):
        if a.startswith("--") or i in skip:
            continue
        shapes.append(tuple(int(v) for v in a.split("x")) if "x" in a else (int(a),) * 3)
    schemes = opts["--scheme"].split(",")
    if not schemes or any(s not in SCHEMES for s in schemes):
        sys.exit("--scheme takes cic, tsc or cic,tsc")
    for shape in shapes or [(1024,) * 3, (1000,) * 3]:
        for rms in [float(v) for v in opts["--rms"].split(",")]:
            run_case(shape, ct, rms, int(opts["--rounds"]), schemes)


if __name__ == "__main__":
    main(sys.argv[1:])
