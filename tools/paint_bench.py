#!/usr/bin/env python3
"""Timing of the cloud-in-cell paint, rf_particles_paint, under its two scatter kernels (rf_particles_set_paint_form): form 1, eight
global 64-bit integer atomics per particle, against form 2, LDS tiles of brick + halo flushed with one global atomic per non-zero tile
cell.  One process, one plan per (grid, displacement scale), the measurements interleaved in rounds (every round paints every case once
under each form, in the same order), medians over the rounds after one warm-up round.  Per paint: the wall clock around call + the
dropped count's arrival, and the scatter kernel alone from rf_kernel_ms ([0] clearing the grid, [1] scatter, [2] conversion).

The displacements are white Gaussian noise of a given rms in cells, made on the device: three realisations of a flat spectrum, each
scaled into one component by rf_particles_accumulate (no host array of the grid's size is ever built).  Both forms must leave the same
accumulator grid: its xor-folded checksum is compared once per case.

What form 2 adds to global memory is counted, not modelled: the displacements of a 256^3 plan made the same way are downloaded and walked
by the CPU emulator with the kernel's own rule (csrc/emu emu_particles_tile_stats -> rf_core.h cic_scatter_tiled, brick and halo from
rf_particles_paint_geometry): the particles that leave their brick's tile, their adds straight into the grid, and the non-zero tile
cells the bricks flush.  White noise is statistically the same in every brick, so the per-particle figures carry over to the large grids;
the bytes per second printed for form 2 are those figures times the grid's particles over the measured scatter time.

--scheme cic|tsc|cic,tsc: the assignment scheme(s), rf_particles_paint_ex; with several, every round paints every case under each scheme
and form in turn, so the unchanged cloud-in-cell kernels are the yardstick of the same run.  The triangular-shaped cloud adds 27 x 8
bytes per particle under form 1; its form 2 figures come from emu_particles_tile_stats_ex with the same scheme.

usage: paint_bench.py [--f64] [--rounds N] [--rms A,B] [--scheme S[,S]] [edge | NXxNYxNZ ...]
       (default: 1024 and 1000, complex64, rms 0.1 and 2, 7 rounds, cic)"""
import ctypes
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from randomfield_amd import _hip, powertools      # noqa: E402

SPACING = 2.5
EMU = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "randomfield_amd", "csrc", "emu", "librf_emu.so")
FORMS = ((1, "global"), (2, "tiled "))
SCHEMES = {"cic": 2, "tsc": 3}                      # name -> RF_ASSIGN_*: the cells per axis


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


class Case(object):
    def __init__(self, shape, ct, rms_cells, stats, schemes):
        self.shape, self.ct, self.rms, self.stats, self.schemes = shape, ct, rms_cells, stats, schemes
        self.plan = white_plan(shape, ct, rms_cells)
        self.wall = {(s, f): [] for s in schemes for f, name in FORMS}
        self.kern = {(s, f): [] for s in schemes for f, name in FORMS}
        self.dropped = None

    def round(self):
        inv_h = [1.0 / SPACING] * 3
        for scheme in self.schemes:
            for form, name in FORMS:
                self.plan.set_paint_form(form)
                self.plan.sync()
                t0 = time.perf_counter()
                self.dropped = self.plan.particles_paint(inv_h, SCHEMES[scheme])
                self.wall[scheme, form].append((time.perf_counter() - t0) * 1e3)
                self.kern[scheme, form].append(self.plan.kernel_ms()[:3])

    def checksums(self, scheme):
        out = []
        for form, name in FORMS:
            self.plan.set_paint_form(form)
            self.plan.particles_paint([1.0 / SPACING] * 3, SCHEMES[scheme])
            A = self.plan.particles_download_counts()
            out.append((int(np.bitwise_xor.reduce(A.ravel())), int(A.sum(dtype=np.uint64))))
        return out

    def report(self):
        cells = float(np.prod(self.shape))
        med = {}
        for scheme in self.schemes:
            head = "%-20s %-10s rms %-4g %s " % (self.shape, np.dtype(self.ct).name, self.rms, scheme)
            per_particle = SCHEMES[scheme] ** 3
            for form, name in FORMS:
                w = self.wall[scheme, form][1:]
                ks = np.asarray(self.kern[scheme, form][1:])
                k = np.median(ks, axis=0)
                med[scheme, form] = float(k[1])
                print(head + "form %d %s wall %8.3f ms (min %.3f max %.3f, %d rounds); clear %.3f scatter %.3f (min %.3f max %.3f) convert %.3f ms"
                      % (form, name, np.median(w), min(w), max(w), len(w), k[0], k[1], ks[:, 1].min(), ks[:, 1].max(), k[2]), flush=True)
            # form 1 adds 8 (27) x 8 bytes per particle
            print(head + "form 1: %.2f TB/s of added bytes; tiled / global scatter = %.3f; dropped %d; plan holds %.2f GB"
                  % (cells * 8 * per_particle / max(med[scheme, 1], 1e-9) / 1e9, med[scheme, 2] / med[scheme, 1], self.dropped, self.plan.nbytes / 1e9),
                  flush=True)
            share, adds, flushed = self.stats[scheme][:3]
            print(head + "form 2: %.4f of the particles leave the tile: %.3f direct + %.3f flushed adds per particle = %.2f TB/s of added bytes"
                  % (share, adds, flushed, cells * 8 * (adds + flushed) / max(med[scheme, 2], 1e-9) / 1e9), flush=True)
            sums = self.checksums(scheme)
            print(head + "accumulator grids of the two forms %s (xor %016x; sum mod 2^64 = %d x 2^48, expected particles mod 65536 = %d)"
                  % ("EQUAL" if sums[0] == sums[1] else "DIFFER", sums[0][0], sums[0][1] >> 48, int(cells) % 65536), flush=True)
        if "cic" in self.schemes and "tsc" in self.schemes:
            head = "%-20s %-10s rms %-4g " % (self.shape, np.dtype(self.ct).name, self.rms)
            print(head + "tsc / cic scatter: global %.3f, tiled %.3f" % (med["tsc", 1] / med["cic", 1], med["tsc", 2] / med["cic", 2]), flush=True)


def tile_stats(ct, rms_cells, scheme, edge=256):
    """per particle of white noise of this rms, by the kernel's own rule: (share that leaves the tile, adds straight into the grid,
    tile cells flushed), and the kernel's brick and halo"""
    shape = (edge,) * 3
    plan = white_plan(shape, ct, rms_cells)
    brick, halo = plan.paint_geometry()
    s3 = [plan.particles_download(axis) for axis in range(3)]
    plan.close()
    emu = ctypes.CDLL(EMU)
    inv_h = (ctypes.c_double * 3)(*[1.0 / SPACING] * 3)
    out = (ctypes.c_ulonglong * 4)()
    emu.emu_particles_tile_stats_ex.argtypes = [ctypes.c_int] * 5 + [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    rc = emu.emu_particles_tile_stats_ex(int(s3[0].dtype == np.float64), SCHEMES[scheme], edge, edge, edge, s3[0].ctypes.data, s3[1].ctypes.data,
                                         s3[2].ctypes.data, ctypes.addressof(inv_h), brick[0], brick[1], brick[2], halo, ctypes.addressof(out))
    assert rc == 0
    n = float(edge) ** 3
    return out[0] / n, out[1] / n, out[2] / n, brick, halo


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
    scales = [float(v) for v in opts["--rms"].split(",")]
    schemes = opts["--scheme"].split(",")
    if not schemes or any(s not in SCHEMES for s in schemes):
        sys.exit("--scheme takes cic, tsc or cic,tsc")
    stats = {}
    for rms in scales:
        stats[rms] = {}
        for scheme in schemes:
            st = stats[rms][scheme] = tile_stats(ct, rms, scheme)
            print("%s form 2, brick %s halo %d, white noise of rms %g cells at 256^3 (emulator count): %.4f of the particles leave the tile, "
                  "%.3f direct adds and %.3f flushed tile cells per particle" % (scheme, st[3], st[4], rms, st[0], st[1], st[2]), flush=True)
    cases = [Case(shape, ct, rms, stats[rms], schemes) for shape in shapes or [(1024,) * 3, (1000,) * 3] for rms in scales]
    for r in range(int(opts["--rounds"]) + 1):  # (the first round warms up: lazy allocations, LDS attributes)
        for case in cases:
            case.round()
    for case in cases:
        case.report()
        case.plan.close()


if __name__ == "__main__":
    main(sys.argv[1:])
