#!/usr/bin/env python3
"""Timing of the interlaced paint, rf_particles_paint_interlaced: the whole call, its parts, and two yardsticks taken in the same run.

One process, one case (grid, displacement scale) at a time -- a 1024^3 complex64 plan with the stash holds 34 GB -- with the assignment
schemes and the three sequences below interleaved in rounds, medians over the rounds after one warm-up round:

  whole    rf_particles_paint_interlaced: the wall clock around call + return, and rf_elapsed_ms, which covers the whole call
  parts    the same sequence through the public calls -- paint (half_cell 0), rf_execute_r2c, rf_kspace_stash, paint (half_cell 1),
           rf_execute_r2c, rf_kspace_interlace, rf_execute_c2r -- each read with rf_elapsed_ms.  (The whole call has no stash sweep:
           its first transform writes straight into the stash.)
  parent   2 x (rf_particles_paint_ex + rf_execute_r2c) + rf_execute_c2r with ANOTHER BUILD of the library, --parent PATH (the commit
           before the feature), on a plan of its own holding the same displacements: what a user paid for the two fields before, on the
           device, without the combine.  whole / parent should exceed 1 by the combine and nothing else.

The combine moves two reads and one write of the half spectrum; its rate is printed beside the best read+write rate of
tools/copy_bench.hip when that program's output of the same job is given with --copy-log PATH.

The displacements are white Gaussian noise of a given rms in cells, made on the device as tools/paint_bench.py makes them.

usage: interlace_bench.py [--f64] [--rounds N] [--rms A,B] [--scheme S[,S]] [--parent LIB] [--copy-log FILE] [edge | NXxNYxNZ ...]
       (default: 1024 and 1000, complex64, rms 0.1 and 2, 5 rounds, cic,tsc)"""
import importlib.util
import os
import re
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from randomfield_amd import _hip, powertools      # noqa: E402

SPACING = 2.5
INV_H = [1.0 / SPACING] * 3
SCHEMES = {"cic": 2, "tsc": 3}
NEW_CALLS = ("rf_particles_paint_shifted", "rf_kspace_stash", "rf_kspace_interlace", "rf_particles_paint_interlaced")
PARTS = ("paint 0", "r2c 0", "stash", "paint 1", "r2c 1", "combine", "c2r")


def load_other_build(path):
    """the binding over another build of the library (one without the interlaced paint's entry points)"""
    spec = importlib.util.spec_from_file_location("randomfield_amd._hip_other", _hip.__file__)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.LIB_PATH = os.path.abspath(path)
    for name in NEW_CALLS:
        mod.SIGNATURES.pop(name, None)
    mod.load()
    return mod


def white_plan(binding, shape, ct, rms_cells):
    """a plan whose displacement buffer holds white Gaussian noise of rms `rms_cells` cells per component (tools/paint_bench.py)"""
    nx, ny, nz = shape
    plan = binding.DevicePlan(nx, ny, nz, ct)
    plan.set_kgrid(*powertools.ksq_axes(nx, ny, nz, SPACING))
    xt, st = powertools.sigma_table(powertools.load_default_power(), shape, SPACING)
    plan.set_power(xt, np.ones_like(st))
    for axis in range(3):
        plan.realise(seed=100 + axis)
        std = plan.moments()[1]
        plan.particles_accumulate(axis, rms_cells * SPACING / std, first=True)
    return plan


def timed(plan, call):
    """(wall ms around call + drain, rf_elapsed_ms) of one call"""
    plan.sync()
    t0 = time.perf_counter()
    call()
    plan.sync()
    wall = (time.perf_counter() - t0) * 1e3
    return wall, plan.elapsed_ms()


class Case(object):
    def __init__(self, shape, ct, rms, schemes, parent):
        self.shape, self.ct, self.rms, self.schemes = shape, ct, rms, schemes
        self.plan = white_plan(_hip, shape, ct, rms)
        self.old = white_plan(parent, shape, ct, rms) if parent else None
        self.tabs = powertools.interlace_phases(shape)
        self.whole = {s: [] for s in schemes}
        self.parts = {s: [] for s in schemes}
        self.parent = {s: [] for s in schemes}

    def round(self):
        p, o = self.plan, self.old
        for s in self.schemes:
            order = SCHEMES[s]
            self.whole[s].append(timed(p, lambda: p.particles_paint_interlaced(INV_H, order, self.tabs)))
            steps = (lambda: p.particles_paint(INV_H, order, half_cell=False), p.execute_r2c, p.kspace_stash,
                     lambda: p.particles_paint(INV_H, order, half_cell=True), p.execute_r2c, lambda: p.kspace_interlace(self.tabs), p.execute_c2r)
            self.parts[s].append([timed(p, step) for step in steps])
            if o is not None:
                steps = (lambda: o.particles_paint(INV_H, order), o.execute_r2c, lambda: o.particles_paint(INV_H, order), o.execute_r2c, o.execute_c2r)
                t0 = time.perf_counter()
                each = [timed(o, step) for step in steps]
                self.parent[s].append(((time.perf_counter() - t0) * 1e3, sum(e[1] for e in each)))

    def report(self, copy_gbs):
        kbytes = float(self.shape[0] * self.shape[1] * (self.shape[2] // 2 + 1) * np.dtype(self.ct).itemsize)
        for s in self.schemes:
            head = "%-20s %-10s rms %-4g %s " % (self.shape, np.dtype(self.ct).name, self.rms, s)
            w = np.asarray(self.whole[s][1:])
            print(head + "whole call: wall %8.3f ms (min %.3f max %.3f, %d rounds), rf_elapsed_ms %8.3f (min %.3f max %.3f); plan holds %.2f GB"
                  % (np.median(w[:, 0]), w[:, 0].min(), w[:, 0].max(), len(w), np.median(w[:, 1]), w[:, 1].min(), w[:, 1].max(), self.plan.nbytes / 1e9),
                  flush=True)
            parts = np.asarray(self.parts[s][1:])[:, :, 1]                       # rounds x parts, rf_elapsed_ms
            med = np.median(parts, axis=0)
            print(head + "parts (rf_elapsed_ms): " + ", ".join("%s %.3f" % (n, v) for n, v in zip(PARTS, med)) + "; sum %.3f, without the stash %.3f"
                  % (med.sum(), med.sum() - med[2]), flush=True)
            c = parts[:, 5]
            rate = 3.0 * kbytes / np.median(c) / 1e6
            line = head + "combine: %.3f ms (min %.3f max %.3f) = %.1f GB/s of two reads and one write of %.2f GB" % (np.median(c), c.min(), c.max(), rate,
                                                                                                                 kbytes / 1e9)
            if copy_gbs:
                line += "; copy_bench reaches %.1f GB/s: combine / copy = %.3f" % (copy_gbs, rate / copy_gbs)
            print(line, flush=True)
            if self.old is not None:
                o = np.asarray(self.parent[s][1:])
                print(head + "parent build, 2 x (paint + r2c) + c2r: wall %8.3f ms (min %.3f max %.3f), sum of rf_elapsed_ms %8.3f; "
                      "whole / parent = %.3f (wall), %.3f (device)"
                      % (np.median(o[:, 0]), o[:, 0].min(), o[:, 0].max(), np.median(o[:, 1]), np.median(w[:, 0]) / np.median(o[:, 0]),
                         np.median(w[:, 1]) / np.median(o[:, 1])), flush=True)

    def close(self):
        self.plan.close()
        if self.old is not None:
            self.old.close()


def copy_rate(path):
    """the best read+write rate tools/copy_bench.hip printed, GB/s"""
    rates = [float(m.group(1)) for m in re.finditer(r"([0-9.]+) GB/s \(read\+write\)", open(path).read())]
    return max(rates) if rates else None


def main(argv):
    ct = np.complex128 if "--f64" in argv else np.complex64
    opts = {"--rounds": "5", "--rms": "0.1,2", "--scheme": "cic,tsc", "--parent": "", "--copy-log": ""}
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
    _hip.require_gpu()
    parent = load_other_build(opts["--parent"]) if opts["--parent"] else None
    copy_gbs = copy_rate(opts["--copy-log"]) if opts["--copy-log"] else None
    for shape in shapes or [(1024,) * 3, (1000,) * 3]:
        for rms in [float(v) for v in opts["--rms"].split(",")]:
            case = Case(shape, ct, rms, schemes, parent)
            for r in range(int(opts["--rounds"]) + 1):      # (the first round warms up: lazy allocations, LDS attributes)
                case.round()
            case.report(copy_gbs)
            case.close()


if __name__ == "__main__":
    main(sys.argv[1:])
