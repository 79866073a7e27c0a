#!/usr/bin/env python3
"""Timing of the binned bispectrum (rf_measure_bispectrum): the whole call by rf_elapsed_ms, data and unit runs, and its parts by
rf_kernel_ms -- [0] the nbins shell filters, [1] the nbins inverse transforms, [2] the triple reduction -- medians over the rounds after
one warm-up round, one process, one plan per grid.  The spectrum is the forward transform of a realisation; linear bins up to 2/3 of
the Nyquist frequency (powertools.default_bispectrum_edges) and the 'closed' triples.

Two yardsticks for the reduction, printed beside it: the time to stream the nbins shell fields ONCE, and the time of `ntriples`
three-field passes, both at the best read+write rate of tools/copy_bench.hip when that program's output of the same job is given with
--copy-log PATH.  The reduction reads every field once per tile of up to 1024 triples; it is bound by LDS reads and float64
arithmetic, not by memory, so reduction / one-pass is expected above 1 -- the ratio is printed as measured.

usage: bispectrum_bench.py [--f64] [--rounds N] [--bins A,B] [--copy-log FILE] [edge | NXxNYxNZ ...]
       (default: 1024 and 1000, complex64, 8 and 16 bins, 5 rounds)"""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from randomfield_amd import _hip, powertools      # noqa: E402

SPACING = 2.5
POWER = powertools.load_default_power()


def copy_rate(path):
    """the best read+write rate tools/copy_bench.hip printed, GB/s"""
    rates = [float(m.group(1)) for m in re.finditer(r"([0-9.]+) GB/s \(read\+write\)", open(path).read())]
    return max(rates) if rates else None


def run(shape, ct, bins, rounds, copy_gbs):
    nx, ny, nz = shape
    plan = _hip.DevicePlan(nx, ny, nz, ct)
    plan.set_kgrid(*powertools.ksq_axes(nx, ny, nz, SPACING))
    plan.set_power(*powertools.sigma_table(POWER, shape, SPACING))
    plan.realise(seed=5)
    plan.execute_r2c()
    base = plan.nbytes
    field_gb = nx * ny * nz * (4 if ct == np.complex64 else 8) / 1e9
    for nbins in bins:
        edges = powertools.default_bispectrum_edges(shape, SPACING, nbins)
        triples = powertools.bispectrum_triples(edges, "closed")
        head = "%-20s %-10s %s %2d bins %4d closed triples " % (shape, np.dtype(ct).name, "tiled  " if plan.tiled else "generic", nbins, len(triples))
        rows = {"data": [], "unit": []}
        for r in range(rounds + 1):
            for what in ("data", "unit"):
                plan.measure_bispectrum(edges, triples, unit=what == "unit")
                if r:
                    rows[what].append([plan.elapsed_ms()] + plan.kernel_ms()[:3])
        for what in ("data", "unit"):
            a = np.array(rows[what])
            med = np.median(a, axis=0)
            print(head + "%s whole call %9.3f ms (min %.3f max %.3f): shell filters %.3f, transforms %.3f, reduction %.3f"
                  % (what, med[0], a[:, 0].min(), a[:, 0].max(), med[1], med[2], med[3]), flush=True)
        red = float(np.median(np.array(rows["data"])[:, 3]))
        chunk, wgs, prows = plan.bispectrum_geometry(nbins, len(triples))
        line = head + "reduction %.3f ms over %d fields of %.2f GB (chunks of %d cells, %d workgroups)" % (red, nbins, field_gb, chunk, wgs)
        if copy_gbs:
            once = nbins * field_gb / (copy_gbs / 2.0) * 1e3            # (the copy's rate counts a read and a write: reading alone moves half)
            passes = len(triples) * 3 * field_gb / (copy_gbs / 2.0) * 1e3
            line += "; copy_bench reaches %.1f GB/s: one pass over the fields %.3f ms, reduction / one pass = %.2f; %d three-field passes %.1f ms, reduction / passes = %.3f" % (
                copy_gbs, once, red / once, len(triples), passes, red / passes)
        print(line, flush=True)
        print(head + "plan holds %.2f GB, of which the call's lazy memory %.2f GB" % (plan.nbytes / 1e9, (plan.nbytes - base) / 1e9), flush=True)
        again = plan.measure_bispectrum(edges, triples)
        print(head + "two calls give the same bits: %s" % np.array_equal(again, plan.measure_bispectrum(edges, triples)), flush=True)
        plan.bispectrum_release()
    plan.close()


def main(argv):
    opts = {"--rounds": "5", "--bins": "8,16", "--copy-log": ""}
    ct, grids, i = np.complex64, [], 0
    while i < len(argv):
        a = argv[i]
        if a == "--f64":
            ct = np.complex128
        elif a in opts:
            opts[a] = argv[i + 1]
            i += 1
        else:
            grids.append(tuple(int(v) for v in a.split("x")) if "x" in a else (int(a),) * 3)
        i += 1
    copy_gbs = copy_rate(opts["--copy-log"]) if opts["--copy-log"] else None
    for shape in grids or [(1024,) * 3, (1000,) * 3]:
        run(shape, ct, [int(b) for b in opts["--bins"].split(",")], int(opts["--rounds"]), copy_gbs)


if __name__ == "__main__":
    main(sys.argv[1:])
