#!/usr/bin/env python3
"""Timing of the power spectrum multipoles (rf_measure_multipoles) by rf_elapsed_ms, median of 10 calls after 2 warm-ups, one process,
on one plan per grid: RF_POWER_FROM_KSPACE and RF_POWER_FROM_FIELD, each without and with the three compensation tables (CIC), and in
the same run rf_measure_power on the same plan and data -- the yardstick (profiles/power_measure_bench.log holds its recorded values).
usage: multipole_bench.py [--f64] [--los A] [edge[:nbins] | NXxNYxNZ[:nbins] ...]     (default: 1024:512 and 1000:500, complex64, los 2)"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from randomfield_amd import _hip, powertools      # noqa: E402

SPACING, WARM, REPS = 2.5, 2, 10
POWER = powertools.load_default_power()


def median_ms(plan, call, prepare=None):
    ms = []
    for i in range(WARM + REPS):
        if prepare is not None:
            prepare()
        call()
        ms.append(plan.elapsed_ms())
    ms = ms[WARM:]
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def run(shape, ct, nbins, los):
    nx, ny, nz = shape
    plan = _hip.DevicePlan(nx, ny, nz, ct)
    plan.set_kgrid(*powertools.ksq_axes(nx, ny, nz, SPACING))
    plan.set_power(*powertools.sigma_table(POWER, shape, SPACING))
    edges = powertools.default_k_edges(shape, SPACING, nbins)
    tables = powertools.window_compensation(shape, "cic")
    K, F = _hip.RF_POWER_FROM_KSPACE, _hip.RF_POWER_FROM_FIELD
    name = "%-20s %-10s %s %4d bins los %d " % (shape, np.dtype(ct).name, "tiled  " if plan.tiled else "generic", len(edges) - 1, los)

    def field():                       # a fresh field on the device (tiled plans consume it)
        plan.realise(seed=5)

    field()
    plan.execute_r2c()
    rows = {}
    for source, sname, prepare in ((K, "FROM_KSPACE", None), (F, "FROM_FIELD ", field)):
        rows[sname, "power"] = median_ms(plan, lambda: plan.measure_power(edges, source), prepare)
        rows[sname, "plain"] = median_ms(plan, lambda: plan.measure_multipoles(edges, los, source), prepare)
        rows[sname, "tables"] = median_ms(plan, lambda: plan.measure_multipoles(edges, los, source, tables), prepare)
        print(name + "%s rf_measure_power               %8.3f ms (min %.3f max %.3f)" % ((sname,) + rows[sname, "power"]), flush=True)
        for what, label in (("plain", "no tables"), ("tables", "3 tables ")):
            print(name + "%s rf_measure_multipoles %s %8.3f ms (min %.3f max %.3f)  ratio to rf_measure_power %.3f"
                  % ((sname, label) + rows[sname, what] + (rows[sname, what][0] / rows[sname, "power"][0],)), flush=True)
    # the two calls agree where they must: null tables give rf_measure_power's count exactly, its sum_k and sum_p to summation order
    ref = plan.measure_power(edges, K)
    got = plan.measure_multipoles(edges, los, K)
    same = np.array_equal(got[0], ref[0]) and all(np.allclose(got[i], ref[i], rtol=1e-9, atol=0) for i in (1, 2))
    print(name + "null tables give rf_measure_power's sums: %s; plan holds %.2f GB" % (same, plan.nbytes / 1e9), flush=True)
    plan.close()


def main(argv):
    ct = np.complex128 if "--f64" in argv else np.complex64
    los = int(argv[argv.index("--los") + 1]) if "--los" in argv else 2
    skip = {argv.index("--los") + 1} if "--los" in argv else set()
    grids = []
    for i, a in enumerate(argv):
        if a.startswith("--") or i in skip:
            continue
        a, _, nb = a.partition(":")
        shape = tuple(int(v) for v in a.split("x")) if "x" in a else (int(a),) * 3
        grids.append((shape, int(nb) if nb else None))
    for shape, nbins in grids or [((1024,) * 3, 512), ((1000,) * 3, 500)]:
        run(shape, ct, nbins, los)


if __name__ == "__main__":
    main(sys.argv[1:])
