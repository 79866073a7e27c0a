#!/usr/bin/env python3
"""Timing of the binned power spectrum measurement (rf_measure_power) by rf_elapsed_ms, median of 10 calls after 2 warm-ups, on one plan
per grid: (a) RF_POWER_FROM_KSPACE alone, (b) RF_POWER_FROM_FIELD (tiled plans: forward passes in place + the sweep of the packed array,
no k-space array), (c) rf_execute_r2c + RF_POWER_FROM_KSPACE (the forward transform with its unpack pass, then the sweep).
usage: power_bench.py [--f64] [--nbins N] [edge | NXxNYxNZ ...]     (default: 1024 and 1000, complex64, min(shape) // 2 bins)"""
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
        ms.append(call.ms() if hasattr(call, "ms") else plan.elapsed_ms())
    ms = ms[WARM:]
    return float(np.median(ms)), float(min(ms)), float(max(ms))


def run(shape, ct, nbins):
    nx, ny, nz = shape
    plan = _hip.DevicePlan(nx, ny, nz, ct)
    plan.set_kgrid(*powertools.ksq_axes(nx, ny, nz, SPACING))
    plan.set_power(*powertools.sigma_table(POWER, shape, SPACING))
    edges = powertools.default_k_edges(shape, SPACING, nbins)
    K, F = _hip.RF_POWER_FROM_KSPACE, _hip.RF_POWER_FROM_FIELD
    name = "%-20s %-10s %s %4d bins " % (shape, np.dtype(ct).name, "tiled  " if plan.tiled else "generic", len(edges) - 1)

    def field():                       # a fresh field on the device (tiled plans consume it)
        plan.realise(seed=5)

    # (a) the sweep alone, on the spectrum of that field
    field()
    plan.execute_r2c()
    a = median_ms(plan, lambda: plan.measure_power(edges, K))
    kbytes = float(nx) * ny * (nz // 2 + 1) * np.dtype(ct).itemsize
    print(name + "(a) FROM_KSPACE          %8.3f ms (min %.3f max %.3f)  %.2f TB/s of k space read" % (a + (kbytes / a[0] / 1e9,)), flush=True)
    ref = plan.measure_power(edges, K)
    # (b) from the field in one call
    b = median_ms(plan, lambda: plan.measure_power(edges, F), prepare=field)
    print(name + "(b) FROM_FIELD           %8.3f ms (min %.3f max %.3f)" % b, flush=True)
    field()
    got = plan.measure_power(edges, F)
    # (c) the two calls: both elapsed times are added
    class Two(object):
        def __call__(self):
            plan.execute_r2c()
            self.t = plan.elapsed_ms()
            plan.measure_power(edges, K)
            self.t += plan.elapsed_ms()

        def ms(self):
            return self.t
    c = median_ms(plan, Two(), prepare=field)
    print(name + "(c) r2c + FROM_KSPACE    %8.3f ms (min %.3f max %.3f)" % c, flush=True)
    same = np.array_equal(got[0], ref[0]) and np.allclose(got[2], ref[2], rtol=1e-9, atol=0)
    print(name + "(b) / (c) = %.3f; (b) and (c) agree: %s; plan holds %.2f GB" % (b[0] / c[0], same, plan.nbytes / 1e9), flush=True)
    plan.close()


def main(argv):
    ct = np.complex128 if "--f64" in argv else np.complex64
    nbins = int(argv[argv.index("--nbins") + 1]) if "--nbins" in argv else None
    skip = {argv.index("--nbins") + 1} if "--nbins" in argv else set()
    shapes = []
    for i, a in enumerate(argv):
        if a.startswith("--") or i in skip:
            continue
        shapes.append(tuple(int(v) for v in a.split("x")) if "x" in a else (int(a),) * 3)
    for shape in shapes or [(1024,) * 3, (1000,) * 3]:
        run(shape, ct, nbins)


if __name__ == "__main__":
    main(sys.argv[1:])
