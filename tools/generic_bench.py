#!/usr/bin/env python3
"""Timing of the generic (non-power-of-two) path: realisations on grids such as 1000^3 against the tiled 1024^3.
usage: generic_bench.py [--lib variant.so] [--fused] [--f64] [--reps N] [edge | NXxNYxNZ ...]
--fused: every generic shape twice in ONE process and on one plan -- generation as a launch of its own (the default of the C ABI), then
inside the x pass (RF_FLAG_FUSED_GENERIC_GENERATION) -- interleaved rounds, median wall time per realisation, rf_kernel_ms of each."""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from randomfield_amd import _hip, powertools      # noqa: E402

POWER = powertools.load_default_power()
KERNELS = ("x", "y", "z", "reduce", "gen")


def make(shape, ct):
    nx, ny, nz = shape
    p = _hip.DevicePlan(nx, ny, nz, ct)
    p.set_kgrid(*powertools.ksq_axes(nx, ny, nz, 2.5))
    p.set_power(*powertools.sigma_table(POWER, shape, 2.5))
    return p


def timed(p, reps, seed0):
    t0 = time.perf_counter()
    for i in range(reps):
        p.realise(seed=seed0 + i)
    p.sync()
    return (time.perf_counter() - t0) / reps * 1e3


def run(shape, ct=np.complex64, reps=3):
    nx, ny, nz = shape
    p = make(shape, ct)
    p.realise(seed=1)
    p.sync()
    ms = timed(p, reps, 2)
    k = p.kernel_ms()
    std = p.moments()[1]
    tiled = p.tiled
    p.close()
    cells = float(nx) * ny * nz
    print("%-20s %-10s %s  %9.3f ms  %9.1f Mcells/s  rms %.4f kernels %s" % (shape, np.dtype(ct).name, "tiled  " if tiled else "generic", ms, cells / ms / 1e3, std,
                                                                      np.round(k, 3)), flush=True)


def run_fused(shape, ct=np.complex64, reps=3, rounds=5):
    """Both forms on one plan, `rounds` interleaved rounds of at least `reps` realisations (and 0.3 s) each after a warm-up of each form;
    medians."""
    nx, ny, nz = shape
    p = make(shape, ct)
    if p.tiled:
        p.close()
        return run(shape, ct, reps)
    wall = {False: [], True: []}
    kern = {False: [], True: []}
    std = {}
    for on in (False, True):
        p.set_fused_generation(on)
        p.realise(seed=1)
        p.sync()
        std[on] = p.moments()[1]
    reps = max(reps, min(400, int(300.0 / max(timed(p, 3, 2), 1e-3)) + 1))      # windows of at least 0.3 s
    for r in range(rounds):
        for on in (False, True):
            p.set_fused_generation(on)
            wall[on].append(timed(p, reps, 2))
            kern[on].append(p.kernel_ms())
    p.close()
    assert std[False] == std[True], "the fused form changed the field's rms: %r" % (std,)
    cells = float(nx) * ny * nz
    med = {on: float(np.median(wall[on])) for on in wall}
    for on in (False, True):
        k = np.median(np.array(kern[on]), axis=0)
        print("%-20s %-10s generic %-8s %9.3f ms (min %.3f max %.3f)  %9.1f Mcells/s  rms %.4f  kernels %s" % (
            shape, np.dtype(ct).name, "fused" if on else "unfused", med[on], min(wall[on]), max(wall[on]), cells / med[on] / 1e3, std[on],
            " ".join("%s %.3f" % (n, v) for n, v in zip(KERNELS, k))), flush=True)
    es = np.dtype(ct).itemsize // 2
    print("%-20s %-10s fused / unfused = %.3f (%d realisations per window);  bytes per cell: algorithmic %.2f, moved %.0f fused, %.0f unfused" % (
        shape, np.dtype(ct).name, med[True] / med[False], reps, 5 * es * (1 + 2.0 / nz), 5 * es, 7 * es), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    fused, ct, reps = False, np.complex64, 3
    while args and args[0].startswith("--"):
        if args[0] == "--lib":
            _hip.LIB_PATH = os.path.abspath(args[1])
            args = args[2:]
        elif args[0] == "--reps":
            reps = int(args[1])
            args = args[2:]
        elif args[0] == "--fused":
            fused = True
            args = args[1:]
        elif args[0] == "--f64":
            ct = np.complex128
            args = args[1:]
        else:
            sys.exit(__doc__)
    for a in args or ["500", "512", "1000", "1024"]:
        shape = tuple(int(v) for v in a.split("x")) if "x" in a else (int(a),) * 3
        (run_fused if fused else run)(shape, ct, reps)
