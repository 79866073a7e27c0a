#!/usr/bin/env python3
"""Timing of the generic (non-power-of-two) path: realisations on grids such as 1000^3 against the tiled 1024^3.
usage: generic_bench.py [--lib variant.so] [--fused | --gradient] [--f64] [--reps N] [edge | NXxNYxNZ ...]
--fused: every generic shape twice in ONE process and on one plan -- generation as a launch of its own (the default of the C ABI), then
inside the x pass (RF_FLAG_FUSED_GENERIC_GENERATION) -- interleaved rounds, median wall time per realisation, rf_kernel_ms of each.
--gradient: one component of the gradient of the potential (rf_execute_gradient_c2r) on every generic shape, in ONE process and on one
plan: the factor inside the x pass against the elementwise kernel + rf_execute_c2r, with the plain rf_execute_c2r as the yardstick."""
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


def run_gradient(shape, ct=np.complex64, reps=3, rounds=5, axis=0):
    """Three forms on one plan with the stored potential of one realisation as the source, interleaved rounds, medians: the plain c2r
    of the k buffer (yardstick), load_gradient + execute_c2r (a read-and-write sweep of k space more), execute_gradient (no sweep)."""
    nx, ny, nz = shape
    p = make(shape, ct)
    if p.tiled:
        p.close()
        print("%-20s tiled plan: rf_execute_gradient_c2r runs the elementwise kernel + rf_execute_c2r there" % (shape,), flush=True)
        return
    P = _hip.RF_GRAD_FROM_POTENTIAL
    dk = 2 * np.pi / (shape[axis] * 2.5)
    p.realise_potential(seed=1)

    def plain():
        p.execute_c2r()

    def unfused():
        p.load_gradient(axis, 1.0, dk, P)
        p.execute_c2r()

    def fused():
        p.execute_gradient(axis, 1.0, dk, P)

    forms = (("c2r", plain), ("sweep+c2r", unfused), ("fused", fused))

    def window(f, n):
        t0 = time.perf_counter()
        for _ in range(n):
            f()
        p.sync()
        return (time.perf_counter() - t0) / n * 1e3

    std = {}
    p.load_gradient(axis, 1.0, dk, P)          # (the yardstick transforms the component too: same data in every form)
    for name, f in forms:
        f()
        p.sync()
        std[name] = p.moments()[1]
    assert std["fused"] == std["sweep+c2r"], "the fused form changed the field's rms: %r" % (std,)
    reps = max(reps, min(400, int(300.0 / max(window(fused, 3), 1e-3)) + 1))      # windows of at least 0.3 s
    wall = {name: [] for name, _ in forms}
    kern = {name: [] for name, _ in forms}
    for r in range(rounds):
        for name, f in forms:
            wall[name].append(window(f, reps))
            kern[name].append(p.kernel_ms())
    p.close()
    med = {name: float(np.median(wall[name])) for name in wall}
    for name, _ in forms:
        k = np.median(np.array(kern[name]), axis=0)
        print("%-20s %-10s axis %d %-10s %9.3f ms (min %.3f max %.3f)  rms %.4g  kernels of the c2r %s" % (
            shape, np.dtype(ct).name, axis, name, med[name], min(wall[name]), max(wall[name]), std[name],
            " ".join("%s %.3f" % (n, v) for n, v in zip(KERNELS, k))), flush=True)
    print("%-20s %-10s fused / (sweep + c2r) = %.3f, fused / c2r = %.3f, (sweep + c2r) / c2r = %.3f (%d calls per window)" % (
        shape, np.dtype(ct).name, med["fused"] / med["sweep+c2r"], med["fused"] / med["c2r"], med["sweep+c2r"] / med["c2r"], reps), flush=True)


if __name__ == "__main__":
    args = sys.argv[1:]
    fused, gradient, ct, reps = False, False, np.complex64, 3
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
        elif args[0] == "--gradient":
            gradient = True
            args = args[1:]
        elif args[0] == "--f64":
            ct = np.complex128
            args = args[1:]
        else:
            sys.exit(__doc__)
    for a in args or ["500", "512", "1000", "1024"]:
        shape = tuple(int(v) for v in a.split("x")) if "x" in a else (int(a),) * 3
        (run_gradient if gradient else run_fused if fused else run)(shape, ct, reps)
