#!/usr/bin/env python3
"""Timing of the second-order (2LPT) potential, rf_lpt2_potential, against its building block as it was before: six
rf_execute_gradient_c2r(RF_GRAD_FROM_POTENTIAL) calls on the same plan.  One process, one plan per grid, the measurements interleaved in
rounds (every round runs every measurement of every grid once, in the same order), wall clock around call + rf_sync, medians over the
rounds after one warm-up round:

    (a) rf_lpt2_potential                       six Hessian transforms + five accumulate sweeps and the first copy + r2c + the 1/k^2 sweep
    (b) 6 x rf_execute_gradient_c2r(POTENTIAL)  the yardstick
    (c) rf_lpt2_source                          (a) without the forward transform and the division
    (d) 6 x rf_execute_hessian_c2r(POTENTIAL)   (c) without the six real-space sweeps
    (e) rf_execute_gradient_c2r(POTENTIAL2)     one component of psi2 afterwards

usage: lpt2_bench.py [--f64] [--rounds N] [edge | NXxNYxNZ ...]     (default: 1024 and 1000, complex64, 9 rounds)"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from randomfield_amd import _hip, powertools      # noqa: E402

SPACING = 2.5
POWER = powertools.load_default_power()
PAIRS = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]


class Case(object):
    def __init__(self, shape, ct):
        nx, ny, nz = shape
        self.shape, self.ct = shape, ct
        self.plan = plan = _hip.DevicePlan(nx, ny, nz, ct)
        plan.set_kgrid(*powertools.ksq_axes(nx, ny, nz, SPACING))
        plan.set_power(*powertools.sigma_table(POWER, shape, SPACING))
        plan.realise_potential(seed=5)
        self.dk = [2 * np.pi / (n * SPACING) for n in shape]
        P, P2 = _hip.RF_GRAD_FROM_POTENTIAL, _hip.RF_GRAD_FROM_POTENTIAL2
        dk = self.dk
        self.calls = [
            ("(a) lpt2_potential", lambda: plan.lpt2_potential(dk)),
            ("(b) 6 x gradient c2r", lambda: [plan.execute_gradient(a % 3, 1.0, dk[a % 3], P) for a in range(6)]),
            ("(c) lpt2_source", lambda: plan.lpt2_source(dk)),
            ("(d) 6 x hessian c2r", lambda: [plan.execute_hessian(a, b, 1.0, dk[a], dk[b], P) for a, b in PAIRS]),
            ("(e) gradient c2r, psi2", lambda: plan.execute_gradient(0, 3.0 / 7.0, dk[0], P2)),
        ]
        self.ms = {name: [] for name, call in self.calls}

    def round(self):
        for name, call in self.calls:
            if name.startswith("(e)"):                  # (untimed: (c) took the second-order potential's memory for its accumulators)
                self.plan.lpt2_potential(self.dk)
            self.plan.sync()
            t0 = time.perf_counter()
            call()
            self.plan.sync()
            self.ms[name].append((time.perf_counter() - t0) * 1e3)

    def report(self):
        head = "%-20s %-10s %s " % (self.shape, np.dtype(self.ct).name, "tiled  " if self.plan.tiled else "generic")
        med = {}
        for name, call in self.calls:
            v = self.ms[name][1:]
            med[name[:3]] = float(np.median(v))
            print(head + "%-24s %8.3f ms (min %.3f max %.3f, %d rounds)" % (name, np.median(v), min(v), max(v), len(v)), flush=True)
        cells = float(np.prod(self.shape))
        sweeps = med["(c)"] - med["(d)"]
        bytes_per_cell = (8 + 16 + 16 + 12 + 12 + 12) / 4.0 * np.dtype(self.ct).itemsize / 2     # FIRST, DIAG2, DIAG3, OFF, OFF, LAST
        print(head + "(a) / (b) = %.3f; six sweeps (c) - (d) = %.3f ms = %.2f TB/s; r2c + division (a) - (c) = %.3f ms; plan holds %.2f GB"
              % (med["(a)"] / med["(b)"], sweeps, cells * bytes_per_cell / max(sweeps, 1e-9) / 1e9, med["(a)"] - med["(c)"], self.plan.nbytes / 1e9),
              flush=True)


def main(argv):
    ct = np.complex128 if "--f64" in argv else np.complex64
    rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 9
    skip = {argv.index("--rounds") + 1} if "--rounds" in argv else set()
    shapes = []
    for i, a in enumerate(argv):
        if a.startswith("--") or i in skip:
            continue
        shapes.append(tuple(int(v) for v in a.split("x")) if "x" in a else (int(a),) * 3)
    cases = [Case(shape, ct) for shape in shapes or [(1024,) * 3, (1000,) * 3]]
    for r in range(rounds + 1):                 # (the first round warms up: lazy allocations, LDS attributes)
        for case in cases:
            case.round()
    for case in cases:
        case.report()
        case.plan.close()


if __name__ == "__main__":
    main(sys.argv[1:])
