#!/usr/bin/env python3
"""Time the stacked initial guess on the device (lto_stack_guess_batch) at B = 1 and B = 4096 starts of the demo's
shape (30 nodes, 10 + 10 days, tau1 spread over [0, 1)): wall-clock median of 20 calls after 3 warm-ups, `lto_last_call_ms` beside
it -- and the route the library had before: examples/halo_transfer_demo.py::stacked_guess (table interpolation on the host, one
start per call), timed per call and scaled to B calls.  Prints one line per figure."""
import importlib.util
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import synth  # noqa: E402
from lowthrustopt_amd.constants import TU, day  # noqa: E402


def median_ms(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ctx = lto.default_context(0)
    tabs = synth.halo_orbits()
    orbits = lto.DirectOrbits(np.linspace(0, 1, 100), tabs[0], np.linspace(0, 1, 100), tabs[1])
    tof = 10.0 * day / TU
    for B in (1, 4096):
        tau1 = (0.75 + np.arange(B) / float(B)) % 1.0
        call = lambda: lto.stack_guess(tau1, tof, tof, 30, orbits, ctx=ctx)
        med, lo, hi = median_ms(call)
        inner = statistics.median([(call(), ctx.last_call_ms())[1] for _ in range(20)])
        g = call()
        print("device, B = %4d: median %.3f ms (min %.3f, max %.3f), lto_last_call_ms %.3f, status 0 for %d starts"
              % (B, med, lo, hi, inner, int(np.count_nonzero(g.status == 0))))
    spec = importlib.util.spec_from_file_location("halo_transfer_demo", os.path.join(ROOT, "examples", "halo_transfer_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    med, lo, hi = median_ms(lambda: mod.stacked_guess(30, 20.0, 0.75))
    print("host table interpolation, one start: median %.3f ms (min %.3f, max %.3f); x 4096 starts = %.1f ms" % (med, lo, hi, med * 4096))


if __name__ == "__main__":
    main()
