#!/usr/bin/env python3
"""Time the resampling of a batch of direct solutions onto one node count (lto_direct_resample_batch) at 4 096
starts, 30 -> 30 nodes, with one pass and with two, beside the mesh refinement (lto_direct_refine_batch, tolerances between which
nothing is removed or split) and one frozen QP step (lto_direct_qp_step) on the same batch: wall-clock median of 20 calls after 3
warm-ups, `lto_last_call_ms` beside it.  The batch is synth.direct_problem at the demo's shape, the end targets its own end
states.  Prints one line per figure."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import synth  # noqa: E402


def median_ms(fn, reps=20, warm=3):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main(B=4096, n=30):
    ctx = lto.default_context(0)
    X, U, T = synth.direct_problem(n, B)
    tgs = [lto.direct_targets(X[:, 0, b], X[:, -1, b], 1000.0, np.zeros(3), np.zeros(3)) for b in range(B)]
    prm = (lto.MU, lto.DU, lto.TU, 2000.0)
    kw = dict(MU=lto.MU, DU=lto.DU, TU=lto.TU, Isp=2000.0, n_new=n, ctx=ctx)
    calls = {"lto_direct_resample_batch, passes = 1": lambda: lto.direct_resample(X, U, T, 10, passes=1, **kw),
             "lto_direct_resample_batch, passes = 2": lambda: lto.direct_resample(X, U, T, 10, passes=2, **kw),
             "lto_direct_refine_batch": lambda: lto.direct_refine(X, U, T, 10, *prm, 0.0, np.inf, n, ctx=ctx),
             "lto_direct_qp_step": lambda: lto.direct_qp_step(X, U, T, 10, *prm, tgs, ctx=ctx)}
    for name, call in calls.items():
        med, lo, hi = median_ms(call)
        inner = statistics.median([(call(), ctx.last_call_ms())[1] for _ in range(20)])
        print("%s, %d x %d nodes: median %.3f ms (min %.3f, max %.3f), lto_last_call_ms %.3f" % (name, B, n, med, lo, hi, inner))


if __name__ == "__main__":
    main()
