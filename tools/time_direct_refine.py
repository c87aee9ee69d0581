#!/usr/bin/env python3
"""Wall time of the direct method's mesh refinement: the device call (lto_direct_refine_batch) against the host loop
drivers.meshRefine_direct on HipDirectOps, batched=False and batched=True, on the same fixture -- the synthetic transfer with
0.4 TU segments at nsteps = 10, tol_min = 1e-16, tol_max = 1e-13 -- at 30 and at 1 025 nodes, and for a batch of 32 trajectories of
30 nodes (the host loop takes them one after the other).  Warm-up, then the median (and the range) of `reps` calls, the forms alternating; lto_last_call_ms
beside the wall clock of the device call.  The removed-node count stands next to the times: the host loop pays one round trip per removed node."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402

ISP, NSTEPS, TOL_MIN, TOL_MAX = 2000.0, 10, 1e-16, 1e-13


def timed_ms(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def stats(ms):
    return "%9.3f ms  (%.3f .. %.3f, %d calls)" % (statistics.median(ms), min(ms), max(ms), len(ms))


def main(reps=9):
    ctx = lto.default_context(0)
    ops = drivers.HipDirectOps(MU, DU, TU, ISP, ctx=ctx)
    for n, B in ((30, 1), (1025, 1), (30, 32)):
        X, U, T = synth.direct_problem(n, n_batch=B, seed=3, dt_seg=0.4)
        M = 8 * n
        each = [(X[:, :, b], U[:, :, b], T[:, b]) for b in range(B)]
        dev_in = (X, U, T) if B > 1 else each[0]
        call_ms = []

        def dev():
            r = lto.direct_refine(*dev_in, NSTEPS, MU, DU, TU, ISP, TOL_MIN, TOL_MAX, M, ctx=ctx)
            call_ms.append(ctx.last_call_ms())
            return r

        def host(batched):
            return [drivers.meshRefine_direct(x, u, t, 6, n, NSTEPS, ISP, MU, DU, TU, tol_min=TOL_MIN, tol_max=TOL_MAX, max_nodes=M,
                                              batched=batched, ops=ops, verbose=False) for x, u, t in each]

        # warm-up of every form at this shape; the results also show that the three compute one mesh
        r = dev()
        dev()
        rs = r if B > 1 else [r]
        for batched in (True, False):
            for q, h in zip(rs, host(batched)):
                assert h[3] == q.n and np.array_equal(h[2], q.t), "the host loop and the device call disagree"
        del call_ms[:]
        # the three forms alternate within a round, so that a disturbance of the machine meets all of them
        hreps = reps if n * B <= 64 else 3
        t_dev, t_true, t_false = [], [], []
        for rep in range(reps):
            t_dev.append(timed_ms(dev))
            if rep < hreps:
                t_true.append(timed_ms(lambda: host(True)))
                t_false.append(timed_ms(lambda: host(False)))
        print("%d nodes x %d: removed %d, inserted %d, passes (max) %d, nodes after %s" % (
            n, B, sum(q.n_removed for q in rs), sum(q.n - (n - q.n_removed) for q in rs), max(q.passes for q in rs),
            rs[0].n if B == 1 else "%d..%d" % (min(q.n for q in rs), max(q.n for q in rs))))
        print("  device call               " + stats(t_dev) + "  lto_last_call_ms " + stats(call_ms))
        print("  host loop, batched=True   " + stats(t_true))
        print("  host loop, batched=False  " + stats(t_false))


if __name__ == "__main__":
    main()
