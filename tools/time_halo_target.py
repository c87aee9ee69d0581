#!/usr/bin/env python3
"""Time the targeted periodic-orbit corrector on the device (lto_halo_target_batch): `lto_last_call_ms`, median of 10
calls after 3 warm-ups.  B = 1 and B = 4096 with one target (the packaged orbit 1 corrected, asked for Jacobi constants spread over
2e-4 .. 1e-3 above its own), a march of 8 members (the L1 and L2 Lyapunov orbits to C = 3.15), and the same march as 8 single-target calls
chained on the host with the same predictor.  Prints one line per figure."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU  # noqa: E402


def median_call_ms(ctx, fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    return statistics.median([fn() for _ in range(reps)])


def main():
    ctx = lto.default_context(0)
    s1 = np.array(synth.halo_orbits()[0][:6, 0])
    s1[[1, 3, 5]] = 0.0
    base = lto.halo_correct(s1, "x0", ctx=ctx)
    C1 = drivers._jacobi_of(base.state, MU)
    for B in (1, 4096):
        seeds = np.repeat(base.state[:, None], B, axis=1)
        q = C1 + 1e-3 * (0.2 + 0.8 * (np.arange(B) + 0.5) / B)                   # 2e-4 .. 1e-3 off: a few Newton steps each
        for what, targets in (("jacobi", q), ("period", base.period + (q - C1))):
            r = lto.halo_target(seeds, targets[None, :], what=what, ctx=ctx)

            def once():
                lto.halo_target(seeds, targets[None, :], what=what, ctx=ctx)
                return ctx.last_call_ms()
            print("halo_target (%s), B = %4d, 1 target: lto_last_call_ms %.3f, status 0 for %d orbits, iterations %d .. %d"
                  % (what, B, median_call_ms(ctx, once), int(np.count_nonzero(r.status == 0)), r.iterations.min(), r.iterations.max()))

    lyap = np.array([drivers.lyapunov_seed(w, 1e-2, MU)[0] for w in (1, 2)]).T
    own = lto.halo_correct(lyap, "planar", ctx=ctx)
    steps = drivers._step_table(drivers._jacobi_of(own.state, MU), 3.15, 8)
    r = lto.halo_target(own.state, steps, planar=True, ctx=ctx)

    def march():
        lto.halo_target(own.state, steps, planar=True, ctx=ctx)
        return ctx.last_call_ms()

    def chained():
        total, pts = 0.0, []
        for k in range(8):
            if k == 0:
                start = own.state
            elif k == 1:
                start = pts[0]
            else:
                start = pts[-1] + (pts[-1] - pts[-2]) * ((steps[k] - steps[k - 1]) / (steps[k - 1] - steps[k - 2]))
            m = lto.halo_target(np.asfortranarray(start), steps[k][None, :], planar=True, ctx=ctx)
            total += ctx.last_call_ms()
            pts.append(m.state[:, 0, :])
        return total
    print("march of 8 members x 2 orbits in one call: lto_last_call_ms %.3f, statuses %s, iterations %s"
          % (median_call_ms(ctx, march), sorted(set(r.status.ravel().tolist())), r.iterations.T.tolist()))
    print("the same march as 8 calls from the host: the sum of lto_last_call_ms %.3f" % median_call_ms(ctx, chained))

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)
    print("wall clock with the Python layer: one call %.3f ms, 8 calls %.3f ms"
          % (median_call_ms(ctx, lambda: wall(march)), median_call_ms(ctx, lambda: wall(chained))))


if __name__ == "__main__":
    main()
