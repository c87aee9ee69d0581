#!/usr/bin/env python3
"""Time the pseudo-arclength continuation on the device (lto_halo_arclength_batch): `lto_last_call_ms`, median of 10
calls after 3 warm-ups.  One family of 24 members (the southern L2 halo branch from the step off the plane, ds = 0.02), 4096 families
of 8 members (the planar L2 Lyapunov family from the Ax = 1e-2 orbit, first steps spread over 0.005 .. 0.01), and the 24-member march
as 24 one-member calls chained on the host.  Prints one line per figure."""
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers  # noqa: E402
from lowthrustopt_amd.constants import MU  # noqa: E402


def median_call_ms(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    return statistics.median([fn() for _ in range(reps)])


def main():
    ctx = lto.default_context(0)
    t0 = time.perf_counter()
    br = drivers.halo_from_lyapunov(2, 24, 0.02, north=False, ctx=ctx)
    print("halo_from_lyapunov(2, 24, 0.02, north=False): %.1f ms of wall clock, branch point C = %.9f, P = %.9f after %d trials"
          % (1e3 * (time.perf_counter() - t0), br.branch_point.jacobi, br.branch_point.period, len(br.branch_point.trials)))
    seed, tangent = br.family.states[:, 0], br.family.tangent[:, 0]
    r = lto.halo_arclength(seed, 24, 0.02, tangent, dir_is_tangent=True, ctx=ctx)

    def march():
        lto.halo_arclength(seed, 24, 0.02, tangent, dir_is_tangent=True, ctx=ctx)
        return ctx.last_call_ms()

    def chained():
        total, s, t = 0.0, seed, tangent
        for k in range(24):
            ds = float(r.ds[k])
            m = lto.halo_arclength(s, 1, ds, t, dir_is_tangent=True, ds_min=ds, ds_max=ds, ctx=ctx)
            total += ctx.last_call_ms()
            s, t = m.state[:, 0], m.tangent[:, 0]
        return total
    flights = int(r.iterations.sum()) + 24
    print("one family of 24 members in one call: lto_last_call_ms %.3f, statuses %s, %d Newton steps, %d flights"
          % (median_call_ms(march), sorted(set(r.status.tolist())), int(r.iterations.sum()), flights))
    print("the same march as 24 calls from the host: the sum of lto_last_call_ms %.3f" % median_call_ms(chained))

    def wall(fn):
        t0 = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t0)
    print("wall clock with the Python layer: one call %.3f ms, 24 calls %.3f ms"
          % (median_call_ms(lambda: wall(march)), median_call_ms(lambda: wall(chained))))

    B = 4096
    lyap = lto.halo_correct(drivers.lyapunov_seed(2, 1e-2, MU)[0], "planar", ctx=ctx)
    seeds = np.repeat(lyap.state[:, None], B, axis=1)
    ds0 = 0.005 * (1.0 + (np.arange(B) + 0.5) / B)
    up = np.array([0.0, 0.0, 1.0])
    rb = lto.halo_arclength(seeds, 8, ds0, up, planar=True, ctx=ctx)

    def many():
        lto.halo_arclength(seeds, 8, ds0, up, planar=True, ctx=ctx)
        return ctx.last_call_ms()
    ms = median_call_ms(many)
    print("%d families of 8 members: lto_last_call_ms %.3f (%.3f us per member), status 0 for %d members, iterations %d .. %d"
          % (B, ms, 1e3 * ms / (8 * B), int(np.count_nonzero(rb.status == 0)), rb.iterations.min(), rb.iterations.max()))


if __name__ == "__main__":
    main()
