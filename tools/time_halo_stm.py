#!/usr/bin/env python3
"""Time the phase-to-phase STMs on the device (lto_halo_stm_batch): 4 096 orbits x 4 phases x 2 horizons (0.5 and 1.0
periods) -- packaged orbit 1 and copies of it with x0 moved by up to 1e-6, each with orbit 1's period, so that every group does
its own arithmetic -- and one orbit alone, DOP853 at 1e-13: `lto_last_call_ms` (entry to return of the host-pointer call: uploads,
the launch, downloads) and `lto_last_kernel_ms` (the kernel alone), median of 5 calls after 2 warm-ups.  The yardstick is
`lto_halo_table_batch` with n_samples = 2 on the same orbits: the same group form over one period, without the coast and with one
record per orbit instead of four; its call does not time its kernel alone, so the ratio is taken call to call.  The gains call (lto_stationkeep_target_gains_batch) on the 16 384 records follows."""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU  # noqa: E402

ORBITS, N_PHASE, HORIZONS = 4096, 4, (0.5, 1.0)


def median_ms(ctx, fn, reps=5, warm=2):
    """(median lto_last_call_ms, median lto_last_kernel_ms, smallest and largest lto_last_kernel_ms) of fn."""
    out = []
    for k in range(warm + reps):
        fn()
        if k >= warm:
            out.append((ctx.last_call_ms(), ctx.last_kernel_ms()))
    return statistics.median(o[0] for o in out), statistics.median(o[1] for o in out), min(o[1] for o in out), max(o[1] for o in out)


def main(n_orbits=ORBITS):
    ctx = lto.default_context(0)
    ctx.set_timing(True)
    seed = np.asarray(synth.halo_orbits()[0][:6], dtype=float)[:, 0].copy()
    seed[[1, 3, 5]] = 0.0
    orbit = drivers.halo_orbit(seed, "x0", ctx=ctx)
    taus = np.arange(N_PHASE) / float(N_PHASE)
    integ = lto.integrator(rtol=1e-13, atol=1e-14)
    for B in (n_orbits, 1):
        s0 = np.asfortranarray(np.repeat(orbit.state0[:, None], B, axis=1))
        s0[0] += 1e-6 * np.arange(B) / max(B, 1)
        per = np.full(B, orbit.period)
        r = lto.halo_stm(s0, per, taus, HORIZONS, MU=MU, integ=integ, ctx=ctx)
        call, kern, lo, hi = median_ms(ctx, lambda: lto.halo_stm(s0, per, taus, HORIZONS, MU=MU, integ=integ, ctx=ctx))
        rec = B * N_PHASE
        print("%d orbits x %d phases x %d horizons: lto_last_call_ms %.3f, kernel %.3f ms (%.3f .. %.3f over the calls) = %.2f us per record; status 0 for %d of %d "
              "records, %.1f accepted and %.1f rejected steps per record"
              % (B, N_PHASE, len(HORIZONS), call, kern, lo, hi, 1e3 * kern / rec, int(np.count_nonzero(r.status == 0)), rec, r.accepted.mean(),
                 r.rejected.mean()))
        t = lto.halo_table(s0, per, 2, MU=MU, integ=integ, ctx=ctx)
        ycall = median_ms(ctx, lambda: lto.halo_table(s0, per, 2, MU=MU, integ=integ, ctx=ctx))[0]
        print("yardstick, lto_halo_table_batch with n_samples = 2 on the same %d orbits: lto_last_call_ms %.3f = %.2f us per orbit; status 0 "
              "for %d; the STM call per record against it, call to call: %.2f"
              % (B, ycall, 1e3 * ycall / B, int(np.count_nonzero(np.atleast_1d(t.status) == 0)), call / rec / (ycall / B)))
        g = lto.stationkeep_target_gains(r.Phi, ctx=ctx)
        gcall, gkern = median_ms(ctx, lambda: lto.stationkeep_target_gains(r.Phi, ctx=ctx))[:2]
        print("gains of the %d records: lto_last_call_ms %.3f, kernel %.3f ms; status 0 for %d" % (rec, gcall, gkern,
                                                                                                  int(np.count_nonzero(g.status == 0))))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else ORBITS)
