#!/usr/bin/env python3
"""Time the station-keeping flights on the device (lto_stationkeep_flight_batch): 65 536 runs x 4 burns x 10 revolutions
of packaged orbit 1 under its Floquet-mode law, DOP853 at 1e-13, one orbit for every run (n_orb = 1), without and with navigation
and execution errors -- `lto_last_call_ms` (entry to return of the host-pointer call: uploads, the launch, downloads) and
`lto_last_kernel_ms` (the flight kernel alone), median of 5 calls after 2 warm-ups.  The per-update histories are left out
(history=False); one more line gives the call with them.  For scale, `lto_section_flight_batch` flies the same 65 536 starts
ballistically over ONE span of a quarter period (n_cross = 0): the cost of a span without the restart, the feedback and the error
reads.  Prints one line per figure and the ratio of the time per span to that yardstick."""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402

RUNS, N_MAN, N_REV, SEED = 65536, 4, 10, 0


def median_ms(ctx, fn, reps=5, warm=2):
    """(median lto_last_call_ms, median lto_last_kernel_ms) of fn."""
    out = []
    for k in range(warm + reps):
        fn()
        if k >= warm:
            out.append((ctx.last_call_ms(), ctx.last_kernel_ms()))
    return statistics.median(o[0] for o in out), statistics.median(o[1] for o in out)


def main(runs=RUNS):
    ctx = lto.default_context(0)
    ctx.set_timing(True)
    seed = np.asarray(synth.halo_orbits()[0][:6], dtype=float)[:, 0].copy()
    seed[[1, 3, 5]] = 0.0
    orbit = drivers.halo_orbit(seed, "x0", ctx=ctx)
    g = drivers.stationkeeping_gains(orbit, n_man=N_MAN, ctx=ctx)
    print("packaged orbit 1: P = %.8f TU, lambda_u = %.3f, alpha %s; gains call lto_last_call_ms %.3f"
          % (orbit.period, g.lam[0], np.array2string(g.alpha, precision=3), ctx.last_call_ms()))
    n_upd = N_MAN * N_REV
    inj, nav, exe = drivers.stationkeep_draws(runs, n_upd, 1.0, 0.01, 0.3, 0.003, 0.01, 1e-4, SEED, DU, TU)
    x0 = np.asfortranarray(g.X_ref[:, :1] + inj)
    spans = runs * n_upd

    def flight(nav=None, exe=None, history=False):
        return lto.stationkeep_flight(g.X_ref, g.dt, g.G, x0, N_REV, nav=nav, exe=exe, MU=MU, ctx=ctx, history=history)

    figures = {}
    for tag, kw in (("no errors", {}), ("nav + exe", dict(nav=nav, exe=exe)), ("nav + exe, histories", dict(nav=nav, exe=exe, history=True))):
        r = flight(**kw)
        call, kern = median_ms(ctx, lambda: flight(**kw))
        figures[tag] = (call, kern)
        print("%d runs x %d burns x %d revolutions, %s: lto_last_call_ms %.2f, kernel %.2f ms = %.1f ns per span; status 0 for %d runs, "
              "%.1f accepted and %.2f rejected steps per span, dv %.4f m/s per run (median)"
              % (runs, N_MAN, N_REV, tag, call, kern, 1e6 * kern / spans, int(np.count_nonzero(r.status == 0)),
                 r.accepted.mean() / n_upd, r.rejected.mean() / n_upd, float(np.median(r.dv_total)) * DU / TU * 1e3))
    T = np.full(runs, orbit.period / N_MAN)
    f = lto.section_flight(x0, T, n_cross=0, MU=MU, ctx=ctx)

    def yard():
        lto.section_flight(x0, T, n_cross=0, MU=MU, ctx=ctx)
    ycall, _ = median_ms(ctx, yard)
    print("yardstick, lto_section_flight_batch, the same %d starts over one span of P / %d: lto_last_call_ms %.2f = %.1f ns per span; "
          "status 0 for %d arcs" % (runs, N_MAN, ycall, 1e6 * ycall / runs, int(np.count_nonzero(f.status == 0))))
    for tag in ("no errors", "nav + exe"):
        call, kern = figures[tag]
        print("%s: per span %.1f ns by the kernel (%.1f ns by the call) against %.1f ns: ratio %.2f (%.2f)"
              % (tag, 1e6 * kern / spans, 1e6 * call / spans, 1e6 * ycall / runs, kern / spans / (ycall / runs), call / spans / (ycall / runs)))


if __name__ == "__main__":
    main(int(sys.argv[1]) if len(sys.argv) > 1 else RUNS)
