#!/usr/bin/env python3
"""Time the invariant-manifold calls on the device (lto_halo_manifold_seeds_batch, lto_section_flight_batch,
lto_state_match_batch): `lto_last_call_ms` (entry to return of the host-pointer call: uploads, launches, downloads),
median of 10 calls after 3 warm-ups.  Seeds for 1 and 256 orbits x 16 phases (the orbits: the packaged orbit 1 marched a fifth of
the way to orbit 2, hold x0, corrected and tabled on the device); flights of 1 and 65 536 arcs (those seeds' four branches at four
values of eps) to x = 1 - MU within 12 TU; a 4 096 x 4 096 match of unstable against stable section states.  Prints one line per
figure."""
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import synth  # noqa: E402


def median_call_ms(ctx, fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    return statistics.median([(fn(), ctx.last_call_ms())[1] for _ in range(reps)])


def main():
    ctx = lto.default_context(0)
    tabs = synth.halo_orbits()
    s1 = np.array(tabs[0][:6, 0])
    s1[[1, 3, 5]] = 0.0
    B = 256
    seeds = np.repeat(s1[:, None], B, axis=1)
    seeds[0] += 0.2 * (tabs[1][0, 0] - s1[0]) * np.arange(B) / float(B)
    c = lto.halo_correct(seeds, "x0", ctx=ctx)
    assert np.all(c.status == 0)
    tb = lto.halo_table(c.state, c.period, 100, ctx=ctx)
    tau = np.arange(16) / 16.0
    for nb in (1, B):
        S, P, M = np.asfortranarray(c.state[:, :nb]), c.period[:nb].copy(), np.asfortranarray(tb.M[:, :, :nb])
        r = lto.manifold_seeds(S, P, M, tau, ctx=ctx)
        ms = median_call_ms(ctx, lambda: lto.manifold_seeds(S, P, M, tau, ctx=ctx))
        print("manifold_seeds, %3d orbits x 16 phases: lto_last_call_ms %.3f, status 0 for %d orbits, |lambda_u lambda_s - 1| <= %.1e"
              % (nb, ms, int(np.count_nonzero(r.status == 0)), float(np.abs(r.lam[0] * r.lam[1] - 1.0).max())))
    starts = [lto.manifold_seeds(c.state, c.period, tb.M, tau, eps=e, ctx=ctx).starts.reshape(6, -1, order="F") for e in (1e-6, 2e-6, 4e-6, 8e-6)]
    Y = np.asfortranarray(np.concatenate(starts, axis=1))                       # 4 x (4 x 16 x 256) = 65 536 starts
    T = np.where((np.arange(Y.shape[1]) % 4) < 2, 12.0, -12.0)
    section = ("x", 1.0 - lto.MU)
    fl = lto.section_flight(Y, T, section=section, ctx=ctx)
    first = int(np.flatnonzero(fl.status == 0)[0])                               # the single arc: one that reaches the section
    for lo, n in ((first, 1), (0, Y.shape[1])):
        y, t = np.asfortranarray(Y[:, lo:lo + n]), T[lo:lo + n].copy()
        r = lto.section_flight(y, t, section=section, ctx=ctx)
        ms = median_call_ms(ctx, lambda: lto.section_flight(y, t, section=section, ctx=ctx))
        print("section_flight to x = 1 - MU, %5d arcs: lto_last_call_ms %.3f, status 0 for %d arcs, |t_end| %.2f .. %.2f, worst Jacobi drift %.1e"
              % (n, ms, int(np.count_nonzero(r.status == 0)), float(np.nanmin(np.abs(r.t_end))), float(np.nanmax(np.abs(r.t_end))),
                 float(np.nanmax(r.dC))))
    ok = fl.status == 0
    A = np.asfortranarray(fl.x_end[:, ok & (T > 0.0)][:, :4096])
    Bs = np.asfortranarray(fl.x_end[:, ok & (T < 0.0)][:, :4096])
    m = lto.state_match(A, Bs, ctx=ctx)
    ms = median_call_ms(ctx, lambda: lto.state_match(A, Bs, ctx=ctx))
    print("state_match, %d x %d: lto_last_call_ms %.3f, smallest distance %.3e" % (A.shape[1], Bs.shape[1], ms, float(np.nanmin(m.dist))))


if __name__ == "__main__":
    main()
