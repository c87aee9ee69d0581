#!/usr/bin/env python3
"""A family of Earth-Moon L2 halo orbits made on the GPU, and a transfer between two of its members.

The packaged orbit 1 is corrected (drivers.halo_orbit: the differential corrector and one revolution with the state-transition
matrix, both on the device), then the family is marched in x0 to the packaged orbit 2's x0 in 8 steps
(drivers.halo_family: natural-parameter continuation with a secant predictor) and every member's period, Jacobi constant and
stability indices are printed.  With --fill K, K more members are corrected between each neighbouring pair in one device call.
Last, the direct demo transfer (30 nodes, 20 days, flagEnd = false; examples/halo_direct_demo.py) is solved between the tables
of the first and the last member -- two GENERATED orbits -- and, for comparison, between the packaged tables.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402


def transfer(t0s, X0s, tfs, Xfs, ctx, n=30, tof_days=20.0, tau1=0.75):
    """The direct demo solve from the ballistic stacked guess; (status, iterations, max |defect|)."""
    tof = 0.5 * tof_days * lto.day / TU
    X, t, tau1, tau2 = drivers.stacked_guess(n, tof, tof, tau1, t0s, X0s, tfs, Xfs, MU, ctx=ctx)
    out = drivers.multiShoot_CRTBP_direct(X, np.zeros((3, n)), tau1, tau2, t, np.zeros(3), np.zeros(3), MU, DU, TU, n, 10, 1000.0, 2000.0,
                                          t0s, X0s, tfs, Xfs, False, False, 0.0, False, 100, verbose=False)
    last = drivers.multiShoot_CRTBP_direct.last
    return last["status"], last["iterations"], float(np.abs(out[7]).max())


def main(fill=0, steps=8):
    ctx = lto.default_context(0)
    tabs = [np.asarray(tb[:6], dtype=float) for tb in synth.halo_orbits()]
    seed = tabs[0][:, 0].copy()
    seed[[1, 3, 5]] = 0.0
    first = drivers.halo_orbit(seed, "x0", ctx=ctx)
    print("orbit 1 from the packaged seed: status %d after %d Newton steps, against the packaged table %.2e"
          % (first.status, first.iterations, np.abs(first.states - tabs[0]).max()))
    values = np.linspace(tabs[0][0, 0], tabs[1][0, 0], steps + 1)[1:]
    fam = drivers.halo_family(first.state0, values, hold="x0", ctx=ctx)
    members = np.column_stack([first.state0, fam.states])
    periods = np.concatenate([[first.period], fam.period])
    tb = lto.halo_table(members, periods, 100, ctx=ctx)
    print("  k        x0              z0              vy0             P          C         nu_1        nu_2   steps  closure")
    for k in range(members.shape[1]):
        print(" %2d  %.12f %.12f %.12f %.9f %.9f %10.6f %11.6f   %d    %.1e" % (
            k, members[0, k], members[2, k], members[4, k], periods[k], tb.jacobi[0, k], tb.nu[0, k], tb.nu[1, k],
            first.iterations if k == 0 else fam.iterations[k - 1], tb.closure[k]))
    print("last member against the packaged orbit 2: start %.2e, table %.2e"
          % (np.abs(members[[0, 2, 4], -1] - tabs[1][[0, 2, 4], 0]).max(), np.abs(tb.X[:, :, -1] - tabs[1]).max()))
    if fill:
        f = drivers.halo_family_fill(members, fill, ctx=ctx)
        print("fill: %d members between the pairs in one call (%.3f ms), %d converged, at most %d Newton steps"
              % (f.status.size, ctx.last_call_ms(), int(np.count_nonzero(f.status == 0)), int(f.iterations.max())))
    st, it, d = transfer(tb.times, tb.X[:, :, 0], tb.times, tb.X[:, :, -1], ctx)
    print("direct transfer between the generated orbits: status %d after %d iterations, max defect %.2e" % (st, it, d))
    times = np.linspace(0.0, 1.0, 100)
    st, it, d = transfer(times, tabs[0], times, tabs[1], ctx)
    print("direct transfer between the packaged tables:  status %d after %d iterations, max defect %.2e" % (st, it, d))


if __name__ == "__main__":
    main(fill=int(sys.argv[sys.argv.index("--fill") + 1]) if "--fill" in sys.argv else 0)
