#!/usr/bin/env python3
"""Halo families from the mass ratio alone, on the GPU.

At L1 and at L2: the linear Lyapunov seed (drivers.lyapunov_seed, nothing but MU), the planar corrector, the planar family
followed by pseudo-arclength in the 3-unknown form until the signed determinant changes sign, the branch point by a secant on that
determinant, one step off the plane and 24 members up the southern halo branch (drivers.halo_from_lyapunov) -- with
every member's table, Jacobi constant and stability indices from one halo_table call.  Printed: the two bifurcations' C and P, the
members, the folds of x0, z0 and vy0 the march went through, and for L2 the member nearest each packaged orbit re-corrected
holding the packaged x0, with its distance to the packaged seed: the packaged orbits are members of the family that starts at MU.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402


def main(n_members=24, ds=0.02):
    ctx = lto.default_context(0)
    for which in (1, 2):
        t0 = time.perf_counter()
        # next to the L1 branch point the halo family turns fast: the kernel halves the first step there, and grow lets it come back
        br = drivers.halo_from_lyapunov(which, n_members, ds, north=False, n_samples=100, grow=2.0, ctx=ctx)
        ms = 1e3 * (time.perf_counter() - t0)
        bp, fam, tb = br.branch_point, br.family, br.table
        print("L%d: halo bifurcation of the Lyapunov family at x0 = %.10f, vy0 = %.10f, C = %.9f, P = %.9f (|det| %.1e after %d "
              "trials); the whole chain %.1f ms" % (which, bp.state[0], bp.state[4], bp.jacobi, bp.period, abs(bp.det), len(bp.trials), ms))
        print("  k        x0              z0              vy0             P          C         nu_1        nu_2     ds    steps")
        for k in range(fam.states.shape[1]):
            print(" %2d  %.12f %+.12f %.12f %.9f %.9f %10.6f %11.6f  %.4f   %d" % (
                k, fam.states[0, k], fam.states[2, k], fam.states[4, k], fam.period[k], tb.jacobi[0, k], tb.nu[0, k], tb.nu[1, k],
                fam.ds[k], fam.iterations[k]))
        print("  folds (the member after the extremum):", drivers.family_folds(fam), " further bifurcations:", drivers.family_bifurcations(fam))
        if which == 2:
            for n, tab in enumerate(synth.halo_orbits()):
                packaged = np.array(tab[:6, 0], dtype=float)
                packaged[[1, 3, 5]] = 0.0
                k = int(np.argmin(np.abs(fam.states[0] - packaged[0])))
                start = fam.states[:, k].copy()
                start[0] = packaged[0]
                got = lto.halo_correct(start, "x0", ctx=ctx)
                print("  packaged orbit %d: member %d re-corrected holding its x0 (status %d, %d steps) is %.2e from the packaged seed"
                      % (n + 1, k, got.status, got.iterations, np.abs(got.state - packaged).max()))


if __name__ == "__main__":
    main()
