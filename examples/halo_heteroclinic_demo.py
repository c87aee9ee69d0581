#!/usr/bin/env python3
"""Earth-Moon L1 -> L2 between planar Lyapunov orbits of ONE Jacobi constant: orbits made to an energy on the device, their tubes
matched on x = 1 - MU, the best pair refined, and the direct demo transfer started from its arcs.

  1. drivers.lyapunov_seed(1 | 2, 1e-2): the linear seeds;  2. hotpath.halo_correct (planar): the two orbits, each at its own C;
  3. drivers.matched_orbits: both marched to the common C (default 3.15) in one device call and tabled;
  4. drivers.manifold_connections: L1's unstable tube against L2's stable tube, 64 phases, eps = 1e-6;
  5. drivers.manifold_connection_refine: four levels of 16 phases round the best pair;
  6. drivers.manifold_guess: the pair's two arcs as a 30-node guess;
  7. the direct demo's solve (halo_direct_demo.py: nsteps = 10, Isp = 2000 s, 1000 kg, frozen ends at the pair's phases, zero
     thrust as the control guess, at most 100 iterations).

Usage: halo_heteroclinic_demo.py [C]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402


def main(C=3.15, n_phase=64, levels=4, n_refine=16, n_nodes=30):
    ctx = lto.default_context(0)
    seeds = np.array([drivers.lyapunov_seed(w, 1e-2, MU)[0] for w in (1, 2)]).T
    own = lto.halo_correct(seeds, "planar", ctx=ctx)
    for k in range(2):
        print("L%d Lyapunov orbit from the linear seed: status %d after %d steps, P = %.9f TU, C = %.9f" % (
            k + 1, own.status[k], own.iterations[k], own.period[k], drivers._jacobi_of(own.state[:, k], MU)))
    t0 = time.perf_counter()
    orbits = drivers.matched_orbits(own.state, C, n_steps=8, planar=True, ctx=ctx)
    for k, o in enumerate(orbits):
        print("  at C = %.6f: status %d, x0 = %.13f, vy0 = %.13f, P = %.12f TU, C - C* = %+.1e, closure %.1e, nu = (%.4f, %.4f)" % (
            C, o.status, o.state0[0], o.state0[4], o.period, o.jacobi[0] - C, o.closure, o.nu[0], o.nu[1]))
    print("matched_orbits (the march of 8 steps and the tables, two device calls): %.3f s" % (time.perf_counter() - t0))
    if any(o.status != 0 for o in orbits):
        return {"orbits": orbits}
    con = drivers.manifold_connections(orbits[0], orbits[1], n_phase=n_phase, eps=1e-6, k=5, ctx=ctx)
    print("the best connections of L1's unstable and L2's stable tube on x = 1 - MU (%d phases):" % n_phase)
    for i, c in enumerate(con):
        print("  %2d. dr %9.1f km, dv %8.2f m/s   tau1 %.4f %s (%.2f days) -> tau2 %.4f %s (%.2f days)" % (
            i + 1, c.dr_km, c.dv_ms, c.tau1, c.branch1, c.t1 * TU / lto.day, c.tau2, c.branch2, -c.t2 * TU / lto.day))
    res = {"orbits": orbits, "connections": con}
    if not con:
        return res
    fine = drivers.manifold_connection_refine(orbits[0], orbits[1], con[0], levels=levels, n_phase=n_refine, spacing=1.0 / n_phase, ctx=ctx)
    for i, c in enumerate(fine):
        print("  level %d: dr %10.3f km, dv %9.4f m/s   tau1 %.8f, tau2 %.8f" % (i + 1, c.dr_km, c.dv_ms, c.tau1, c.tau2))
    res["refined"] = fine
    best = fine[-1]
    X, t, tau1, tau2 = drivers.manifold_guess(best, n_nodes, ctx=ctx)
    tables = (orbits[0].times, orbits[0].states, orbits[1].times, orbits[1].states)
    t0 = time.perf_counter()
    out = drivers.multiShoot_CRTBP_direct(X, np.zeros((3, n_nodes)), tau1, tau2, t, np.zeros(3), np.zeros(3), MU, DU, TU, n_nodes, 10, 1000.0,
                                          2000.0, *tables, False, False, 0.0, False, 100, verbose=False)
    last = drivers.multiShoot_CRTBP_direct.last
    it = last["iterations"]
    cost = float(last["history"][1, it - 1]) if it > 0 else float("nan")
    defect = float(np.abs(out[7]).max())
    print("direct from the refined pair: tf = %.2f days, status %d after %d iterations, max defect %.2e, cost %.6e, max thrust %.3e N (%.2f s)"
          % (t[-1] * TU / lto.day, last["status"], it, defect, cost, np.linalg.norm(out[1], axis=0).max(), time.perf_counter() - t0))
    res["solve"] = {"status": last["status"], "iterations": it, "max_defect": defect, "cost": cost}
    return res


if __name__ == "__main__":
    main(C=float(sys.argv[1]) if len(sys.argv) > 1 else 3.15)
