#!/usr/bin/env python3
"""Earth-Moon L2 halo -> halo: the invariant-manifold tubes of the two packaged orbits, their closest approaches on a section, and
the direct demo transfer started from the best pair's arcs -- beside the stacked guess of the reference demos.

Both orbits are corrected and tabled on the device (drivers.halo_orbit from the packaged seeds, hold x0), which hands back their
monodromy matrices.  drivers.manifold_connections flies the unstable tube of orbit 1 and the stable tube of orbit 2 (64 phases, both
branches, eps = 1e-6) to x = 1 - MU and matches them; the ten best pairs are printed with their gap in km and m/s.  The best one
becomes a 30-node guess (drivers.manifold_guess) for the direct demo's solve (halo_direct_demo.py: nsteps = 10, Isp = 2000 s,
1000 kg, frozen ends at the pair's phases, zero thrust as the control guess, at most 100 iterations); the same solve from
drivers.stacked_guess (10 days ballistically on each orbit from tau1 = 0.75) is printed beside it: iterations, final defect, cost.

--section y  uses the plane y = 0 (second crossing) instead;  --eps E, --phases N change the tubes."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402


def _solve(tag, X, t, tau1, tau2, tables, maxIter=100):
    n = X.shape[1]
    t0 = time.perf_counter()
    out = drivers.multiShoot_CRTBP_direct(X, np.zeros((3, n)), tau1, tau2, t, np.zeros(3), np.zeros(3), MU, DU, TU, n, 10, 1000.0, 2000.0,
                                          *tables, False, False, 0.0, False, maxIter, verbose=False)
    last = drivers.multiShoot_CRTBP_direct.last
    it = last["iterations"]
    cost = float(last["history"][1, it - 1]) if it > 0 else float("nan")
    defect = float(np.abs(out[7]).max())
    print("%s: tf = %.2f days, status %d after %d iterations, max defect %.2e, cost %.6f, max thrust %.3f N (%.2f s)" % (
        tag, t[-1] * TU / lto.day, last["status"], it, defect, cost, np.linalg.norm(out[1], axis=0).max(), time.perf_counter() - t0))
    return {"status": last["status"], "iterations": it, "max_defect": defect, "cost": cost, "tf_days": float(t[-1] * TU / lto.day)}


def main(section="x", eps=1e-6, n_phase=64, n_nodes=30):
    ctx = lto.default_context(0)
    tabs = synth.halo_orbits()
    times = [np.linspace(0.0, 1.0, tb.shape[1]) for tb in tabs]
    orbits = []
    for k, tb in enumerate(tabs):
        seed = np.array(tb[:6, 0])
        seed[[1, 3, 5]] = 0.0
        o = drivers.halo_orbit(seed, "x0", ctx=ctx)
        orbits.append(o)
        print("orbit %d: P = %.9f TU, C = %.9f, nu = (%.4f, %.4f)" % (k + 1, o.period, o.jacobi[0], o.nu[0], o.nu[1]))
    sec, n_cross = (("x", 1.0 - MU), 1) if section == "x" else (("y", 0.0), 2)
    t0 = time.perf_counter()
    tube = drivers.halo_manifold(orbits[0], n_phase, eps=eps, section=sec, n_cross=n_cross, ctx=ctx)
    print("tubes of orbit 1 to %s = %.6f: lambda_u = %.6f, lambda_s = %.9f, %d of %d arcs reach the section, |t| %.2f .. %.2f TU" % (
        sec[0], sec[1], tube.lam[0], tube.lam[1], int(np.count_nonzero(tube.status == 0)), tube.status.size,
        np.abs(tube.t_end[tube.status == 0]).min(), np.abs(tube.t_end[tube.status == 0]).max()))
    con = drivers.manifold_connections(orbits[0], orbits[1], section=sec, n_phase=n_phase, eps=eps, n_cross=n_cross, k=10, ctx=ctx)
    print("the ten best connections of %d x %d arcs (%.2f s with the tubes):" % (2 * n_phase, 2 * n_phase, time.perf_counter() - t0))
    for i, c in enumerate(con):
        print("  %2d. dr %9.1f km, dv %8.2f m/s   tau1 %.4f %s (%.2f days) -> tau2 %.4f %s (%.2f days)" % (
            i + 1, c.dr_km, c.dv_ms, c.tau1, c.branch1, c.t1 * TU / lto.day, c.tau2, c.branch2, -c.t2 * TU / lto.day))
    tables = (times[0], tabs[0], times[1], tabs[1])
    res = {"connections": con}
    if con:
        X, t, tau1, tau2 = drivers.manifold_guess(con[0], n_nodes, ctx=ctx)
        res["manifold"] = _solve("direct from the manifold guess", X, t, tau1, tau2, tables)
    tof = 10.0 * lto.day / TU
    X, t, tau1, tau2 = drivers.stacked_guess(n_nodes, tof, tof, 0.75, *tables, MU)
    res["stacked"] = _solve("direct from the stacked guess ", X, t, tau1, tau2, tables)
    return res


def _arg(flag, default, cast=float):
    if flag not in sys.argv:
        return default
    return cast(sys.argv[sys.argv.index(flag) + 1])


if __name__ == "__main__":
    main(section=_arg("--section", "x", str), eps=_arg("--eps", 1e-6), n_phase=_arg("--phases", 64, int))
