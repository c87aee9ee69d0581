#!/usr/bin/env python3
"""Earth-Moon L2 halo -> halo low-thrust transfer by indirect multiple shooting, on the GPU.

Follows the indirect part of the reference demo (CRTBP_Multishoot_indirect_demo.jl): 30 nodes over 20 days,
trajectory-stacking initial guess (:74-115), p = 2 with adjoints-only iterations first (:178-186), then all
variables (:188-192), then p = 1 at 0.05 N (:240-247) and the rho continuation (:277-281).  The reference first runs
its direct method (JuMP/Ipopt QP, out of scope here) to smooth the stacked guess; this script goes straight to the
indirect method, so it needs a few more Newton iterations.  Every defect / Jacobian / Newton solve runs in
liblto_hip.so; random costates are seeded (the reference's are not).

--mass [Isp] (default 2000 s) continues with the variable-mass system: the p = 2 solution lifted to 14 rows, m0 = 1000 kg,
free final mass, then p = 1 and the rho continuation; m_f and the fuel used are printed per level.
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU, day  # noqa: E402


def stacked_guess(n_nodes=30, tof_days=20.0, tau1=0.75):
    """Nodes on halo 1 for the first half of the flight and on halo 2 afterwards (demo :74-115), using periodic
    interpolation of the orbit tables instead of ballistic propagation + cubic splines."""
    tof = tof_days * day / TU
    t = np.linspace(0.0, tof, n_nodes)
    tof1 = tof / 2
    T1, T2 = 99 * synth.HALO_DT[0], 99 * synth.HALO_DT[1]
    X = np.zeros((6, n_nodes))
    first = t < tof1
    X[:, first] = synth.halo_state(0, tau1 * T1 + t[first])
    # closest point of orbit 2 to the end of the first arc
    xe = synth.halo_state(0, tau1 * T1 + tof1)
    taus = np.linspace(0, T2, 2001)
    d = np.linalg.norm(synth.halo_state(1, taus) - xe[:, None], axis=0)
    tau2 = taus[np.argmin(d)]
    X[:, ~first] = synth.halo_state(1, tau2 + (t[~first] - tof1))
    return X, t


def solve_p2(seed=0, verbose=True, ops=None, n=30, mass=1e3):
    """The demo's p = 2 (minimum energy) solve, thrust unconstrained (10 N): adjoints only, then everything.
    Returns (XC [12 x n], t, defect, status)."""
    X, t = stacked_guess(n)
    rng = np.random.default_rng(seed)
    XC = np.vstack([X, 0.1 * rng.standard_normal((6, n))])
    XC[:, 1:-1] += 1e-10 * rng.standard_normal((12, n - 2))
    XC, defect, flag = drivers.multiShoot_CRTBP_indirect(XC, t, MU, DU, TU, n, mass, 10.0, False, True, 10, 2.0, 1.0, ops=ops, verbose=verbose)
    XC, defect, flag = drivers.multiShoot_CRTBP_indirect(XC, t, MU, DU, TU, n, mass, 10.0, False, False, 50, 2.0, 1.0, ops=ops, verbose=verbose)
    return XC, t, defect, flag


def mass_run(XC, t, Isp, rho_target, ctx, verbose=True, n=30, mass0=1e3):
    """Variable-mass extension: the p = 2 solution lifted to 14 rows (m0 = mass0, lambda_m = 0) and solved with the free final
    mass at the given Isp, then p = 1 at 0.05 N and the rho continuation 1/2, 1/4, ... down to rho_target.
    Returns {level: (status, max defect, m_f)}."""
    X14 = drivers.lift_to_mass(XC, mass0)
    X14, defect, flag = drivers.multiShoot_CRTBP_indirect_mass(X14, t, MU, DU, TU, n, Isp, 10.0, False, False, 50, 2.0, 1.0, verbose=verbose)
    out = {"p2": (flag, float(np.abs(defect).max()), float(X14[6, -1]))}
    print("mass, p = 2, Isp %g s: status %d, max defect %.2e, m_f %.3f kg, fuel %.3f kg" % (Isp, flag, np.abs(defect).max(), X14[6, -1], mass0 - X14[6, -1]))
    if flag != 0:
        return out
    X1, defect, flag1 = drivers.multiShoot_CRTBP_indirect_mass(X14, t, MU, DU, TU, n, Isp, 0.05, False, False, 30, 1.0, 1.0, verbose=verbose)
    out["p1"] = (flag1, float(np.abs(defect).max()), float(X1[6, -1]))
    print("mass, p = 1, rho = 1: status %d, max defect %.2e, m_f %.3f kg, fuel %.3f kg" % (flag1, np.abs(defect).max(), X1[6, -1], mass0 - X1[6, -1]))
    if flag1 != 0:
        return out
    # rho continuation 1/2, 1/4, ... down to rho_target, each level started from the one before (one device solve per level;
    # a level that does not converge in 30 iterations falls back to reduceFuel_indirect_mass's back-off from the last good level)
    rhos = []
    while (rhos[-1] if rhos else 1.0) / 2 > rho_target:
        rhos.append((rhos[-1] if rhos else 1.0) / 2)
    rhos.append(rho_target)
    X, rho_prev = X1, 1.0
    for r in rhos:
        prm = lto.make_params(MU, DU, TU, 0.05, Isp, 1.0, 1.0, r)
        Xn, Dn, st, its, _ = lto.indirect_solve(X, t, prm, None, False, 30, ctx=ctx)
        how = "%2d iterations" % its
        if st != 0:
            Xn, Dn, st = drivers.reduceFuel_indirect_mass(X, t, MU, DU, TU, n, Isp, 0.05, rho_prev, r, verbose=False)
            how = "continuation"
        out["rho=%g" % r] = (int(st), float(np.abs(Dn).max()), float(Xn[6, -1]))
        print("mass, p = 1, rho = %-9g status %d, %s, max defect %.2e, m_f %.3f kg, fuel %.3f kg"
              % (r, st, how, np.abs(Dn).max(), Xn[6, -1], mass0 - Xn[6, -1]))
        if st != 0:
            break
        X, rho_prev = Xn, r
    # arcs and mass budget of the last level reached, read off the integration (drivers.thrust_arcs_mass)
    a = drivers.thrust_arcs_mass(X, t, MU, DU, TU, Isp, 0.05, 1.0, rho_prev, ctx=ctx)
    out["arcs"] = a
    burns = ", ".join("%.3f-%.3f d" % (b0 * TU / 86400.0, b1 * TU / 86400.0) for b0, b1 in a["arcs"])
    print("mass, arcs, rho = %-9g dv %.3f m/s (rocket equation of the mass ratio %.3f m/s), burning %.3f d in %d arcs: %s"
          % (rho_prev, a["dv_ms"], a["dv_rocket_ms"], a["burn_days"], len(a["arcs"]), burns))
    print("mass, budget: propellant %.4f kg over the segments, m_f %.4f kg (last node %.4f kg)" % (a["propellant_kg"], a["mass_final_kg"], X[6, -1]))
    return out


def print_arcs(XC1, t, mass, rho_target, ctx):
    """--arcs: the burn list and dv of every rho level of the ladder (one batched call behind homotopy_solve), beside the
    trapezoid of umag over 200 samples of the dense output."""
    rhos = [1.0]
    while rhos[-1] / 2 > rho_target:
        rhos.append(rhos[-1] / 2)
    rhos.append(rho_target)
    X, _, status, _, arcs = drivers.homotopy_solve(XC1, t, MU, DU, TU, mass, 0.05, rhos, ctx=ctx, verbose=False, arcs=True)
    aL = 0.05 / mass / 1e3 * TU ** 2 / DU
    for k, r in enumerate(rhos):
        if arcs[k] is None:
            print("arcs, rho = %-9g not converged (status %d)" % (r, status[k]))
            continue
        XD, td = lto.densify(X[:, :, k], t, lto.make_params(MU, DU, TU, 0.05, mass, 1.0, 1.0, r), 200, ctx=ctx)
        u = 0.5 * (1 + np.tanh((np.linalg.norm(XD[9:12], axis=0) - 1) / (2 * r))) * aL
        trap = float(np.sum(np.diff(td) * (u[1:] + u[:-1]) / 2))
        a = arcs[k]
        burns = ", ".join("%.3f-%.3f d" % (b0 * TU / 86400.0, b1 * TU / 86400.0) for b0, b1 in a["arcs"])
        print("arcs, rho = %-9g dv %.6e DU/TU = %.3f m/s (trapezoid %.6e), burning %.3f d in %d arcs: %s"
              % (r, a["dv"], a["dv_ms"], trap, a["burn_days"], len(a["arcs"]), burns))


def main(seed=0, verbose=True, rho_target=1e-2, python_loop=False, mass_isp=None, arcs=False):
    ctx = lto.default_context(0)
    # default: every multiShoot_CRTBP_indirect call is ONE library call (lto_indirect_solve: Newton loop, line search
    # and end-state pinning on the device); --python-loop drives the same device operators from the Python mirror of
    # the reference loop.  Integrator: adaptive order-8 pair @1e-13 (the reference's setting).
    ops = drivers.HipOps(ctx) if python_loop else None
    n = 30
    mass = 1e3
    t0 = time.perf_counter()
    XC, t, defect, flag = solve_p2(seed, verbose, ops, n, mass)
    print("p = 2: status %d, max defect %.2e" % (flag, np.abs(defect).max()))
    res = {"p2": (flag, float(np.abs(defect).max()))}
    if flag == 0:
        # p = 1 (minimum fuel) at 0.05 N, rho = 1, then continuation to rho = 1e-2
        XC1, defect, flag1 = drivers.multiShoot_CRTBP_indirect(XC, t, MU, DU, TU, n, mass, 0.05, False, False, 30, 1.0, 1.0, ops=ops, verbose=verbose)
        print("p = 1, rho = 1: status %d, max defect %.2e" % (flag1, np.abs(defect).max()))
        res["p1"] = (flag1, float(np.abs(defect).max()))
        if flag1 == 0:
            XC2, defect, flag2 = drivers.reduceFuel_indirect(XC1, t, MU, DU, TU, n, mass, 0.05, 1.0, rho_target, ops=ops, verbose=verbose)
            print("rho -> %g: status %d, max defect %.2e" % (rho_target, flag2, np.abs(defect).max()))
            res["rho"] = (flag2, float(np.abs(defect).max()))
            if flag2 == 0:
                XD, td = lto.densify(XC2, t, lto.make_params(MU, DU, TU, 0.05, mass, 1.0, 1.0, rho_target), 300, ctx=ctx)
                lam = np.linalg.norm(XD[9:12], axis=0)
                thr = 0.5 * (1 + np.tanh((lam - 1) / (2 * rho_target))) * 0.05
                print("thrust profile: on %.0f %% of the flight, max %.3f N" % (100 * np.mean(thr > 0.025), thr.max()))
                if arcs:
                    print_arcs(XC1, t, mass, rho_target, ctx)
    if mass_isp is not None and flag == 0:
        res["mass"] = mass_run(XC, t, mass_isp, rho_target, ctx, verbose, n, mass)
    print("wall time %.2f s" % (time.perf_counter() - t0))
    return res


if __name__ == "__main__":
    # usage: halo_transfer_demo.py [rho_target] [-q] [--python-loop] [--mass [Isp]] [--arcs]
    argv = sys.argv[1:]
    mass_isp = None
    if "--mass" in argv:
        i = argv.index("--mass")
        mass_isp = 2000.0
        if i + 1 < len(argv) and not argv[i + 1].startswith("-"):
            mass_isp = float(argv[i + 1])
            del argv[i + 1]
        del argv[i]
    args = [a for a in argv if not a.startswith("-")]
    main(rho_target=float(args[0]) if args else 1e-2, verbose="-q" not in argv, python_loop="--python-loop" in argv, mass_isp=mass_isp,
         arcs="--arcs" in argv)
