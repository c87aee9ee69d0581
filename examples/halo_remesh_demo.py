#!/usr/bin/env python3
"""Mesh re-distribution of the halo -> halo transfer (lto_indirect_remesh_batch).

The demo transfer (halo_transfer_demo.py) is taken down the rho ladder 1, 1/2, 1/4, ... on its uniform 30-node grid; the last level
is then re-meshed so that every segment takes the same share of the integrator's trial steps, and re-solved on the new grid.
Printed: max / mean / total trial steps per defect sweep before and after, and the defect- and STM-sweep kernel times on both grids.

With --mass the ladder's last level is lifted to the 14-row variable-mass system (drivers.lift_to_mass), solved there with a free
final mass, re-meshed (lto_indirect_remesh_mass_batch) and the trial steps and the propellant before and after are
printed.

usage: halo_remesh_demo.py [rho_target] [n_new] [passes]
       halo_remesh_demo.py --mass [Isp]
"""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402

MASS, THRUST = 1e3, 0.05
RHO_TARGET = 1.0 / 32


def params(rho):
    return lto.make_params(MU, DU, TU, THRUST, MASS, 1.0, 1.0, rho)


def rho_ladder(rho_target=RHO_TARGET, verbose=False, seed=0):
    """The demo's p = 2 transfer, then p = 1 at 0.05 N, then rho halved level by level down to rho_target, every level started from
    the one before on the same uniform grid.  Returns (t, [(rho, XC)], ...) with every converged level, rho = 1 first."""
    spec = importlib.util.spec_from_file_location("halo_demo_remesh", os.path.join(ROOT, "examples", "halo_transfer_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    XC, t, _, flag = demo.solve_p2(seed=seed, verbose=verbose)
    if flag != 0:
        raise RuntimeError("the p = 2 solve did not converge")
    n = t.size
    XC, _, flag = drivers.multiShoot_CRTBP_indirect(XC, t, MU, DU, TU, n, MASS, THRUST, False, False, 30, 1.0, 1.0, verbose=verbose)
    if flag != 0:
        raise RuntimeError("the p = 1 solve did not converge")
    levels = [(1.0, np.asfortranarray(XC))]
    rho = 1.0
    while rho > rho_target:
        nxt = max(rho / 2, rho_target)
        Xn, _, st, _, _ = lto.indirect_solve(levels[-1][1], t, params(nxt), None, False, 30)
        if st != 0:
            Xn, _, st = drivers.reduceFuel_indirect(levels[-1][1], t, MU, DU, TU, n, MASS, THRUST, rho, nxt, verbose=verbose)
        if st != 0:
            break
        rho = nxt
        levels.append((rho, np.asfortranarray(Xn)))
    return np.asarray(t, dtype=np.float64), levels


def stats(steps):
    return "max %3d  mean %6.2f  total %5d" % (steps.max(), steps.mean(), steps.sum())


def sweep_times(XC, t, prm, ctx, reps=5):
    """Kernel time (lto_set_timing) of one defect sweep and one STM sweep on this grid: the fastest of `reps`, in microseconds."""
    ctx.set_timing(True)
    d = s = np.inf
    for _ in range(reps):
        lto.indirect_defectCalc(XC, t, prm, ctx=ctx)
        d = min(d, ctx.last_kernel_ms())
        lto.indirect_stm(XC, t, prm, ctx=ctx)
        s = min(s, ctx.last_kernel_ms())
    ctx.set_timing(False)
    return 1e3 * d, 1e3 * s


def main(rho_target=RHO_TARGET, n_new=None, passes=2):
    ctx = lto.default_context(0)
    t, levels = rho_ladder(rho_target)
    rho, XC = levels[-1]
    n = t.size
    n_new = n_new or n
    print("rho ladder: " + ", ".join("%g" % r for r, _ in levels))
    r = lto.indirect_remesh(XC, t, params(rho), n_new=n_new, passes=passes, ctx=ctx)
    print("rho = %g, %d -> %d nodes, %d passes: status %d after %d iterations, max |defect| %.2e"
          % (rho, n, n_new, passes, r.status, r.iterations, np.abs(r.defect).max()))
    print("trial steps per defect sweep, old grid: " + stats(r.steps_before))
    print("trial steps per defect sweep, new grid: " + stats(r.steps_after))
    print("segment lengths (TU), old grid: %.4f everywhere; new grid: min %.4f  max %.4f" % (t[1] - t[0], np.diff(r.t_out).min(), np.diff(r.t_out).max()))
    if r.status == 0:
        d0, s0 = sweep_times(XC, t, params(rho), ctx)
        d1, s1 = sweep_times(r.XC_out, r.t_out, params(rho), ctx)
        print("defect sweep: %.1f -> %.1f us;  STM sweep: %.1f -> %.1f us" % (d0, d1, s0, s1))
    return r


def main_mass(Isp=2000.0, rho_target=RHO_TARGET, n_new=None, passes=2):
    ctx = lto.default_context(0)
    t, levels = rho_ladder(rho_target)
    rho, XC12 = levels[-1]
    n = t.size
    n_new = n_new or n
    XC, _, flag = drivers.multiShoot_CRTBP_indirect_mass(drivers.lift_to_mass(XC12, MASS), t, MU, DU, TU, n, Isp, THRUST, False, False,
                                                         30, 1.0, rho, verbose=False)
    if flag != 0:
        raise RuntimeError("the variable-mass solve did not converge (status %d)" % flag)
    prm = lto.make_params(MU, DU, TU, THRUST, Isp, 1.0, 1.0, rho)
    r = lto.indirect_remesh_mass(XC, t, prm, n_new=n_new, passes=passes, ctx=ctx)
    print("variable mass, Isp = %g s, rho = %g, %d -> %d nodes, %d passes: status %d after %d iterations, max |defect| %.2e"
          % (Isp, rho, n, n_new, passes, r.status, r.iterations, np.abs(r.defect).max()))
    print("trial steps per defect sweep, old grid: " + stats(r.steps_before))
    print("trial steps per defect sweep, new grid: " + stats(r.steps_after))
    a0 = drivers.thrust_arcs_mass(XC, t, MU, DU, TU, Isp, THRUST, 1.0, rho, ctx=ctx)
    print("propellant, old grid: %.6f kg (final mass %.6f kg)" % (a0["propellant_kg"], a0["mass_final_kg"]))
    if r.status == 0:
        a1 = drivers.thrust_arcs_mass(r.XC_out, r.t_out, MU, DU, TU, Isp, THRUST, 1.0, rho, ctx=ctx)
        print("propellant, new grid: %.6f kg (final mass %.6f kg), relative difference %.2e"
              % (a1["propellant_kg"], a1["mass_final_kg"], abs(a1["propellant_kg"] - a0["propellant_kg"]) / a0["propellant_kg"]))
    return r


if __name__ == "__main__":
    a = sys.argv[1:]
    if a and a[0] == "--mass":
        main_mass(float(a[1]) if len(a) > 1 else 2000.0)
        sys.exit(0)
    main(float(a[0]) if a else RHO_TARGET, int(a[1]) if len(a) > 1 else None, int(a[2]) if len(a) > 2 else 2)
