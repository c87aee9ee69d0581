#!/usr/bin/env python3
"""Cost versus time of flight of the Earth-Moon L2 halo -> halo transfer, on the GPU.

The demo's p = 2 (minimum energy) solution of halo_transfer_demo.py, then addTimeFinal (src/HelperFunctions.jl:196-250) for 32
extra times of flight from 0.25 to 8 days in ONE library call (drivers.tf_sweep -> lto_indirect_add_time_batch): every guess is
re-meshed from a ballistic coast along the arrival halo, snapped onto the orbit table and re-solved by the fixed-end indirect
loop, side by side.  Prints status, iterations, the arrival phase tau* and the cost (Delta-v of the control law) per Delta-t.

  python examples/halo_tf_sweep.py --mass [Isp]

does the same on the 14-row variable-mass system: the p = 2 solution is lifted to 1000 kg, solved at the given Isp
(default 2000 s) with a free final mass, and drivers.tf_sweep_mass -> lto_indirect_add_time_mass_batch gives the propellant in
kilograms, read off the integrated mass, against the time of flight.
"""
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU, day  # noqa: E402


def main(n_dt=32, verbose=True):
    spec = importlib.util.spec_from_file_location("halo_demo", os.path.join(ROOT, "examples", "halo_transfer_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    XC, t, _, flag = demo.solve_p2(verbose=False)
    if flag != 0:
        raise RuntimeError("the p = 2 solve did not converge (status %d)" % flag)
    tab = synth.halo_orbits()[1][:6]
    times = np.linspace(0.0, 1.0, tab.shape[1])
    dts = np.linspace(0.25, 8.0, n_dt) * day / TU
    t0 = time.perf_counter()
    out = drivers.tf_sweep(XC, t, dts, MU, DU, TU, 1e3, 10.0, 2.0, 1.0, times, tab, maxIter=30)
    wall = time.perf_counter() - t0
    if verbose:
        print("p = 2 transfer, tof %.3f days; %d time-of-flight changes in %.1f ms" % ((t[-1] - t[0]) * TU / day, n_dt, wall * 1e3))
        print("  dt [days]  tof [days]  status  iters    tau*   max|defect|   cost [m/s]")
        for k in range(n_dt):
            print("  %9.3f  %10.3f  %6d  %5d  %6.3f  %12.3e  %11.4f" % (
                dts[k] * TU / day, out["tof"][k] * TU / day, out["status"][k], out["iterations"][k], out["tau"][k],
                out["max_defect"][k], out["cost"][k] * DU * 1e3 / TU))
    return out


def main_mass(isp=2000.0, n_dt=32, verbose=True):
    spec = importlib.util.spec_from_file_location("halo_demo", os.path.join(ROOT, "examples", "halo_transfer_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    XC, t, _, flag = demo.solve_p2(verbose=False)
    if flag != 0:
        raise RuntimeError("the p = 2 solve did not converge (status %d)" % flag)
    n = XC.shape[1]
    X14, _, flag = drivers.multiShoot_CRTBP_indirect_mass(drivers.lift_to_mass(XC, 1e3), t, MU, DU, TU, n, isp, 10.0, False, False, 50,
                                                          2.0, 1.0, verbose=False)
    if flag != 0:
        raise RuntimeError("the variable-mass solve did not converge (status %d)" % flag)
    tab = synth.halo_orbits()[1][:6]
    times = np.linspace(0.0, 1.0, tab.shape[1])
    dts = np.linspace(0.25, 8.0, n_dt) * day / TU
    t0 = time.perf_counter()
    out = drivers.tf_sweep_mass(X14, t, dts, MU, DU, TU, isp, 10.0, 2.0, 1.0, times, tab, maxIter=30)
    wall = time.perf_counter() - t0
    if verbose:
        print("p = 2 transfer at Isp = %g s, tof %.3f days, propellant %.6f kg of %.1f; %d time-of-flight changes in %.1f ms" % (
            isp, (t[-1] - t[0]) * TU / day, X14[6, 0] - X14[6, -1], X14[6, 0], n_dt, wall * 1e3))
        print("  dt [days]  tof [days]  status  iters    tau*   max|defect|   cost [m/s]  propellant [kg]  final mass [kg]")
        for k in range(n_dt):
            print("  %9.3f  %10.3f  %6d  %5d  %6.3f  %12.3e  %11.4f  %15.6f  %15.6f" % (
                dts[k] * TU / day, out["tof"][k] * TU / day, out["status"][k], out["iterations"][k], out["tau"][k],
                out["max_defect"][k], out["cost"][k] * DU * 1e3 / TU, out["propellant_kg"][k], out["mass_final_kg"][k]))
    return out


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--mass":
        main_mass(float(sys.argv[2]) if len(sys.argv) > 2 else 2000.0)
    else:
        main()
