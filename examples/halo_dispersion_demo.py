#!/usr/bin/env python3
"""Monte-Carlo dispersion of the Earth-Moon L2 halo -> halo transfer, on the GPU.

The demo's p = 2 (minimum energy) solution of halo_transfer_demo.py, then its thrust history flown OPEN LOOP from 4 096 starts
around the nominal one (drivers.dispersion -> lto_control_replay_batch): Gaussian injection errors of 1 km and 1 cm/s
per axis, lambda_v(t) of the solution as a natural cubic spline over 257 even knots, every start integrated knot interval by knot
interval in one library call.  Prints the nominal replay's miss at the arrival node and the 50th, 95th and 99th percentiles of
the dispersed misses.  The transfer is 20 days along an unstable orbit family and nothing corrects the flight: the misses show
how fast an injection error grows, which is what a corrector would have to take out.

  python examples/halo_dispersion_demo.py [n_samples] [--guided [update_every]] [--mass] [--covariance]

With --guided the same starts are also flown with neighbouring-extremal feedback (drivers.dispersion_guided ->
lto_guidance_gains_batch, lto_guided_flight_batch): the costate is reset from the feedback gains at every
update_every-th node of the solution (default 1), and the open-loop and guided percentiles are printed side by side with the
dv the feedback costs over the nominal's.

With --mass the transfer is the variable-mass one (14 rows, m0 = 1000 kg, Isp = 2000 s, free final mass:
drivers.multiShoot_CRTBP_indirect_mass from the lifted p = 2 solution), the replay carries the mass, and --guided flies it through
drivers.dispersion_guided_mass (lto_guidance_gains_mass_batch, lto_guided_flight_mass_batch): the table gains the
propellant the feedback costs over the nominal's, in kg, read off the integrated mass.

With --covariance the guided flight's arrival sigmas come from the linear covariance as well (drivers.covariance_guided /
covariance_guided_mass -> lto_guidance_covariance_batch): first beside the sample sigmas of dispersion_guided at the
same settings (navigation errors of 0.1 km and 1 mm/s per axis at every update), then as a table of arrival sigmas over three
navigation sigmas x three update cadences, all nine from one call and without sampling noise.
"""
import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU, day  # noqa: E402

NAV_KM = (0.03, 0.1, 0.3)          # the table of --covariance: navigation sigma per position axis, 1e-2 of it in m/s per velocity axis
CADENCES = (1, 3, 10)


def covariance(ctx, XC, t, prm, n_samples, sigma_r_km, sigma_v_ms, seed, update_every, mass, verbose=True):
    """The arrival sigmas of the guided flight from the linear covariance beside those of n_samples drawn flights at the same
    settings, and the table over NAV_KM x CADENCES from one call.  Returns (the comparison's covariance dict, the Monte Carlo's
    dict, the table's dict)."""
    cov_call = drivers.covariance_guided_mass if mass else drivers.covariance_guided
    mc_call = drivers.dispersion_guided_mass if mass else drivers.dispersion_guided
    nav_r, nav_v = 0.1, 1e-3
    t0 = time.perf_counter()
    one = cov_call(ctx, XC, t, prm, sigma_r_km, sigma_v_ms, update_every=update_every, nav_sigma_r_km=nav_r, nav_sigma_v_ms=nav_v)
    wall_c = time.perf_counter() - t0
    t0 = time.perf_counter()
    mc = mc_call(ctx, XC, t, prm, n_samples, sigma_r_km, sigma_v_ms, seed, update_every=update_every, nav_sigma_r_km=nav_r,
                 nav_sigma_v_ms=nav_v, nav_seed=seed + 1)
    wall_m = time.perf_counter() - t0
    ok = np.asarray(mc["status"]) == 0
    ok[0] = False                                       # sample 0 is the undisturbed one
    d = mc["x_final"][:6, ok] - XC[:6, -1:]
    s_r = float(np.sqrt(np.mean(np.sum(d[0:3] ** 2, axis=0)))) * DU
    s_v = float(np.sqrt(np.mean(np.sum(d[3:6] ** 2, axis=0)))) * DU / TU * 1e3
    t0 = time.perf_counter()
    table = cov_call(ctx, XC, t, prm, sigma_r_km, sigma_v_ms, update_every=np.array(CADENCES)[None, :],
                     nav_sigma_r_km=np.array(NAV_KM)[:, None], nav_sigma_v_ms=1e-2 * np.array(NAV_KM)[:, None])
    wall_t = time.perf_counter() - t0
    if verbose:
        print("linear covariance, navigation sigma %.3g km and %.3g m/s per axis, an update every %d node(s): arrival sigma (RSS)" % (
            nav_r, nav_v, update_every))
        print("  covariance (%.1f ms)            %11.4g km  %11.4g m/s   largest principal %.4g km%s" % (
            wall_c * 1e3, one["miss_r_km_rss"], one["miss_v_ms_rss"], one["miss_r_km_max"],
            "   final mass %.4g kg" % one["sigma_mf_kg"] if mass else ""))
        print("  %d drawn flights (%.1f ms)  %11.4g km  %11.4g m/s   sampling noise %.1f %%" % (
            int(ok.sum()), wall_m * 1e3, s_r, s_v, 100.0 / np.sqrt(2.0 * max(int(ok.sum()), 1))))
        print("arrival sigma [km] / [m/s] over navigation sigma x update cadence, one call (%.1f ms):" % (wall_t * 1e3))
        print("  nav [km]  " + "".join("      every %-2d         " % c for c in CADENCES))
        for i, nav in enumerate(NAV_KM):
            print("  %8.3g  " % nav + "".join("  %9.4g / %-9.4g" % (table["miss_r_km_rss"][i, j], table["miss_v_ms_rss"][i, j])
                                              for j in range(len(CADENCES))))
    return one, mc, table


def main(n_samples=4096, sigma_r_km=1.0, sigma_v_ms=0.01, seed=0, n_knots=257, verbose=True, guided=None, mass=False, Isp=2000.0,
         with_covariance=False):
    spec = importlib.util.spec_from_file_location("halo_demo", os.path.join(ROOT, "examples", "halo_transfer_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    XC, t, _, flag = demo.solve_p2(verbose=False)
    if flag != 0:
        raise RuntimeError("the p = 2 solve did not converge (status %d)" % flag)
    ctx = lto.default_context(0)
    prm = (MU, DU, TU, 10.0, 1e3, 1.0, 2.0, 1.0)
    if mass:
        XC, _, flag = drivers.multiShoot_CRTBP_indirect_mass(drivers.lift_to_mass(XC, 1e3), t, MU, DU, TU, XC.shape[1], Isp, 10.0, False,
                                                             False, 50, 2.0, 1.0, verbose=False)
        if flag != 0:
            raise RuntimeError("the variable-mass p = 2 solve did not converge (status %d)" % flag)
        prm = (MU, DU, TU, 10.0, Isp, 1.0, 2.0, 1.0)
    nominal = drivers.fly_control(ctx, XC, t, prm, n_knots=n_knots)
    t0 = time.perf_counter()
    out = drivers.dispersion(ctx, XC, t, prm, n_samples, sigma_r_km, sigma_v_ms, seed, n_knots=n_knots)
    wall = time.perf_counter() - t0
    if verbose:
        pc = out["percentiles"]
        print("p = 2 transfer%s, tof %.3f days, %d knots; nominal replay: miss %.4g km, %.4g m/s, dv %.4f m/s" % (
            " with variable mass (Isp %g s, propellant %.4f kg)" % (Isp, XC[6, 0] - XC[6, -1]) if mass else "",
            (t[-1] - t[0]) * TU / day, n_knots, nominal["miss_r_km"][0], nominal["miss_v_ms"][0], nominal["dv_ms"][0]))
        print("%d starts, sigma %.3g km and %.3g m/s per axis, in %.1f ms; %d of them with status 0" % (
            n_samples, sigma_r_km, sigma_v_ms, wall * 1e3, int((out["status"] == 0).sum())))
        print("  percentile   miss [km]    miss [m/s]")
        for q in (50, 95, 99):
            print("  %9d  %11.4g  %12.4g" % (q, pc["miss_r_km"][q], pc["miss_v_ms"][q]))
    cov = None
    if with_covariance:
        cov = covariance(ctx, XC, t, prm, n_samples, sigma_r_km, sigma_v_ms, seed, guided or 1, mass, verbose)
    if guided is None:
        return (nominal, out) if cov is None else (nominal, out, cov)
    t0 = time.perf_counter()
    g = (drivers.dispersion_guided_mass if mass else drivers.dispersion_guided)(ctx, XC, t, prm, n_samples, sigma_r_km, sigma_v_ms, seed,
                                                                                update_every=guided)
    wall = time.perf_counter() - t0
    if verbose:
        pg = g["percentiles"]
        print("guided, an update every %d node(s) of %d: gains and %d flights in %.1f ms; %d of them with status 0; nominal dv %.4f m/s" % (
            guided, XC.shape[1], n_samples, wall * 1e3, int((g["status"] == 0).sum()), g["dv_nominal_ms"]))
        if mass:
            print("  nominal propellant %.6f kg (the guided flight of the nominal start)" % g["propellant_nominal_kg"])
        print("  percentile   open loop [km]  [m/s]      guided [km]     [m/s]   dv excess [m/s]%s" % ("  propellant excess [kg]" if mass else ""))
        for q in (50, 95, 99):
            print("  %9d  %14.4g  %9.4g  %12.4g  %9.4g  %12.4g%s" % (q, pc["miss_r_km"][q], pc["miss_v_ms"][q], pg["miss_r_km"][q],
                                                                      pg["miss_v_ms"][q], pg["dv_excess_ms"][q],
                                                                      "  %18.4g" % pg["propellant_excess_kg"][q] if mass else ""))
    return (nominal, out, g) if cov is None else (nominal, out, g, cov)


if __name__ == "__main__":
    args = sys.argv[1:]
    guided = None
    if "--guided" in args:
        i = args.index("--guided")
        guided = int(args[i + 1]) if i + 1 < len(args) and args[i + 1].isdigit() else 1
        del args[i:i + (2 if i + 1 < len(args) and args[i + 1].isdigit() else 1)]
    mass = "--mass" in args
    if mass:
        args.remove("--mass")
    with_covariance = "--covariance" in args
    if with_covariance:
        args.remove("--covariance")
    main(int(args[0]) if args else 4096, guided=guided, mass=mass, with_covariance=with_covariance)
