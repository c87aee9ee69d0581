#!/usr/bin/env python3
"""What it costs per year to stay on a halo orbit, by Monte Carlo on the GPU.

The packaged orbit 1 is corrected and tabled on the device (drivers.halo_orbit), its stable and unstable directions are carried to
four burn phases per revolution and turned into the Floquet-mode feedback law (drivers.stationkeeping_gains: the burn is the
smallest velocity change that zeroes the unstable component of the measured deviation).  Then RUNS spacecraft, injected 1 km and
1 cm/s (1 sigma per axis) off the orbit, are flown for 6 and for 20 revolutions with execution errors of 1 % and 0.1 mm/s per axis,
at three levels of navigation error, each case in ONE call of lto_stationkeep_flight_batch (drivers.stationkeep): the yearly dv at
the 50, 95 and 99 % levels over the runs that stay within 5 000 km, the share that does not, the largest deviation, the deviation
at the end -- and beside them how long the same runs stay within 5 000 km of the orbit without control.

The law leaves the centre directions alone: a run drifts along the orbit (its period is not the orbit's) while its unstable
component stays small.  Over 6 revolutions that is harmless.  Over 20 the drift of some runs reaches hundreds of km, the deviation
from the reference point at the same TIME is then no longer a small displacement, the law reads part of it as unstable component,
burns against it, and feeds the drift: those runs leave.  Keeping the orbit for long needs the phase re-targeted as well, which this
law does not do; the 20-revolution rows show by how much.

Last, a short family of halo orbits between the packaged orbits 1 and 2 (drivers.halo_family), every member with its own law, all
members' runs in one call with one orbit per run (n_orb = n_batch), 6 revolutions: the yearly cost against the unstable multiplier
lambda_u.

With --law target-point the table is printed for both laws from the same draws: the target-point law of Howell &
Pernicka (drivers.target_point_gains) asks the position deviation to vanish at --horizons periods after every burn, weighted by
--weights against --q times |dv|^2.  It feeds the whole deviation back, the along-track part included, and keeps the runs the
Floquet-mode law loses at 20 revolutions.

  python examples/halo_stationkeeping_demo.py [runs] [--law target-point [--horizons 0.5 1.0] [--q 1e-2] [--weights 1 1]]
"""
import argparse
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU, day  # noqa: E402

SEED, N_MAN, N_REVS, N_REV_FAMILY, R_LOST_KM = 2026, 4, (6, 20), 6, 5000.0
NAV_LEVELS = ((0.1, 0.001), (1.0, 0.01), (10.0, 0.1))       # km, m/s, 1 sigma per axis
MS = DU / TU * 1e3


def main(runs=4096, law="floquet", horizons=(0.5, 1.0), q=1e-2, weights=None):
    ctx = lto.default_context(0)
    tabs = [np.asarray(tb[:6], dtype=float) for tb in synth.halo_orbits()]
    seed = tabs[0][:, 0].copy()
    seed[[1, 3, 5]] = 0.0
    orbit = drivers.halo_orbit(seed, "x0", ctx=ctx)
    g = drivers.stationkeeping_gains(orbit, n_man=N_MAN, ctx=ctx)
    print("orbit 1: P = %.6f TU = %.2f days, lambda_u = %.3f, lambda_s = %.6f; alpha at the burn phases %s"
          % (orbit.period, orbit.period * TU / day, g.lam[0], g.lam[1], np.array2string(g.alpha, precision=3)))
    print("%d runs, %d burns per revolution, injection 1 km / 1 cm/s, execution 1 %% + 0.1 mm/s, lost beyond %.0f km, seed %d"
          % (runs, N_MAN, R_LOST_KM, SEED))
    common = dict(inj_sigma_r_km=1.0, inj_sigma_v_ms=0.01, exe_sigma_frac=0.01, exe_sigma_ms=1e-4, r_lost_km=R_LOST_KM, seed=SEED, MU=MU,
                  gains=g, ctx=ctx)
    laws = [("", g)]
    if law == "target-point":
        gt = drivers.target_point_gains(orbit, n_man=N_MAN, horizons=horizons, q=q, weights=weights, MU=MU, ctx=ctx)
        print("target-point law: horizons %s periods, q %g, weights %s (DU, DU/TU); both laws fly the same draws"
              % (list(horizons), q, "ones" if weights is None else list(weights)))
        laws = [("Floquet       ", g), ("target-point  ", gt)]
    print(("law           " if len(laws) > 1 else "") +
          "  revolutions  navigation error    dv per year, m/s (50 / 95 / 99 %)   lost    largest deviation, km (50 / 99 %)  at the end, km (50 %)"
          "  call ms   uncontrolled: days kept (50 %), lost")
    for n_rev, (nr, nv) in itertools.product(N_REVS, NAV_LEVELS):
        # the uncontrolled runs do not depend on the law: once per row of draws
        free = drivers.stationkeep(orbit, n_rev, runs, nav_sigma_r_km=nr, nav_sigma_v_ms=nv,
                                   **dict(common, gains=g._replace(G=np.zeros_like(g.G)), exe_sigma_frac=None, exe_sigma_ms=None))
        for name, gl in laws:
            out = drivers.stationkeep(orbit, n_rev, runs, nav_sigma_r_km=nr, nav_sigma_v_ms=nv, **dict(common, gains=gl))
            ms = ctx.last_call_ms()
            p = out["percentiles"]
            print(name + "  %3d (%3.0f d)  %5.1f km %5.1f cm/s   %8.3f / %8.3f / %8.3f      %5.1f %%     %9.1f / %9.1f             %9.1f         %7.2f    %6.1f, %.1f %%"
                  % (n_rev, n_rev * orbit.period * TU / day, nr, nv * 100.0, p["dv_per_year_ms"][50], p["dv_per_year_ms"][95],
                     p["dv_per_year_ms"][99], 100.0 * out["lost_share"], p["dev_r_km"][50], p["dev_r_km"][99],
                     float(np.median(out["dev_final_r_km"][out["status"] == 0])), ms, float(np.median(free["t_days"])),
                     100.0 * free["lost_share"]))

    # a family, one orbit per run
    K, R = 8, max(runs // 8, 1)
    values = np.linspace(tabs[0][0, 0], tabs[1][0, 0], K + 1)[1:]
    fam = drivers.halo_family(orbit.state0, values, hold="x0", ctx=ctx)
    members = np.asfortranarray(np.column_stack([orbit.state0, fam.states]))
    periods = np.concatenate([[orbit.period], fam.period])
    tb = lto.halo_table(members, periods, 100, ctx=ctx)
    n = members.shape[1]
    seeds = lto.manifold_seeds(members, periods, tb.M, np.arange(N_MAN) / float(N_MAN), MU=MU, ctx=ctx)
    gains = lto.stationkeep_gains(seeds.V, ctx=ctx)
    assert np.all(seeds.status == 0) and np.all(gains.status == 0)
    own = np.repeat(np.arange(n), R)                                              # the orbit of every run
    X_ref = np.asfortranarray(seeds.X[:, 1][:, :, own])
    dt = np.asfortranarray(np.stack([drivers.stationkeep_spans(seeds.tau, periods[k]) for k in own], axis=1))
    inj, nav, exe = drivers.stationkeep_draws(n * R, N_MAN * N_REV_FAMILY, 1.0, 0.01, 1.0, 0.01, 0.01, 1e-4, SEED, DU, TU)
    r = lto.stationkeep_flight(X_ref, dt, np.asfortranarray(gains.G[..., own]), np.asfortranarray(X_ref[:, 0] + inj), N_REV_FAMILY, nav=nav,
                               exe=exe, r_lost=R_LOST_KM / DU, MU=MU, ctx=ctx, history=False)
    print("family from orbit 1 to orbit 2 in x0, %d members x %d runs x %d revolutions in one call with n_orb = n_batch (%.2f ms), "
          "navigation 1 km / 1 cm/s:" % (n, R, N_REV_FAMILY, ctx.last_call_ms()))
    print("   k        x0          P, days   lambda_u    dv per year, m/s (50 / 95 %)   kept")
    for k in range(n):
        sel = (own == k) & (r.status == 0)
        per_year = r.dv_total[sel] * MS / (N_REV_FAMILY * periods[k] * TU / day / drivers.YEAR_DAYS)
        print("  %2d  %.9f  %8.3f  %9.2f       %8.3f / %8.3f             %5d of %d"
              % (k, members[0, k], periods[k] * TU / day, seeds.lam[0, k], np.percentile(per_year, 50), np.percentile(per_year, 95),
                 int(np.count_nonzero(sel)), R))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("runs", nargs="?", type=int, default=4096)
    ap.add_argument("--law", choices=("floquet", "target-point"), default="floquet")
    ap.add_argument("--horizons", nargs="+", type=float, default=[0.5, 1.0], help="targets, in periods after every burn")
    ap.add_argument("--q", type=float, default=1e-2, help="weight of |dv|^2")
    ap.add_argument("--weights", nargs="+", type=float, default=None, help="weight of the position deviation at each target")
    a = ap.parse_args()
    main(a.runs, a.law, tuple(a.horizons), a.q, None if a.weights is None else tuple(a.weights))
