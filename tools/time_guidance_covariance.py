#!/usr/bin/env python3
"""Times of the linear covariance of guided flights on one GPU: the demo's p = 2 solution on its own 30 nodes, DOP853
at 1e-13.  lto_guidance_covariance_batch for one trajectory x 1 case, one trajectory x 9 cases (three navigation sigmas x three
update cadences) and 4 096 copies of the trajectory x 9 cases, with the gains call alone beside each -- the difference is the
forward pass k_guidance_covariance -- and the Monte Carlo that gives the same nine-entry table for one trajectory: nine guided
flights of 4 096 draws each (lto_guided_flight_batch, gains in hand).  Kernel time by lto_set_timing, the median of five calls
after three warm-ups; the call's wall time beside it.

  python tools/time_guidance_covariance.py [--mass]

--mass: the same for the 14-row variable-mass system (the solution lifted and re-solved with the free final mass at Isp = 2000 s).
"""
import importlib.util
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402

NAV = ((0.03, 3e-4), (0.1, 1e-3), (0.3, 3e-3))       # km, m/s
EVERY = (1, 3, 10)


def timed(ctx, call):
    ker, wall = [], []
    for _ in range(8):
        t0 = time.perf_counter()
        r = call()
        wall.append((time.perf_counter() - t0) * 1e3)
        ker.append(ctx.last_kernel_ms())
    return r, statistics.median(ker[3:]), statistics.median(wall[3:])


def main(mass=False, Isp=2000.0):
    spec = importlib.util.spec_from_file_location("halo_demo", os.path.join(ROOT, "examples", "halo_transfer_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    XC, t, _, flag = demo.solve_p2(verbose=False)
    assert flag == 0
    ctx = lto.default_context(0)
    prm = lto.make_params(MU, DU, TU, 10.0, 1e3, 1.0, 2.0, 1.0)
    gains, flight, nx = lto.guidance_gains, lto.guided_flight, 6
    if mass:
        XC, _, flag = drivers.multiShoot_CRTBP_indirect_mass(drivers.lift_to_mass(XC, 1e3), t, MU, DU, TU, XC.shape[1], Isp, 10.0, False,
                                                             False, 50, 2.0, 1.0, verbose=False)
        assert flag == 0
        prm = lto.make_params(MU, DU, TU, 10.0, Isp, 1.0, 2.0, 1.0)
        gains, flight, nx = lto.guidance_gains_mass, lto.guided_flight_mass, 7
    tag = " (14 rows)" if mass else ""
    P0 = drivers.covariance_diag(nx, 1.0, 0.01, 1.0, DU, TU)
    cases = [(nav, ev) for nav in NAV for ev in EVERY]
    P9 = np.asfortranarray(np.repeat(P0[:, :, None], 9, axis=2))
    R9 = np.asfortranarray(np.stack([drivers.covariance_diag(nx, nav[0], nav[1], 0.1, DU, TU) for nav, _ in cases], axis=2))
    E9 = np.array([ev for _, ev in cases], dtype=np.int32)
    ctx.set_timing(True)
    for B, nc in ((1, 1), (1, 9), (4096, 9)):
        X = np.asfortranarray(np.repeat(XC[:, :, None], B, axis=2))
        c, ker, wall = timed(ctx, lambda: lto.guidance_covariance(X, t, prm, P9[:, :, :nc], R9[:, :, :nc], E9[:nc], ctx=ctx))
        g, gker, gwall = timed(ctx, lambda: gains(X, t, prm, ctx=ctx))
        print("covariance%s, B = %4d x %d cases x %d nodes: sweep + gains + forward pass %.3f ms (median of 5 after 3 warm-ups; the gains "
              "call alone %.3f ms, the forward pass by difference %.3f ms), call %.3f ms (gains call %.3f ms); status 0: %d of %d" % (
                  tag, B, nc, XC.shape[1], ker, gker, ker - gker, wall, gwall, int((np.asarray(c.cov_status) == 0).sum()), B * nc))
    # the Monte Carlo of the same nine-entry table for one trajectory
    K = g.K[:, :, :, 0]
    N = 4096
    x0 = drivers.dispersion_starts(XC[:nx, 0], N, 1.0, 0.01, 0, DU, TU)
    ker_sum = wall_sum = 0.0
    for (nav, ev) in cases:
        n_upd = lto.guided_updates(XC.shape[1], ev)
        e = np.zeros((nx, n_upd, N), order="F")
        e[0:6] = drivers.guided_nav(n_upd, N, nav[0], nav[1], 1, DU, TU)
        _, ker, wall = timed(ctx, lambda: flight(XC, t, K, x0, prm, ev, e, ctx=ctx))
        ker_sum += ker
        wall_sum += wall
    print("Monte Carlo of the same table%s, one trajectory: 9 guided flights of %d draws, gains in hand: kernels %.3f ms, calls %.3f ms "
          "in all; each entry then carries 1 / sqrt(2 N) = %.1f %% of sampling noise in its sigma" % (
              tag, N, ker_sum, wall_sum, 100.0 / np.sqrt(2.0 * N)))
    ctx.set_timing(False)


if __name__ == "__main__":
    main(mass="--mass" in sys.argv[1:])
