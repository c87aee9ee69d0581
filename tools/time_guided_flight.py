#!/usr/bin/env python3
"""Times of the neighbouring-extremal guidance on one GPU: the demo's p = 2 solution on its own 30 nodes, DOP853 at
1e-13.  The gains call (STM sweep + backward sweep, and the sweep of lto_indirect_jacobian alone beside it) for one trajectory and for
4 096 copies of it; the guided flight with an update
at every node and open loop (update_every = 0), one nominal for all starts, B = 4 096 and B = 65 536 dispersed starts (1 km,
1 cm/s).  Kernel time by lto_set_timing, the median of five calls after three warm-ups; the call's wall time beside it.  4 096
lanes are 64 wavefronts: they cannot fill the chip's 1 024 SIMDs, and that figure is the latency of one lane, not throughput.

  python tools/time_guided_flight.py [--mass]

--mass: the same for the 14-row variable-mass system: the p = 2 solution lifted and re-solved with the free final
mass at Isp = 2000 s, lto_guidance_gains_mass_batch and lto_guided_flight_mass_batch.
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
    gains, flight, ns = lto.guidance_gains, lto.guided_flight, 6
    if mass:
        XC, _, flag = drivers.multiShoot_CRTBP_indirect_mass(drivers.lift_to_mass(XC, 1e3), t, MU, DU, TU, XC.shape[1], Isp, 10.0, False,
                                                             False, 50, 2.0, 1.0, verbose=False)
        assert flag == 0
        prm = lto.make_params(MU, DU, TU, 10.0, Isp, 1.0, 2.0, 1.0)
        gains, flight, ns = lto.guidance_gains_mass, lto.guided_flight_mass, 7
    ctx.set_timing(True)
    for B in (1, 4096):
        X = np.asfortranarray(np.repeat(XC[:, :, None], B, axis=2))
        g, ker, wall = timed(ctx, lambda: gains(X, t, prm, ctx=ctx))
        _, stm, _ = timed(ctx, lambda: lto.indirect_stm(X, t, prm, ctx=ctx))
        print("gains%s, B = %5d x %d nodes: STM sweep + backward sweep %.3f ms (median of 5 after 3 warm-ups; lto_indirect_jacobian's "
              "sweep alone %.3f ms), call %.3f ms; status 0: %d" % (" (14 rows)" if mass else "", B, XC.shape[1], ker, stm, wall, int((np.asarray(g.status) == 0).sum())))
    K = g.K[:, :, :, 0]
    for B in (4096, 65536):
        x0 = drivers.dispersion_starts(XC[:ns, 0], B, 1.0, 0.01, 0, DU, TU)
        for every in (1, 0):
            r, ker, wall = timed(ctx, lambda: flight(XC, t, K, x0, prm, every, ctx=ctx))
            steps = r.accepted + r.rejected
            print("flight%s, B = %6d, update_every = %d: kernel %.3f ms (median of 5 after 3 warm-ups), call %.3f ms; %.3f us per "
                  "trajectory; status 0: %d; trial steps per trajectory %d .. %d" % (
                      " (14 rows)" if mass else "", B, every, ker, wall, ker * 1e3 / B, int((r.status == 0).sum()), steps.min(), steps.max()))
    ctx.set_timing(False)


if __name__ == "__main__":
    main(mass="--mass" in sys.argv[1:])
