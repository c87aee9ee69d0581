#!/usr/bin/env python3
"""Times of the control replay on one GPU: the demo's p = 2 solution, 257 knots, DOP853 at 1e-13, one history for
all starts, B = 4 096 and B = 65 536 dispersed starts (1 km, 1 cm/s).  Kernel time by lto_set_timing (the moment kernel and the
replay kernels of one call), the median of five calls after three warm-ups; the call's wall time beside it.  With --cpu also the
seconds per trajectory of the CPU reference of the tests (tests/replay_reference.py: scipy DOP853 at 1e-13, interval by interval).
4 096 lanes are 64 wavefronts: they cannot fill the chip's 1 024 SIMDs, and that figure is the latency of one lane, not throughput.

  python tools/time_control_replay.py [--cpu]
"""
import importlib.util
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402


def main(cpu=False):
    spec = importlib.util.spec_from_file_location("halo_demo", os.path.join(ROOT, "examples", "halo_transfer_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    XC, t, _, flag = demo.solve_p2(verbose=False)
    assert flag == 0
    ctx = lto.default_context(0)
    prm = (MU, DU, TU, 10.0, 1e3, 1.0, 2.0, 1.0)
    lamv = drivers.fly_control(ctx, XC, t, prm, n_knots=257)["lamv"]
    ctx.set_timing(True)
    for B in (4096, 65536):
        x0 = drivers.dispersion_starts(XC[:6, 0], B, 1.0, 0.01, 0, DU, TU)
        ker, wall = [], []
        for k in range(8):
            t0 = time.perf_counter()
            r = lto.control_replay(x0, lamv, t[0], t[-1], prm, ctx=ctx)
            wall.append((time.perf_counter() - t0) * 1e3)
            ker.append(ctx.last_kernel_ms())
        steps = r.accepted + r.rejected
        print("B = %6d: kernels %.3f ms (median of 5 after 3 warm-ups), call %.3f ms; %.3f us per trajectory; status 0: %d; trial steps "
              "per trajectory %d .. %d" % (B, statistics.median(ker[3:]), statistics.median(wall[3:]),
                                           statistics.median(ker[3:]) * 1e3 / B, int((r.status == 0).sum()), steps.min(), steps.max()))
    ctx.set_timing(False)
    if cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import replay_reference as R
        t0 = time.perf_counter()
        fl = R.fly(XC[:6, 0], lamv, t[0], t[-1], prm)
        print("CPU reference (scipy DOP853 at 1e-13, 256 intervals): %.2f s per trajectory, ok %s" % (time.perf_counter() - t0, fl.ok))


if __name__ == "__main__":
    main("--cpu" in sys.argv[1:])
