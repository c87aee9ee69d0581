#!/usr/bin/env python3
"""Wall time of addTimeFinal on the device for the 14-row variable-mass system (lto_indirect_add_time_mass_batch) beside the 12-row
call (lto_indirect_add_time_batch), both in one process: the library's own call timer (lto_set_timing / lto_last_call_ms), median
of five calls after two warm-ups.

usage: python tools/time_add_time_mass.py [K ...]   (default 256; the demo's 30 nodes, n_desired = 200, DOP853 at 1e-13, dt from 0.25
to 8 days, maxIter = 10)
The 12-row call runs the demo's p = 2 transfer at a frozen 1000 kg, the 14-row call the same transfer solved at Isp = 2000 s.  The
guesses alone (XC_out = NULL) are timed too: what is left is the Newton loop and the cost.  Prints one JSON line per K."""
import importlib.util
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU, day  # noqa: E402


def median_ms(ctx, fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        fn()
        ts.append(ctx.last_call_ms())
    return statistics.median(ts)


def main(Ks):
    spec = importlib.util.spec_from_file_location("halo_demo", os.path.join(ROOT, "examples", "halo_transfer_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    XC, t, _, flag = mod.solve_p2(seed=0, verbose=False)
    assert flag == 0
    n = XC.shape[1]
    X14, _, flag = drivers.multiShoot_CRTBP_indirect_mass(drivers.lift_to_mass(XC, 1e3), t, MU, DU, TU, n, 2000.0, 10.0, False, False, 50,
                                                          2.0, 1.0, verbose=False)
    assert flag == 0
    tab = synth.halo_orbits()[1][:6]
    times = np.linspace(0.0, 1.0, tab.shape[1])
    prm12 = lto.make_params(MU, DU, TU, 10.0, 1e3, 1.0, 2.0, 1.0)
    prm14 = lto.make_params(MU, DU, TU, 10.0, 2000.0, 1.0, 2.0, 1.0)
    ctx = lto.Context(0)
    ctx.set_timing(True)
    for K in Ks:
        dts = np.linspace(0.25, 8.0, K) * day / TU
        res = {}

        def run(key, fn, X, prm, solve):
            def call():
                res[key] = fn(X, t, prm, times, tab, dts, maxIter=10, solve=solve, ctx=ctx)
            return median_ms(ctx, call)
        g12 = run("g12", lto.indirect_add_time, XC, prm12, False)
        g14 = run("g14", lto.indirect_add_time_mass, X14, prm14, False)
        f12 = run("f12", lto.indirect_add_time, XC, prm12, True)
        f14 = run("f14", lto.indirect_add_time_mass, X14, prm14, True)
        r12, r14 = res["f12"], res["f14"]
        print(json.dumps({"K": K, "n_nodes": int(n), "n_desired": 200,
                          "rows12": {"guess_ms": round(g12, 3), "full_ms": round(f12, 3), "iters_max": int(r12.iterations.max()),
                                     "iters_sum": int(r12.iterations.sum()), "converged": int((r12.status == 0).sum())},
                          "rows14": {"guess_ms": round(g14, 3), "full_ms": round(f14, 3), "iters_max": int(r14.iterations.max()),
                                     "iters_sum": int(r14.iterations.sum()), "converged": int((r14.status == 0).sum())},
                          "ratio_full": round(f14 / f12, 3), "ratio_guess": round(g14 / g12, 3)}), flush=True)
    ctx.set_timing(False)
    ctx.close()


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [256])
