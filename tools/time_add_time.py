#!/usr/bin/env python3
"""Time addTimeFinal on the device (lto_indirect_add_time_batch) for K time-of-flight changes of the demo's p = 2 transfer.

usage: python tools/time_add_time.py [K ...]   (default 256; the demo's 30 nodes, n_desired = 200, DOP853 at 1e-13)
Every library call here ends synchronised, so each phase is the wall time of calls that contain only it, median of 5:
  guess_ms   the guesses alone (XC_out = NULL): the extended trajectories' dense sweep, re-mesh, snap and copies
  solve_ms / iters / iter_ms  lto_indirect_solve_batch on the K guesses: the whole loop, its iteration count, their ratio
  full_ms    the whole call, solve and cost included
Run it under `rocprofv3 --kernel-trace --stats --output-format csv` for the per-kernel split (k_indirect_dense, k_remesh_spline,
k_find_tau, k_dense_cost and the Newton loop's kernels).
Prints one JSON line per K."""
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU, day  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def median_ms(fn, reps=5):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main(Ks):
    import importlib.util
    spec = importlib.util.spec_from_file_location("halo_demo", os.path.join(ROOT, "examples", "halo_transfer_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    XC, t, _, flag = mod.solve_p2(seed=0, verbose=False)
    assert flag == 0
    tab = synth.halo_orbits()[1][:6]
    times = np.linspace(0.0, 1.0, tab.shape[1])
    prm = lto.make_params(MU, DU, TU, 10.0, 1e3, 1.0, 2.0, 1.0)
    for K in Ks:
        dts = np.linspace(0.25, 8.0, K) * day / TU
        g = lto.indirect_add_time(XC, t, prm, times, tab, dts, solve=False)
        guess_ms = median_ms(lambda: lto.indirect_add_time(XC, t, prm, times, tab, dts, solve=False))
        res = {}

        def solve():
            res["r"] = lto.indirect_solve_batch(g.XC_guess, g.t_out, prm, maxIter=10)
        solve_ms = median_ms(solve)
        iters = int(res["r"][3].max())
        full_ms = median_ms(lambda: lto.indirect_add_time(XC, t, prm, times, tab, dts, maxIter=10))
        print(json.dumps({"K": K, "n_nodes": int(t.size), "n_desired": 200, "guess_ms": round(guess_ms, 3),
                          "solve_ms": round(solve_ms, 3), "iters": iters, "iter_ms": round(solve_ms / max(iters, 1), 3),
                          "full_ms": round(full_ms, 3), "converged": int((res["r"][2] == 0).sum())}), flush=True)


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [256])
