#!/usr/bin/env python3
"""Time one device Newton iteration of the indirect method on device-resident operands: the STM sweep, the Newton solve
(structured cyclic reduction, lto_indirect_newton_solve_dev) and the second-order-correction re-solve through the stored
factorisation (Phi = NULL).

usage: python tools/time_indirect_newton.py [--ndim 12|14] [segments ...]   (default 12-dim; 30 4096 16384 segments, one trajectory,
       the reference's adaptive order-8 integrator)
Prints one JSON line per size: the median over 20 repetitions of each step (torch events around each launch sequence) and of
their sum.  14-dim plans carry Isp = 2000 s in the parameter tuple's mass slot and m0 = 1000 kg.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402


def run(S, ndim=12, reps=20):
    n = S + 1
    dev = torch.device("cuda", 0)
    XC, T = synth.indirect_problem(n, lam_sigma=0.1)
    X = XC if ndim == 12 else drivers.lift_to_mass(XC, 1000.0)
    prm = lto.make_params(lto.MU, lto.DU, lto.TU, 0.05, 1000.0 if ndim == 12 else 2000.0, 1.0, 1.0, 1.0)
    ctx = lto.default_context(0)
    plan = lto.IndirectPlan(ctx, n, 1, prm, lto.integrator(), ndim=ndim)
    Xd = torch.from_numpy(synth.to_soa_nodes(X)).to(dev)
    td = torch.from_numpy(np.ascontiguousarray(T[:, 0])).to(dev)
    Phi = torch.empty((ndim * ndim, S), dtype=torch.float64, device=dev)
    d = torch.empty((ndim, S), dtype=torch.float64, device=dev)
    d2 = torch.empty_like(d)
    delta = torch.empty((ndim, n), dtype=torch.float64, device=dev)
    delta2 = torch.empty_like(delta)
    st = lto.current_stream_ptr()
    steps = (("stm_ms", lambda: plan.jacobian(Xd, n, td, 1, Phi, S, d, S, stream=st)),
             ("solve_ms", lambda: plan.newton_solve(Phi, S, d, S, delta, n, stream=st)),
             ("resolve_ms", lambda: plan.newton_solve(None, 0, d2, S, delta2, n, stream=st)))
    steps[0][1]()
    d2.copy_(d * 0.5)
    out = {"ndim": ndim, "segments": S}
    for name, f in steps:
        ms = []
        for k in range(reps + 3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            if k >= 3:
                ms.append(e0.elapsed_time(e1))
        out[name] = float(np.median(ms))
    out["iteration_ms"] = out["stm_ms"] + out["solve_ms"] + out["resolve_ms"]
    out["finite"] = bool(torch.isfinite(delta).all() and torch.isfinite(delta2).all())
    plan.close()
    return out


if __name__ == "__main__":
    argv = sys.argv[1:]
    ndim = 12
    if "--ndim" in argv:
        i = argv.index("--ndim")
        ndim = int(argv[i + 1])
        del argv[i:i + 2]
    if ndim not in (12, 14):
        raise SystemExit("--ndim takes 12 or 14")
    for S in [int(a) for a in argv] or [30, 4096, 16384]:
        print(json.dumps(run(S, ndim)), flush=True)
