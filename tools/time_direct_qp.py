#!/usr/bin/env python3
"""Time the direct QP step (lto_direct_qp_step_dev) beside the Jacobian sweep it follows, on device-resident operands.

usage: python tools/time_direct_qp.py [--free] [segments ...]   (default 30 4096 16384; nstate 6, nsteps 10, one trajectory)
Prints one line per size: mean wall time of the Jacobian sweep and of the QP step over 20 repetitions (HIP events).  For
per-kernel times run it under `rocprofv3 --kernel-trace --stats -- python tools/time_direct_qp.py` (a run of its own).
--free: the free-end step (flagEnd = true, lto_direct_qp_step_free) beside the frozen-end step, both through the host-pointer
entries with the library's kernel timing (HIP events around the QP launches only): median over the repetitions.
--free-tf: the same, with the free-end, free-tf step (lto_direct_qp_step_free_tf, 1-day step) timed beside the two.
"""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import synth  # noqa: E402


def run(S, reps=20, ns=6, nsteps=10):
    n = S + 1
    dev = torch.device("cuda", 0)
    X, U, T = synth.direct_problem(n, nstate=ns)
    Xd = torch.tensor(np.ascontiguousarray(X[:, :, 0]), device=dev)
    Ud = torch.tensor(np.ascontiguousarray(U[:, :, 0]), device=dev)
    td = torch.tensor(T[:, 0], device=dev)
    nj = ns * 2 * (ns + 3)
    Jac = torch.empty((nj, S), dtype=torch.float64, device=dev)
    defect = torch.empty((ns, S), dtype=torch.float64, device=dev)
    tg = lto.direct_targets(X[:6, 0, 0], X[:6, -1, 0], 1000.0, np.zeros(3), np.zeros(3))
    tgd = torch.tensor(np.frombuffer(bytes(tg), dtype=np.float64).copy(), device=dev)
    dX, dU = torch.empty_like(Xd), torch.empty_like(Ud)
    dV, cost = torch.empty(6, dtype=torch.float64, device=dev), torch.empty(1, dtype=torch.float64, device=dev)
    ctx = lto.default_context(0)
    plan = lto.DirectPlan(ctx, ns, n, 1, nsteps, lto.MU, lto.DU, lto.TU, 2000.0)
    st = lto.current_stream_ptr()

    def jac():
        plan.jacobian(Xd, n, Ud, n, td, 1, Jac, S, None, defect, S, None, stream=st)

    def qp():
        plan.qp_step(Jac, S, defect, S, Xd, n, Ud, n, td, 1, tgd, dX, dU, dV, cost, stream=st)

    out = {"segments": S}
    for name, f in (("jacobian_ms", jac), ("qp_step_ms", qp)):
        for _ in range(3):
            f()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            f()
        e1.record()
        torch.cuda.synchronize()
        out[name] = e0.elapsed_time(e1) / reps
    out["cost_finite"] = bool(torch.isfinite(cost).all())
    plan.close()
    return out


def run_free(S, reps=20, ns=6, nsteps=10, free_tf=False):
    n = S + 1
    X, U, T = synth.direct_problem(n, nstate=ns)
    X, U, t = X[:, :, 0], U[:, :, 0], T[:, 0]
    tg = lto.direct_targets(X[:6, 0], X[:6, -1], 1000.0, np.zeros(3), np.zeros(3))
    em = lto.direct_end_model(np.full(6, 0.1), np.full(6, -0.1), 1.0, 1.0)
    ctx = lto.default_context(0)
    ctx.set_timing(True)
    out = {"segments": S}
    steps = (("frozen_qp_ms", lambda: lto.direct_qp_step(X, U, t, nsteps, lto.MU, lto.DU, lto.TU, 2000.0, tg, ctx=ctx)),
             ("free_qp_ms", lambda: lto.direct_qp_step_free(X, U, t, nsteps, lto.MU, lto.DU, lto.TU, 2000.0, tg, em, 1.0, ctx=ctx)))
    if free_tf:
        day = lto.day / lto.TU
        tb = lto.direct_tf_bounds(day, t[0] + day, t[-1] + 10 * day)       # the synthetic grids run past 40 days
        steps += (("free_tf_qp_ms", lambda: lto.direct_qp_step_free_tf(X, U, t, nsteps, lto.MU, lto.DU, lto.TU, 2000.0, tg, em, 1.0, tb,
                                                                       ctx=ctx)),)
    for name, f in steps:
        ms = []
        for k in range(reps + 3):
            f()
            if k >= 3:
                ms.append(ctx.last_kernel_ms())
        out[name] = float(np.median(ms))
    ctx.set_timing(False)
    return out


if __name__ == "__main__":
    free_tf = "--free-tf" in sys.argv
    free = "--free" in sys.argv or free_tf
    sizes = [int(a) for a in sys.argv[1:] if not a.startswith("--")] or [30, 4096, 16384]
    for S in sizes:
        print(json.dumps(run_free(S, free_tf=free_tf) if free else run(S)), flush=True)
