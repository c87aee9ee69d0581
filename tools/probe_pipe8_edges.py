#!/usr/bin/env python3
"""Development aid: where a wavefront of the eight-wave contract sweep spends its ticks (probe build, LTO_HIP_LIB=build/liblto_probe.so).
Per wave of the workgroup, medians over the workgroups: the fill (first hook to leaving the first phase barrier), the ticks waited at
the phase barriers, the drain (leaving the second-to-last barrier to arriving at the last), the epilogue (leaving the last barrier to
the end of the role, Phi / defect stores issued) and the number of barriers; the base wave's whole loop in ticks and microseconds.
The column waves' epilogue is split by three stamps, in ticks since the last barrier: `first` = before the first Phi store, `issued` =
after the last one is issued, `drained` = after s_waitcnt vmcnt(0) (the probe build waits there; the product does not)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import lowthrustopt_amd as lto
from lowthrustopt_amd import synth
from probe_kernels import timeit

# role of wave 0..7 per dimension: the placement table of kernels_indirect_pipe8.hip (P8Map<ND>::map), kept in step by hand
COL0, COL1, COL2, BASE, COEF, EVEN, ODD, EXIT = "cols 0-3", "cols 4-7", "cols 8-11", "base", "coef", "cols 12-15 even", "cols 12-15 odd", "(exits)"
PLACEMENT = {14: [COEF, COL1, BASE, ODD, COL0, EVEN, EXIT, COL2],
             12: [ODD, COL1, BASE, COEF, COL0, EVEN, EXIT, COL2]}


def main():
    ctx = lto.Context(0)
    st = lto.current_stream_ptr()
    S = 4096
    n = S + 1
    for ndim in (14, 12):
        XC, T = synth.indirect_problem(n)
        if ndim == 14:
            Xh = np.zeros((14, n, 1), order="F")
            Xh[:6] = XC[:6]; Xh[6] = 1000.0; Xh[7:13] = XC[6:]; Xh[13] = 0.2
            slot = 2000.0
        else:
            Xh, slot = XC, 1000.0
        prm = lto.make_params(lto.MU, lto.DU, lto.TU, 0.05, slot, 1.0, 1.0, 1.0)
        X = torch.from_numpy(synth.to_soa_nodes(Xh)).cuda()
        t = torch.from_numpy(np.ascontiguousarray(T[:, 0])).cuda()
        d = torch.zeros(32, S, dtype=torch.float64, device="cuda")   # rows 16..23: probe build diagnostics
        Phi = torch.zeros(ndim * ndim, S, dtype=torch.float64, device="cuda")
        plan = lto.IndirectPlan(ctx, n, 1, prm, lto.integrator(lto.RK4, steps=64, max_steps=1 << 20), ndim=ndim)
        plan.set_kernel(5)
        ms = timeit(lambda: plan.jacobian(X, n, t, 1, Phi, S, d, S, stream=st), iters=30, warm=5)
        dh = d.cpu().numpy()
        cyc, wall = dh[17, ::16], dh[18, ::16]
        ghz = np.median(cyc / wall) * 0.1
        print("ndim=%d  pipe8 %.1f us; base loop %.0f kticks = %.1f us at %.3f GHz" % (ndim, ms * 1e3, np.median(cyc) / 1e3, np.median(wall) / 100.0, ghz))
        print("  %-2s %-16s %8s %8s %8s %8s %6s %8s %8s %8s" % ("w", "role", "fill", "waited", "drain", "epilog", "syncs", "first", "issued", "drained"))
        for w in range(8):
            col = lambda r: np.median(dh[r].reshape(-1, 16)[:, w])
            print("  w%d %-16s %8.0f %8.0f %8.0f %8.0f %6.0f %8.0f %8.0f %8.0f" % (w, PLACEMENT[ndim][w], col(20), col(16), col(21), col(22), col(23), col(24), col(25), col(26)))
        plan.close()


if __name__ == "__main__":
    main()
