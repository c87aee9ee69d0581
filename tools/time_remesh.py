#!/usr/bin/env python3
"""Times of the indirect mesh re-distribution on the demo transfer at rho = 1/32: defect- and STM-sweep kernel times
(lto_set_timing) on the old and the new grid, alternating, at 30 nodes and at 4 097 nodes (the fixture put on a uniform 4 097-node
grid, then re-meshed by counts), and the wall time of the re-mesh call itself with and without its re-solve.  Run it under
`rocprofv3 --kernel-trace --stats -- python tools/time_remesh.py` for the split into k_remesh_grid / k_remesh_nodes / the loop."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402


def main(reps=7):
    spec = importlib.util.spec_from_file_location("halo_remesh_demo_time", os.path.join(ROOT, "examples", "halo_remesh_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    ctx = lto.default_context(0)
    t, levels = demo.rho_ladder()
    rho, XC = levels[-1]
    prm = demo.params(rho)
    n = t.size
    uni = lto.indirect_remesh(XC, t, prm, n_new=4097, weights=np.ones(n - 1), passes=1, ctx=ctx)
    assert uni.status == 0
    for name, X0, t0 in (("30 nodes", XC, t), ("4097 nodes", uni.XC_out, uni.t_out)):
        r = lto.indirect_remesh(X0, t0, prm, passes=2, ctx=ctx)
        call = []
        for solve in (False, True):
            best = np.inf
            for _ in range(3):
                lto.indirect_remesh(X0, t0, prm, passes=2, ctx=ctx, solve=solve)
                best = min(best, ctx.last_call_ms())
            call.append(best)
        print("%s: status %d, %d iterations, max |defect| %.2e" % (name, r.status, r.iterations, np.abs(r.defect).max()))
        print("  trial steps  old grid: %s" % demo.stats(r.steps_before))
        print("  trial steps  new grid: %s" % demo.stats(r.steps_after))
        ctx.set_timing(True)
        rows = []
        for _ in range(reps):                     # old and new grid alternate inside one process
            row = []
            for X, tt in ((X0, t0), (r.XC_out, r.t_out)):
                lto.indirect_defectCalc(X, tt, prm, ctx=ctx)
                row.append(1e3 * ctx.last_kernel_ms())
                lto.indirect_stm(X, tt, prm, ctx=ctx)
                row.append(1e3 * ctx.last_kernel_ms())
            rows.append(row)
        ctx.set_timing(False)
        rows = np.array(rows[1:])                 # the first round warms up
        med, lo, hi = np.median(rows, axis=0), rows.min(axis=0), rows.max(axis=0)
        for j, what in enumerate(("defect sweep, old grid", "STM sweep,    old grid", "defect sweep, new grid", "STM sweep,    new grid")):
            print("  %s: median %7.1f us  (min %7.1f, max %7.1f, %d runs)" % (what, med[j], lo[j], hi[j], rows.shape[0]))
        print("  re-mesh call (2 passes), wall: grid + nodes + counts %.2f ms; with the re-solve %.2f ms" % (call[0], call[1]))


if __name__ == "__main__":
    main()
