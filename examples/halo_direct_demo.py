#!/usr/bin/env python3
"""Earth-Moon L2 halo -> halo transfer by DIRECT multiple shooting, on the GPU.

Follows the direct demo of the reference (CRTBP_Multishoot_direct_demo.jl:183-196): the stacked halo guess (the stacking of
halo_transfer_demo.py: tau1 = 0.75, 30 nodes over 20 days), zero thrust, nsteps = 10, Isp = 2000 s, mass = 1000 kg,
flagEnd = false, beta = 0, no impulses, at most 100 iterations.  The whole loop -- Jacobian sweep, the minimum-energy QP step
solved exactly on the device, the batched line search -- is one lto_direct_solve call.  With --then-indirect the smoothed
states are handed to the indirect method (p = 2, adjoints only first), the reference's sequence.

With --costate-guess the indirect method starts from the costates the direct solve already holds -- the multipliers of its QP
step (drivers.direct_to_indirect, one device call for the seed) -- with full Newton from the first iteration; given
with --then-indirect too, the iteration counts of both routes are printed side by side.

--free-ends [beta] runs the reference's other mode, flagEnd = true (default beta = 0): odd iterations also move the departure and
arrival phases tau1, tau2 (by at most 0.1 per step), so the transfer finds where on the two orbits it starts and ends.  The run
starts from tau2 offset by --tau2-offset (default 0.02) from the stacked value and prints the final phases.
--free-tf [days] also makes the time of flight a variable of the free iterations, at most `days` per step (default 1, the
reference's bound; implies --free-ends 0 unless given): tf in [1 day, 40 days].
--refine [tol_max] instead solves, refines the mesh on the device (lto_direct_refine, DESIGN 4.14: nodes removed while a segment's
RKF7(8) estimate is below tol_max / 1000, segments bisected while one is above tol_max, default 1e-16) and solves again on the
refined mesh; prints node counts and the largest estimate before and after, and the re-solve's status and iterations.
--equidistribute N solves, refines as --refine does, moves the refined mesh onto N nodes whose estimates are equidistributed
(drivers.meshEquidistribute_direct, lto_direct_resample, DESIGN 4.17: two passes) and solves again on them; prints node counts,
the largest and smallest estimate before and after, and the re-solve's status.
--ballistic-guess takes the guess from drivers.stacked_guess instead: the reference's own construction (demo :116-157), 10 days
ballistically on each orbit, made in one device call (lto_stack_guess_batch).
--multi-start N runs N departure phases tau1 evenly spread over [0, 1) side by side (drivers.multiStart_direct: the guesses, the
end targets and the solves are one device call each) and prints the ranking of the converged starts by cost.
"""
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402


def _stacking():
    spec = importlib.util.spec_from_file_location("halo_transfer_demo", os.path.join(ROOT, "examples", "halo_transfer_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def demo_problem(n_nodes=30, tof_days=20.0, tau1=0.75, ballistic=False):
    """(X_all [6 x n], u_all [3 x n], t_TU, tau1, tau2, X0_times, X0_states, Xf_times, Xf_states): the stacked guess and the two
    orbit tables on normalised times LinRange(0, 1, 100) (demo :68-71).  tau2 = the phase of orbit 2 the stacking joins.
    ballistic: the guess and tau2 of drivers.stacked_guess (half of tof_days on each orbit) instead of the table interpolation."""
    tabs = synth.halo_orbits()
    times = [np.linspace(0.0, 1.0, tb.shape[1]) for tb in tabs]
    if ballistic:
        tof = 0.5 * tof_days * lto.day / TU
        X, t, tau1, tau2 = drivers.stacked_guess(n_nodes, tof, tof, tau1, times[0], tabs[0], times[1], tabs[1], MU)
        return X, np.zeros((3, n_nodes)), t, tau1, tau2, times[0], tabs[0], times[1], tabs[1]
    X, t = _stacking().stacked_guess(n_nodes, tof_days, tau1)
    # phase of the guess's last node on orbit 2 (find_tau, demo :151): nearest table sample, refined on a fine grid
    taus = np.linspace(0.0, 1.0, 20001)
    d = np.linalg.norm(synth.halo_state(1, taus * 99 * synth.HALO_DT[1]) - X[:, -1:], axis=0)
    tau2 = float(taus[np.argmin(d)])
    U = np.zeros((3, n_nodes))
    return X, U, t, tau1, tau2, times[0], tabs[0], times[1], tabs[1]


def main(verbose=True, then_indirect=False, python_loop=False, maxIter=100, free_ends=None, tau2_offset=0.0, free_tf=None,
         ballistic=False, costate_guess=False):
    ctx = lto.default_context(0)
    X, U, t, tau1, tau2, t0s, X0s, tfs, Xfs = demo_problem(ballistic=ballistic)
    tau2 += tau2_offset
    n, nsteps, Isp, mass = X.shape[1], 10, 2000.0, 1000.0
    ops = drivers.HipDirectOps(MU, DU, TU, Isp, ctx) if python_loop else None
    t0 = time.perf_counter()
    flag_end = free_ends is not None
    X, U, tau1, tau2, t, dV1, dV2, defect = drivers.multiShoot_CRTBP_direct(
        X, U, tau1, tau2, t, np.zeros(3), np.zeros(3), MU, DU, TU, n, nsteps, mass, Isp, t0s, X0s, tfs, Xfs, False, flag_end,
        float(free_ends or 0.0), False, maxIter, ops=None if flag_end else ops, verbose=verbose,
        tf_step=float(free_tf or 0.0) * lto.day / TU if flag_end else 0.0)
    last = drivers.multiShoot_CRTBP_direct.last
    res = {"direct": (last["status"], last["iterations"], float(np.abs(defect).max())), "X": X, "U": U, "tau": (tau1, tau2),
           "tf_days": float(t[-1] * TU / lto.day)}
    print("direct%s: status %d after %d iterations, max defect %.2e, cost %.6f, tau = (%.9f, %.9f), max thrust %.3f N (%.2f s)" % (
        " (free ends, beta = %g)" % free_ends if flag_end else "", last["status"], last["iterations"], np.abs(defect).max(),
        last["history"][1, last["iterations"] - 1], tau1, tau2, np.linalg.norm(U, axis=0).max(), time.perf_counter() - t0))
    if free_tf and flag_end:
        print("free tf (step %g days): tf = %.6f days" % (free_tf, res["tf_days"]))
    if then_indirect and last["status"] == 0:
        rng = np.random.default_rng(0)
        XC = np.vstack([X, 0.1 * rng.standard_normal((6, n))])
        prm = lto.make_params(MU, DU, TU, 10.0, mass, 1.0, 2.0, 1.0)
        XC, d, flag, it1, h1 = lto.indirect_solve(XC, t, prm, None, True, 10, ctx=ctx)
        XC, d, flag, it2, h2 = lto.indirect_solve(XC, t, prm, None, False, 50, ctx=ctx)
        for k, (er, alpha) in enumerate(list(h1) + list(h2) if verbose else []):
            print("Iter %d. Max defect = %.2e. alpha = %.3f." % (k + 1 if k < len(h1) else k + 1 - len(h1), er, alpha))
        print("indirect p = 2 from the direct solution, random costates: status %d, max defect %.2e, %d adjoints-only + %d full "
              "iterations" % (flag, np.abs(d).max(), min(it1, 10), it2))
        res["indirect"] = (flag, float(np.abs(d).max()))
        res["indirect_iterations"] = (min(it1, 10), it2)
    if costate_guess and last["status"] == 0:
        s0, sf = drivers.interpEndStates(tau1, tau2, t0s, X0s, tfs, Xfs)
        r = drivers.direct_to_indirect(X, U, t, nsteps, mass, Isp, MU, DU, TU, 10.0, 50, state_0=s0, state_f=sf, ctx=ctx)
        print("indirect p = 2 from the direct solution, costates from the QP multipliers: status %d, max defect %.2e, %d full "
              "iterations (KKT residual of the seed %.1e)" % (r["status"][0], r["max_defect"][0], r["iterations"][0], r["kkt_res"][0]))
        res["costate_guess"] = (int(r["status"][0]), float(r["max_defect"][0]), int(r["iterations"][0]))
        if "indirect_iterations" in res:
            print("iterations: %d + %d with random costates, %d with the multipliers" % (*res["indirect_iterations"], r["iterations"][0]))
    return res


def refine_and_resolve(tol_max=1e-16, tol_min=None, max_nodes=120, maxIter=100, ctx=None, verbose=True):
    """Solve on the demo's 30 nodes, refine the mesh of the solution in one device call, solve again on the refined mesh (one
    lto_direct_solve call each).  Returns the figures it prints."""
    ctx = ctx or lto.default_context(0)
    tol_min = tol_max / 1000.0 if tol_min is None else tol_min
    X, U, t, tau1, tau2, t0s, X0s, tfs, Xfs = demo_problem()
    n, nsteps, Isp, mass = X.shape[1], 10, 2000.0, 1000.0

    def solve(X, U, t, n):
        out = drivers.multiShoot_CRTBP_direct(X, U, tau1, tau2, t, np.zeros(3), np.zeros(3), MU, DU, TU, n, nsteps, mass, Isp, t0s, X0s,
                                              tfs, Xfs, False, False, 0.0, False, maxIter, verbose=False)
        last = drivers.multiShoot_CRTBP_direct.last
        return out[0], out[1], out[4], last["status"], last["iterations"], float(np.abs(out[7]).max())

    X, U, t, st0, it0, d0 = solve(X, U, t, n)
    _, e0 = lto.direct_defectCalc(X, U, t, nsteps, MU, DU, TU, Isp, ctx=ctx)
    r = lto.direct_refine(X, U, t, nsteps, MU, DU, TU, Isp, tol_min, tol_max, max_nodes, ctx=ctx)
    X2, U2, t2, st, it, d = solve(r.X, r.U, r.t, r.n)
    _, e2 = lto.direct_defectCalc(X2, U2, t2, nsteps, MU, DU, TU, Isp, ctx=ctx)
    res = {"n_before": n, "n_after": r.n, "n_removed": r.n_removed, "passes": r.passes, "refine_status": r.status, "tol_max": tol_max,
           "max_error_before": float(e0.max()), "max_error_refined": float(r.errors.max()), "max_error_after": float(e2.max()),
           "first_status": st0, "first_iterations": it0, "first_max_defect": d0, "status": st, "iterations": it, "max_defect": d}
    if verbose:
        print("direct: status %d after %d iterations on %d nodes, max defect %.2e, max estimate %.2e" % (st0, it0, n, d0, e0.max()))
        print("refine (tol_min %.1e, tol_max %.1e): %d -> %d nodes (%d removed, %d insertion passes, status %d), max estimate %.2e"
              % (tol_min, tol_max, n, r.n, r.n_removed, r.passes, r.status, r.errors.max()))
        print("re-solve on %d nodes: status %d after %d iterations, max defect %.2e, max estimate %.2e" % (r.n, st, it, d, e2.max()))
    return res


def equidistribute_and_resolve(n_new=30, tol_max=1e-16, max_nodes=120, passes=2, w_floor=None, maxIter=100, ctx=None, verbose=True):
    """Solve on the demo's 30 nodes, refine the solution's mesh, resample it onto n_new nodes of equidistributed estimates and solve
    again on them (one device call each).  Returns the figures it prints."""
    ctx = ctx or lto.default_context(0)
    X, U, t, tau1, tau2, t0s, X0s, tfs, Xfs = demo_problem()
    n, nsteps, Isp, mass = X.shape[1], 10, 2000.0, 1000.0

    def solve(X, U, t, n):
        out = drivers.multiShoot_CRTBP_direct(X, U, tau1, tau2, t, np.zeros(3), np.zeros(3), MU, DU, TU, n, nsteps, mass, Isp, t0s, X0s,
                                              tfs, Xfs, False, False, 0.0, False, maxIter, verbose=False)
        last = drivers.multiShoot_CRTBP_direct.last
        return out[0], out[1], out[4], last["status"], last["iterations"], float(np.abs(out[7]).max())

    X, U, t, st0, it0, d0 = solve(X, U, t, n)
    _, e0 = lto.direct_defectCalc(X, U, t, nsteps, MU, DU, TU, Isp, ctx=ctx)
    r = lto.direct_refine(X, U, t, nsteps, MU, DU, TU, Isp, tol_max / 1000.0, tol_max, max_nodes, ctx=ctx)
    kw = {} if w_floor is None else {"w_floor": w_floor}
    Xe, Ue, te, rs = drivers.meshEquidistribute_direct(r, None, None, 6, None, nsteps, Isp, MU, DU, TU, int(n_new), passes=passes, ctx=ctx, **kw)
    eq = drivers.meshEquidistribute_direct.last
    X2, U2, t2, st, it, d = solve(Xe, Ue, te, int(n_new))
    _, e2 = lto.direct_defectCalc(X2, U2, t2, nsteps, MU, DU, TU, Isp, ctx=ctx)
    res = {"n_before": n, "n_refined": r.n, "n_after": int(n_new), "resample_status": int(rs), "first_status": st0,
           "max_error_before": float(e0.max()), "min_error_before": float(e0.min()), "max_error_refined": float(r.errors.max()),
           "min_error_refined": float(r.errors.min()), "max_error_resampled": float(eq.errors_after.max()),
           "min_error_resampled": float(eq.errors_after.min()), "max_error_after": float(e2.max()), "min_error_after": float(e2.min()),
           "status": st, "iterations": it, "max_defect": d}
    if verbose:
        print("direct: status %d after %d iterations on %d nodes, max defect %.2e, estimates %.2e .. %.2e" % (st0, it0, n, d0, e0.min(), e0.max()))
        print("refine (tol_max %.1e): %d -> %d nodes, estimates %.2e .. %.2e" % (tol_max, n, r.n, r.errors.min(), r.errors.max()))
        print("equidistribute (%d passes): %d -> %d nodes (status %d), estimates of the guess %.2e .. %.2e" % (
            passes, r.n, n_new, rs, eq.errors_after.min(), eq.errors_after.max()))
        print("re-solve on %d nodes: status %d after %d iterations, max defect %.2e, estimates %.2e .. %.2e" % (n_new, st, it, d, e2.min(), e2.max()))
    return res


def multi_start(n_starts, n_nodes=30, tof_days=20.0, maxIter=100, verbose=True):
    """n_starts departure phases over [0, 1), the demo's setting otherwise (flagEnd = false); returns drivers.multiStart_direct's dict."""
    tabs = synth.halo_orbits()
    times = [np.linspace(0.0, 1.0, tb.shape[1]) for tb in tabs]
    tof = 0.5 * tof_days * lto.day / TU
    tau1s = np.arange(int(n_starts)) / float(n_starts)
    t0 = time.perf_counter()
    m = drivers.multiStart_direct(tau1s, tof, tof, n_nodes, 10, 1000.0, 2000.0, times[0], tabs[0], times[1], tabs[1], MU, DU, TU,
                                  flagEnd=False, maxIter=maxIter)
    if verbose:
        print("multi-start: %d starts, %d converged (%.2f s)" % (tau1s.size, m["order"].size, time.perf_counter() - t0))
        for rank, b in enumerate(m["order"]):
            print("  %2d. tau1 = %.4f, tau2 = %.3f, cost %.6f, %d iterations, max defect %.2e, junction gap %.3e" % (
                rank + 1, m["tau"][0, b], m["tau"][1, b], m["cost"][b], m["iterations"][b], m["max_defect"][b], m["gap"][0, b]))
    return m


def _arg(flag, default):
    """Value after `flag` (a number), the default if absent or not followed by a number, None if the flag is absent."""
    if flag not in sys.argv:
        return None
    k = sys.argv.index(flag)
    try:
        return float(sys.argv[k + 1])
    except (IndexError, ValueError):
        return default


if __name__ == "__main__":
    if "--refine" in sys.argv:
        refine_and_resolve(tol_max=_arg("--refine", 1e-16))
        sys.exit(0)
    if "--equidistribute" in sys.argv:
        equidistribute_and_resolve(int(_arg("--equidistribute", 30)))
        sys.exit(0)
    if "--multi-start" in sys.argv:
        multi_start(int(_arg("--multi-start", 8)))
        sys.exit(0)
    free = _arg("--free-ends", 0.0)
    off = _arg("--tau2-offset", 0.02)
    if off is None:
        off = 0.02 if free is not None else 0.0
    free_tf = _arg("--free-tf", 1.0)
    if free_tf is not None and free is None:
        free = 0.0                                        # a free tf moves on the free-end iterations
    main(verbose="-q" not in sys.argv, then_indirect="--then-indirect" in sys.argv, python_loop="--python-loop" in sys.argv,
         free_ends=free, tau2_offset=off, free_tf=free_tf, ballistic="--ballistic-guess" in sys.argv,
         costate_guess="--costate-guess" in sys.argv)
