"""The three addTimeFinal kernels (k_remesh_spline, k_find_tau, k_dense_cost; kernels_addtime.hip) across their shapes, each against
a restatement more precise than the kernel (tests/dense_reference.py).  The input is synth.indirect_problem's nodes on the arrival
orbit's table, not a converged transfer: every comparison is with a restatement of the same steps.  The dense output that feeds
them is pinned against the oracle in test_dense_shapes_gpu.py; the end-to-end convergence tests stay in test_add_time_gpu.py.

Re-mesh   (n, n_desired) in dense_reference.REMESH_PAIRS -- n = 2 (no interior node), n > n_desired, n - 1 dividing n_desired - 1
          (new nodes on knots) -- each with K = 1, 6 and 11 flight-time changes (12, 72 and 132 lanes in workgroups of 64), DOP853 and
          RK4 x 64.  Expected: the long-double natural spline of lto.densify of the extended trajectory, per-row relative 1e-12; node 0,
          the zero end costates, the new grid and its end bit for bit.
Snap      the last node set to the device's own s(tau_j), j in {0, 1, 63, 64, 255, 256, 257, 511, 512, 999, 1000}, and a coast of
          1e-11 TU: the device's index is numpy's first arg-min over the device's 1001 candidates (ties within 1e-15 allowed, as in
          test_add_time_gpu.py), G[:6, -1] is s(tau*) to 1e-15, tau * 1000 is an integer.  The halo table is closed to 1.6e-9 only, so
          on it candidate 1000 wins its own case; on a copy whose last column is set equal to its first the device's s(0) and s(1)
          agree to rounding and the same rule decides between 0 and 1000.  A last node of NaN gives tau = 0 and s(0).
Cost      maxIter = 0 (the loop is not entered: XC_out is the guess), K = 3, n_desired in {4, 65}, p = 0, p = 1 (rho 1 and 0.1), and
          p = 2, 1.5, 3 at 0.05 N with samples on both sides of the clamp (asserted): relative 1e-12 against the long-double
          trapezoid of lto.densify of XC_out.

Largest differences measured on an MI355X (device against reference, bar beside it):
  re-mesh, per-row relative, 28 tests x 18 trajectories   4.6e-15   (1e-12)   at 30 nodes from 257 knots, RK4 x 64, p = 1
  cost, relative, 12 tests x 3 trajectories               1.2e-15   (1e-12)
  snap: every winner is numpy's own; onto candidate 1000 of the halo table d[0] = 2.1e-9, d[1000] = 1.2e-11, both take 1000"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import addtime_reference as R  # noqa: E402
import dense_reference as D  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402

pytestmark = pytest.mark.gpu

TAUS = np.arange(1001) / 1000.0


def _params(p=2.0, rho=1.0, thrust=10.0):
    return lto.make_params(MU, DU, TU, thrust, D.MASS, 1.0, p, rho)


def _rel_err(a, b):
    """max over components of |a - b| / max |b| (per component row): test_add_time_gpu.py's measure."""
    scale = np.maximum(np.abs(b).max(axis=1, keepdims=True), 1e-300)
    return float((np.abs(a - b) / scale).max())


def _integ(mname):
    method, steps = D.METHODS[mname]
    return lto.integrator(method, steps=steps)


def _candidates(ctx, times, tab):
    """The device's own s(j / 1000), [6 x 1001]."""
    _, S, _, _, _, _ = lto.direct_end_states(np.vstack([TAUS, TAUS]), (times, tab, times, tab), ctx=ctx)
    return np.array(S)


@pytest.mark.parametrize("mname", ["dop853", "rk4x64"])
@pytest.mark.parametrize("n,m", D.REMESH_PAIRS, ids=["%dfrom%d" % q for q in D.REMESH_PAIRS])
def test_remesh_shapes(gpu_ctx, n, m, mname):
    times, tab = D.arrival_table()
    XC, t = D.addtime_problem(n)
    p = 1.0 if D.REMESH_PAIRS.index((n, m)) % 2 else 2.0
    prm, integ = _params(p), _integ(mname)
    worst = 0.0
    for K in D.REMESH_K:
        dts = D.add_time_dts(K)
        r = lto.indirect_add_time(XC, t, prm, times, tab, dts, n_desired=m, integ=integ, solve=False, ctx=gpu_ctx)
        assert r.XC_out is None and r.XC_guess.shape == (12, n, K) and r.t_out.shape == (n, K)
        for k, dt in enumerate(dts):
            G = r.XC_guess[:, :, k]
            XCe, te = R.extended(XC, t, dt)
            XCd, td = lto.densify(XCe, te, prm, m, integ, ctx=gpu_ctx)
            t_new = R.linrange(td[0], td[-1], n)
            want = D.natural_spline_ld(td, XCd, t_new)
            assert np.array_equal(r.t_out[:, k], t_new)
            assert r.t_out[-1, k] == t[-1] + dt
            assert np.array_equal(G[:, 0], XC[:, 0])                  # bit for bit
            assert np.all(G[6:, -1] == 0.0)
            assert np.all(np.isfinite(G))
            if (m - 1) % (n - 1) == 0:
                assert np.all(np.isin(t_new, td))                     # every new node falls on a knot
            e = _rel_err(G[6:, -1:], want[6:, -1:])
            if n > 2:
                e = max(e, _rel_err(G[:, :-1], want[:, :-1]))
            worst = max(worst, e)
    print("re-mesh %d nodes from %d knots, %s, p = %g: worst per-row relative difference %.2e (bar 1e-12)" % (n, m, mname, p, worst))
    assert worst < 1e-12


def _snap(ctx, times, tab, S, j, integ=None):
    """One call with the last node at s(tau_j): (result, XCd of the extended trajectory, its numpy winner and distances)."""
    XC, t = D.addtime_problem(5)
    XC[:6, -1] = S[:, j]
    r = lto.indirect_add_time(XC, t, _params(), times, tab, [D.SNAP_DT], n_desired=8, integ=integ, solve=False, ctx=ctx)
    XCe, te = R.extended(XC, t, D.SNAP_DT)
    XCd, _ = lto.densify(XCe, te, _params(), 8, integ, ctx=ctx)
    return r, XCd, R.find_tau_from_samples(S, XCd[:6, -1])


@pytest.mark.parametrize("closed", [False, True], ids=["table", "closed-table"])
def test_snap_winner_at_the_stride_and_wave_edges(gpu_ctx, closed):
    times, tab = D.arrival_table()
    if closed:
        tab = tab.copy(order="F")
        tab[:, -1] = tab[:, 0]                                        # s(0) and s(1) agree to rounding: candidates 0 and 1000 all but tie
    S = _candidates(gpu_ctx, times, tab)
    assert (np.abs(S[:, 0] - S[:, 1000]).max() <= 1e-15) == closed
    for j in (D.SNAP_J if not closed else (0, 1000)):
        r, XCd, (jn, d) = _snap(gpu_ctx, times, tab, S, j)
        assert np.abs(XCd[:6, -1] - S[:, j]).max() <= 1e-8            # the coast is far inside the 1e-3 candidate spacing
        tau = r.tau[0]
        assert tau * 1000.0 == np.round(tau * 1000.0)
        jd = int(round(tau * 1000.0))
        if j == 1000:
            print("snap onto candidate 1000, %s: numpy's first arg-min is %d (d[0] = %.3e, d[1000] = %.3e), the device's %d" % (
                "closed table" if closed else "table", jn, d[0], d[1000], jd))
            assert closed or jn == 1000
        elif not closed:
            assert jn == j
        assert jn in ((0, 1000) if closed else (j,))
        assert jd == jn or abs(d[jd] - d[jn]) <= 1e-15, (j, jd, jn, d[jd], d[jn])
        _, sf, _, _, _, _ = lto.direct_end_states([tau, tau], (times, tab, times, tab), ctx=gpu_ctx)
        G = r.XC_guess[:, :, 0]
        assert np.abs(G[:6, -1] - sf).max() <= 1e-15 * max(1.0, np.abs(sf).max())
        assert np.all(G[6:, -1] == 0.0)


def test_snap_of_a_nan_end_takes_candidate_zero(gpu_ctx):
    """Every distance is NaN: j = 0, as k_find_tau's comment promises.  RK4, so that no adaptive loop sees the NaN."""
    times, tab = D.arrival_table()
    XC, t = D.addtime_problem(5)
    XC[:6, -1] = np.nan
    r = lto.indirect_add_time(XC, t, _params(), times, tab, [0.01], n_desired=8, integ=_integ("rk4x64"), solve=False, ctx=gpu_ctx)
    s0, _, _, _, _, _ = lto.direct_end_states([0.0, 0.0], (times, tab, times, tab), ctx=gpu_ctx)
    assert r.tau[0] == 0.0
    assert np.array_equal(r.XC_guess[:6, -1, 0], s0)
    assert np.array_equal(r.XC_guess[:, 0, 0], XC[:, 0])


@pytest.mark.parametrize("m", D.COST_M)
@pytest.mark.parametrize("p,rho,thrust,lam_sigma,seed", D.COST_CASES, ids=["p%g-rho%g" % c[:2] for c in D.COST_CASES])
def test_cost_branches(gpu_ctx, p, rho, thrust, lam_sigma, seed, m):
    times, tab = D.arrival_table()
    XC, t = D.addtime_problem(D.COST_N, seed=seed, lam_sigma=lam_sigma)
    prm = _params(p, rho, thrust)
    dts = D.add_time_dts(D.COST_K)
    r = lto.indirect_add_time(XC, t, prm, times, tab, dts, n_desired=m, maxIter=0, ctx=gpu_ctx)
    assert np.array_equal(r.XC_out, r.XC_guess)                     # maxIter = 0: the loop is not entered
    aL = D.thrust_accel(thrust)
    worst = 0.0
    for k in range(D.COST_K):
        XCd, td = lto.densify(r.XC_out[:, :, k], r.t_out[:, k], prm, m, ctx=gpu_ctx)
        want, u = D.dense_cost_ld(XCd, td, thrust, p, rho, D.MASS, DU, TU)
        assert np.all(np.isfinite(XCd)) and want > 0.0
        if p > 1.0:
            hi, lo = D.clamp_sides(u, aL)
            assert hi >= 1 and lo >= 1, (k, u / aL)                   # both branches of the clamp are run
        elif p == 1.0:
            assert u.min() > 0.0 and u.max() > 1.01 * u.min()              # the tanh branch, not a constant
        else:
            assert want == pytest.approx(aL * (td[-1] - td[0]), rel=1e-14)
        worst = max(worst, abs(r.cost[k] - want) / abs(want))
    print("cost p = %g, rho = %g, %g N, %d samples: worst relative difference %.2e (bar 1e-12)" % (p, rho, thrust, m, worst))
    assert worst <= 1e-12
