"""The kernels of the 14-row addTimeFinal (k_remesh_spline<14>, k_dense_cost_mass; kernels_addtime.hip) across their
shapes, and the tail of step 1 as the device integrates it.  The nodes are mass_dense_reference.fixture's -- on one trajectory of the
oracle's flow, not a converged transfer: every comparison is with a restatement of the same steps.

Re-mesh   (n, n_desired) in addtime_mass_reference.SHAPES, K = 1, 4, 5, 9 flight-time changes (14, 56, 70, 126 lanes in workgroups of
          64: inside one, just below and just above it, into the second), DOP853 and RK4 x 8, parameter sets p1, p2-10N and p0-isp20.
          Expected: addtime_reference.remesh of lto.densify_mass of the extended trajectory, per-row relative 1e-12 (the same
          arithmetic on the same samples: the bar of test_add_time_gpu.py); the new grid, node 0 and rows 7..13 of the last node bit
          for bit; the mass of the last node is the dense output's last sample.  The K = 9 call goes through the C entry with 16
          sentinel doubles on both sides of XC_guess, t_out and tau_out.
Tail      lto.densify_mass of the extended trajectory: on every sample past t[n-1] rows 7..13 are exactly 0; p > 1: the mass row
          bit-constant; p = 0: the loss at t_end against thrustLimit / (Isp 9.81) TU dt to 1e-13 relative, and at every tail sample
          to 1e-13 of that whole loss (relative to a sample's own, smaller loss the rounding of a mass near 900 kg alone is more);
          all 14 rows against the oracle's flow of the zeroed last node at mass_dense_reference.TOL, the mass row to mass_bar besides
          (DOP853 from the node; RK4 x 64 hop by hop against the oracle's RK4 x 64.  Its linear loss is held to hops x 64 eps m0 kg
          instead, mass_bar's own floor of one rounding of a mass below m0 per fixed step, carried over the 14 hops: 2.0e-10 kg,
          which is beyond 1e-13 of a 22 kg loss by construction; measured 8.8e-11 kg).
Cost      maxIter = 0 (XC_out is the guess bit for bit), K = 3, n_desired in {4, 65}: p = 0, p = 1 (rho 1 and 0.1), p = 2 unclamped,
          p = 3 clamped (the class asserted on the first sample), relative 1e-12 against the long-double trapezoid of lto.densify_mass
          of XC_out with every sample's own mass.

Every test prints its figures before it asserts (MEASURED lines)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import addtime_mass_reference as AM  # noqa: E402
import addtime_reference as R  # noqa: E402
import dense_reference as D  # noqa: E402
import mass_dense_reference as M  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import hotpath  # noqa: E402
from lowthrustopt_amd.constants import DU, TU, day  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e77
GUARD = 16
SETS = (0, 2, 5)                                     # p1, p2-10N, p0-isp20


def _integ(mname):
    method, steps = M.METHODS[mname]
    return lto.integrator(method, steps=steps)


def _rel_err(a, b):
    """max over components of |a - b| / max |b| (per component row): test_add_time_gpu.py's measure."""
    scale = np.maximum(np.abs(b).max(axis=1, keepdims=True), 1e-300)
    return float((np.abs(a - b) / scale).max())


def _guarded(count):
    buf = np.full(count + 2 * GUARD, SENTINEL)
    return buf, buf[GUARD:GUARD + count]


def _raw_guess(ctx, X, t, prm, integ, times, tab, dts, m):
    """lto_indirect_add_time_mass_batch through the C entry, guesses only, every output between sentinels."""
    n, K = t.size, dts.size
    X = np.asfortranarray(X)
    ob = hotpath.DirectOrbits(times, tab, times, tab)
    bufs = [_guarded(14 * n * K), _guarded(n * K), _guarded(K)]
    rc = ctx.fn("indirect_add_time_mass_batch")(
        ctx.handle, n, X.ctypes.data, t.ctypes.data, ctypes.byref(prm), ctypes.byref(integ), ctypes.byref(ob.struct), K, dts.ctypes.data,
        m, 0, 10, bufs[0][1].ctypes.data, None, bufs[1][1].ctypes.data, bufs[2][1].ctypes.data, None, None, None, None, None, None)
    assert rc == 0
    for buf, inner in bufs:
        assert np.all(buf[:GUARD] == SENTINEL) and np.all(buf[-GUARD:] == SENTINEL)
        assert not np.any(inner == SENTINEL)
    return (bufs[0][1].reshape((14, n, K), order="F"), bufs[1][1].reshape((n, K), order="F"), bufs[2][1])


@pytest.mark.parametrize("k", SETS, ids=lambda k: M.SETS[k].name)
@pytest.mark.parametrize("mname", ["dop853", "rk4x8"])
@pytest.mark.parametrize("n,m", AM.SHAPES, ids=["%dfrom%d" % q for q in AM.SHAPES])
def test_remesh_shapes(gpu_ctx, n, m, mname, k):
    times, tab = D.arrival_table()
    X, t, prm_l = M.fixture(n, k)
    X, t = np.asfortranarray(X), np.array(t)
    prm, integ = lto.make_params(*prm_l), _integ(mname)
    worst = 0.0
    for K in AM.SHAPE_K:
        dts = D.add_time_dts(K)
        r = lto.indirect_add_time_mass(X, t, prm, times, tab, dts, n_desired=m, integ=integ, solve=False, ctx=gpu_ctx)
        assert r.XC_out is None and r.propellant is None and r.XC_guess.shape == (14, n, K) and r.t_out.shape == (n, K)
        if K == AM.SHAPE_K[-1]:
            G_raw, t_raw, tau_raw = _raw_guess(gpu_ctx, X, t, prm, integ, times, tab, dts, m)
            assert np.array_equal(G_raw, r.XC_guess) and np.array_equal(t_raw, r.t_out) and np.array_equal(tau_raw, r.tau)
        for j, dt in enumerate(dts):
            G = r.XC_guess[:, :, j]
            XCe, te = AM.extended14(X, t, dt)
            XCd, td = lto.densify_mass(XCe, te, prm, m, integ, ctx=gpu_ctx)
            want, t_new = R.remesh(XCd, td, n)
            assert np.array_equal(r.t_out[:, j], t_new)
            assert r.t_out[-1, j] == t[-1] + dt
            assert np.array_equal(G[:, 0], X[:, 0])                  # bit for bit
            assert np.all(G[7:, -1] == 0.0)
            assert np.all(np.isfinite(G))
            e = _rel_err(G[6:, -1:], want[6:, -1:])                  # rows 0..5 of the last node are snapped
            if n > 2:
                e = max(e, _rel_err(G[:, :-1], want[:, :-1]))
            worst = max(worst, e)
    print("MEASURED re-mesh %d nodes from %d knots, %s, %s: worst per-row relative difference %.2e (bar 1e-12)" % (n, m, mname, M.SETS[k].name, worst))
    assert worst < 1e-12


@pytest.mark.parametrize("mname", ["dop853", "rk4x64"])
@pytest.mark.parametrize("k", [0, 2, 3, 5], ids=lambda k: M.SETS[k].name)
def test_tail_through_the_device(gpu_ctx, oracle, k, mname):
    X, t, prm_l = M.fixture(9, k)
    s = M.SETS[k]
    _, e_m = M.self_errors()
    dt = day / TU
    XCe, te = AM.extended14(X, t, dt)
    XCd, td = lto.densify_mass(XCe, te, lto.make_params(*prm_l), 65, _integ(mname), ctx=gpu_ctx)
    tail = np.flatnonzero(td > t[-1])
    assert tail.size >= 5 and td[-1] == t[-1] + dt
    assert np.all(XCd[7:14, tail] == 0.0)                              # exactly
    y0 = XCe[:, -2]
    assert np.all(y0[7:14] == 0.0) and np.array_equal(y0[:7], X[:7, -1])
    # DOP853: from the node.  RK4 x 64: hop by hop from the device's own previous sample with the oracle's RK4 of the same step count,
    # as mass_dense_reference compares that method -- a chain of 14 hops x 64 fixed steps adds the same small decrement to a mass
    # near 1000 kg 896 times, and its roundings (measured from the node: 1.2e-10 kg) are the method's, not the tail's
    method, steps = M.METHODS[mname]
    want = np.zeros((14, tail.size))
    prev, tprev = y0, t[-1]
    for i, j in enumerate(tail):
        want[:, i] = M.flow14(oracle, prev, prm_l, td[j] - tprev, method, steps)
        if mname != "dop853":
            prev, tprev = XCd[:, j], td[j]
    err = M.rel_rows(XCd[:, tail], want)
    em = float(np.abs(XCd[6, tail] - want[6]).max())
    print("MEASURED tail %s %s: %d samples, rows 0..13 against the oracle's flow %.3e (bar %.0e), mass row %.3e kg (bar %.3e kg)"
          % (s.name, mname, tail.size, err, M.TOL[mname], em, M.mass_bar(e_m)))
    assert err <= M.TOL[mname]
    assert em <= M.mass_bar(e_m)
    if s.p > 1.0:
        assert np.all(XCd[6, tail] == X[6, -1])                        # umag(0, m) = 0: bit for bit
    elif s.p == 0.0:
        rate = s.thrust / (s.isp * 9.81) * TU
        loss = X[6, -1] - XCd[6, tail]
        lin = rate * (td[tail] - t[-1])
        rel_end = abs(loss[-1] - lin[-1]) / lin[-1]
        rel_all = float(np.abs(loss - lin).max() / lin[-1])
        print("MEASURED tail %s %s: loss at t_end %.12f kg, against the linear law %.3e relative, every sample %.3e of it (bar 1e-13)"
              % (s.name, mname, loss[-1], rel_end, rel_all))
        if mname == "dop853":                                          # the bar is DESIGN 4.19's, for the adaptive integrator's few steps
            assert rel_end <= 1e-13 and rel_all <= 1e-13
        else:                                                          # one rounding of a mass below m0 per fixed step
            assert float(np.abs(loss - lin).max()) <= tail.size * steps * M.EPS * M.M0
    else:
        assert np.all(np.diff(XCd[6, tail]) < 0.0)                     # the law's idle flow


COST_SETS = (5, 0, 1, 2, 3)                          # p = 0, p = 1 (rho 1, rho 0.1), p = 2 unclamped, p = 3 clamped


@pytest.mark.parametrize("m", [4, 65])
@pytest.mark.parametrize("k", COST_SETS, ids=lambda k: M.SETS[k].name)
def test_cost_branches(gpu_ctx, k, m):
    times, tab = D.arrival_table()
    X, t, prm_l = M.fixture(9, k)
    s = M.SETS[k]
    prm = lto.make_params(*prm_l)
    dts = D.add_time_dts(3)
    r = lto.indirect_add_time_mass(X, t, prm, times, tab, dts, n_desired=m, maxIter=0, ctx=gpu_ctx)
    assert np.array_equal(r.XC_out, r.XC_guess)                     # maxIter = 0: the loop is not entered
    assert np.array_equal(r.propellant, X[6, 0] - r.XC_out[6, -1, :])
    worst = 0.0
    for j in range(3):
        XCd, td = lto.densify_mass(r.XC_out[:, :, j], r.t_out[:, j], prm, m, ctx=gpu_ctx)
        want, u = AM.dense_cost14(XCd, td, s.thrust, s.p, s.rho, DU, TU)
        aL = AM.c_thrust(s.thrust, DU, TU) / XCd[6]
        assert np.all(np.isfinite(XCd)) and want > 0.0
        assert aL.max() > aL.min()                                    # the mass moves: a frozen aL would not pass
        if s.p == 0.0:
            assert np.array_equal(u, aL)
        elif s.p == 1.0:
            assert u.min() > 0.0 and np.all(u < aL) and (u / aL).max() > 1.01 * (u / aL).min()      # the tanh branch, not a constant
        elif s.p == 2.0:
            assert 0.0 < u[0] < aL[0]                                 # the unclamped branch
        else:
            assert u[0] == aL[0]                                      # the clamp
        worst = max(worst, abs(r.cost[j] - want) / abs(want))
    print("MEASURED cost %s, %d samples: worst relative difference %.2e (bar 1e-12)" % (s.name, m, worst))
    assert worst <= 1e-12
