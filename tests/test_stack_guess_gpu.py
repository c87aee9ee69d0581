"""GPU checks of the stacked initial guess on the device (lto_stack_guess_batch): every stored node against the
oracle's flow of the node before it, the end nodes against the device's own table spline bit for bit, the two find_tau searches
against the host distances, the whole guess against the host restatement (tests/stack_reference.py) within the trajectory's own
measured sensitivity, batch == singles, a start that runs out of steps, the refusals, and the guess fed to the direct solve.
The starts are those of stack_reference.CASES, vetted on the host (tests/test_stack_guess_host.py).

Figures measured on an MI355X are in the CHANGELOG entry of this call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import addtime_reference as R  # noqa: E402
import stack_reference as SR  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU, day  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_DOP853, TOL_RK4 = 1e-11, 1e-10          # node to node, the bars of test_densify_vs_oracle (test_gpu_parity.py)
SHORT_HOP = 0.0011 * day / TU               # a recovery flow this short is exact to rounding (one step, local error << 1e-16)


@pytest.fixture(scope="module")
def tables():
    tabs = synth.halo_orbits()
    return tuple(v for tb in tabs for v in (np.linspace(0.0, 1.0, tb.shape[1]), np.asfortranarray(tb[:6])))


@pytest.fixture(scope="module")
def cand(gpu_ctx, tables):
    """The device's own s(j / 1000) of the arrival table, [6 x 1001]."""
    _, sf, _, _, _, _ = lto.direct_end_states(np.vstack([SR.TAUS, SR.TAUS]), tables, ctx=gpu_ctx)
    return np.array(sf)


def _flow(oracle, rtol=1e-13):
    def flow(x, span):
        y, _ = oracle.flow_prop_ep(x, np.zeros(3), 1.0, span, oracle.DOP853_ADAPTIVE, 0, MU, DU, TU, 2000.0, rtol, rtol)
        return y
    return flow


def _case(name):
    n, tau1, d1, d2 = SR.CASES[name]
    return n, tau1, d1 * day / TU, d2 * day / TU


_GUESS = {}


def _guess(gpu_ctx, tables, name, rk4=False):
    """The device's guess of a case, computed once and shared (never modified)."""
    key = (name, rk4)
    if key not in _GUESS:
        n, tau1, tof1, tof2 = _case(name)
        integ = lto.integrator(lto.RK4, steps=64) if rk4 else None
        _GUESS[key] = lto.stack_guess(tau1, tof1, tof2, n, tables, integ=integ, ctx=gpu_ctx)
    return _GUESS[key]


NODE_CASES = [(name, False) for name in sorted(SR.CASES)] + [("rk4_short", True)]


@pytest.mark.parametrize("name,rk4", NODE_CASES, ids=["%s%s" % (c, "-rk4" if r else "") for c, r in NODE_CASES])
def test_nodes_follow_the_oracle_flow_node_to_node(gpu_ctx, oracle, tables, name, rk4):
    n, tau1, tof1, tof2 = _case(name)
    g = _guess(gpu_ctx, tables, name, rk4)
    tol = TOL_RK4 if rk4 else TOL_DOP853
    flow = _flow(oracle)
    assert g.status == 0 and g.X.shape == (6, n) and np.all(np.isfinite(g.X))
    assert np.array_equal(g.t, R.linrange(0.0, tof1 + tof2, n))
    assert g.tau1 == SR.wrap(tau1)
    for tau in (g.tau2_0, g.tau2):
        assert 0.0 <= tau <= 1.0 and tau * 1000.0 == np.round(tau * 1000.0)
    s0, sf0, _, _, _, _ = lto.direct_end_states([tau1, g.tau2_0], tables, ctx=gpu_ctx)
    _, sf, _, _, _, _ = lto.direct_end_states([tau1, g.tau2], tables, ctx=gpu_ctx)
    assert np.array_equal(g.X[:, 0], s0)                              # bit for bit
    assert np.array_equal(g.X[:, n - 1], sf)                          # bit for bit
    n1 = int(np.count_nonzero(g.t < tof1))
    worst = 0.0
    for k in range(n - 2):                                            # node n-1 is the snap, not a flow
        if k + 1 == n1:
            continue                                                  # the junction: arc 2 does not continue arc 1
        ref = flow(g.X[:, k], g.t[k + 1] - g.t[k])
        worst = max(worst, np.abs(g.X[:, k + 1] - ref).max() / max(1.0, np.abs(ref).max()))
    if n1 < n - 1:                                                    # the first node of arc 2, where it is not the last node
        span = g.t[n1] - tof1
        if span == 0.0:
            assert np.array_equal(g.X[:, n1], sf0)                    # bit for bit
        else:
            ref = flow(sf0, span)                                     # the first node of arc 2 is the flow of sf(tau2_0)
            worst = max(worst, np.abs(g.X[:, n1] - ref).max() / max(1.0, np.abs(ref).max()))
    print("%s%s: n1 = %d, tau = (%.3f, %.3f, %.3f), worst node-to-node difference %.2e (bar %.0e)" % (
        name, " rk4" if rk4 else "", n1, g.tau1, g.tau2_0, g.tau2, worst, tol))
    assert worst <= tol


def test_rk4_nodes_equal_the_oracles_rk4(gpu_ctx, oracle, tables):
    """The demo's grid with RK4 x 64 against the oracle's RK4 x 64 from the same node: the same method and step, so what is left is
    rounding -- 64 steps of a few ulp each on O(1) states; 1e-12 leaves two orders.  (Against the adaptive oracle these 0.16 TU
    hops show RK4's own truncation error, which is no property of the kernel; that comparison is made on the rk4_short case.)"""
    n, tau1, tof1, tof2 = _case("demo")
    g = _guess(gpu_ctx, tables, "demo", True)
    assert g.status == 0
    n1 = int(np.count_nonzero(g.t < tof1))
    worst = trunc = 0.0
    for k in range(n - 2):
        if k + 1 == n1:
            continue
        span = g.t[k + 1] - g.t[k]
        ref, _ = oracle.flow_prop_ep(g.X[:, k], np.zeros(3), 1.0, span, oracle.RK4, 64, MU, DU, TU, 2000.0)
        worst = max(worst, np.abs(g.X[:, k + 1] - ref).max() / max(1.0, np.abs(ref).max()))
        trunc = max(trunc, np.abs(g.X[:, k + 1] - _flow(oracle)(g.X[:, k], span)).max())
    print("demo rk4: worst difference to the oracle's RK4 x 64 %.2e (bar 1e-12); to the adaptive oracle %.2e" % (worst, trunc))
    assert worst <= 1e-12


def test_wrapped_phases_give_the_same_bits(gpu_ctx, tables):
    base = _guess(gpu_ctx, tables, "n5_4_8")
    for name in ("wrap_hi", "wrap_lo"):
        g = _guess(gpu_ctx, tables, name)
        assert g.tau1 == 0.75
        assert np.array_equal(g.X, base.X) and np.array_equal(g.t, base.t) and np.array_equal(g.gap, base.gap)
        assert (g.tau2_0, g.tau2) == (base.tau2_0, base.tau2)


@pytest.mark.parametrize("name", sorted(SR.CASES))
def test_the_two_searches(gpu_ctx, oracle, tables, cand, name):
    """The device's winner against the host distances from the device's own candidates to the searched point.  Neither point is
    an output: the end of arc 1 is recovered as the oracle's flow of the last arc-1 node to tof1, node n-1 before its snap as the
    flow of the stored state before it.  The recovered point carries the difference of the two integrators over that hop, and
    a distance moves by at most as much as its point: so gap_out must equal d[jd] to the larger of 1e-12 relative (the search's
    own bar, which governs where the hop is a thousandth of a day: the *_late cases) and ten times the hop's own sensitivity,
    measured as the difference of the oracle's flows at 1e-13 and 1e-14 (the margin of the whole-guess comparison below)."""
    n, tau1, tof1, tof2 = _case(name)
    g = _guess(gpu_ctx, tables, name)
    n1 = int(np.count_nonzero(g.t < tof1))
    _, sf0, _, _, _, _ = lto.direct_end_states([tau1, g.tau2_0], tables, ctx=gpu_ctx)
    hop0 = (g.X[:, n1 - 1], tof1 - g.t[n1 - 1])
    hop1 = (g.X[:, n - 2], g.t[n - 1] - g.t[n - 2]) if n - 2 >= n1 else (sf0, g.t[n - 1] - tof1)
    for which, (x, span), tau in ((0, hop0, g.tau2_0), (1, hop1, g.tau2)):
        p13, p14 = _flow(oracle, 1e-13)(x, span), _flow(oracle, 1e-14)(x, span)
        sens = np.abs(p13 - p14).max()
        j, d = R.find_tau_from_samples(cand, p13)
        jd = int(round(tau * 1000.0))
        tol = max(1e-12 * d[jd], 10.0 * sens)
        print("%s search %d: hop %.3e TU, sensitivity %.2e, jd = %d, argmin = %d, gap %.15e, host %.15e, difference %.2e (bar %.2e)"
              % (name, which, span, sens, jd, j, g.gap[which], d[jd], abs(g.gap[which] - d[jd]), tol))
        assert jd == j or abs(d[jd] - d[j]) <= 1e-15, (name, which, jd, j, d[jd], d[j])
        if which == 0 and name.endswith("_late"):
            assert span <= SHORT_HOP and tol == 1e-12 * d[jd]      # the junction search at its own precision
        assert abs(g.gap[which] - d[jd]) <= tol, (name, which)


@pytest.mark.parametrize("name", [c for c in sorted(SR.CASES) if not c.startswith("wrap")])
def test_whole_guess_against_the_restatement(gpu_ctx, oracle, tables, cand, name):
    """stack_reference with the oracle's DOP853 from the same start state and candidates: the same two indices, and every node
    within ten times the trajectory's own sensitivity -- the largest node difference between the restatement at oracle
    tolerances 1e-13 and 1e-14 (one order for a different step-size controller history)."""
    n, tau1, tof1, tof2 = _case(name)
    g = _guess(gpu_ctx, tables, name)
    r13 = SR.stack(tau1, tof1, tof2, n, *tables, _flow(oracle, 1e-13), S=cand, x0=g.X[:, 0])
    r14 = SR.stack(tau1, tof1, tof2, n, *tables, _flow(oracle, 1e-14), S=cand, x0=g.X[:, 0])
    assert r13.j == r14.j
    assert (g.tau2_0, g.tau2) == (r13.tau2_0, r13.tau2)
    assert np.array_equal(g.t, r13.t)
    sens = np.abs(r13.X - r14.X).max()
    diff = np.abs(g.X - r13.X).max()
    print("%s: sensitivity of the restatement %.3e, device - restatement %.3e" % (name, sens, diff))
    assert diff <= 10.0 * sens


def test_batch_equals_singles(gpu_ctx, tables):
    """B = 65, one lane past a wavefront: distinct starts whose arcs hold different numbers of nodes."""
    B, n = 65, 6
    k = np.arange(B)
    tau1 = (0.013 * k + 0.05) % 1.0
    tof1 = (1.0 + 0.17 * k) * day / TU                                # 1 .. 11.9 days
    tof2 = (12.0 - 0.11 * k) * day / TU
    gb = lto.stack_guess(tau1, tof1, tof2, n, tables, ctx=gpu_ctx)
    assert gb.X.shape == (6, n, B) and gb.t.shape == (n, B) and gb.gap.shape == (2, B)
    assert np.array_equal(gb.status, np.zeros(B))
    assert len({int(np.count_nonzero(gb.t[:, b] < tof1[b])) for b in range(B)}) >= 3
    for b in range(B):
        g1 = lto.stack_guess(tau1[b], tof1[b], tof2[b], n, tables, ctx=gpu_ctx)
        assert np.array_equal(gb.X[:, :, b], g1.X) and np.array_equal(gb.t[:, b], g1.t), b
        assert (gb.tau1[b], gb.tau2_0[b], gb.tau2[b]) == (g1.tau1, g1.tau2_0, g1.tau2), b
        assert np.array_equal(gb.gap[:, b], g1.gap) and gb.status[b] == g1.status, b


def test_a_start_that_runs_out_of_steps(gpu_ctx, tables):
    tau1 = np.array([0.70, 0.75, 0.80])
    tof = 10.0 * day / TU
    first = lto.stack_guess(tau1, tof, tof, 5, tables, ctx=gpu_ctx)
    assert np.array_equal(first.status, [0, 0, 0])
    short = lto.stack_guess(tau1[1], tof, tof, 5, tables, integ=lto.integrator(max_steps=1), ctx=gpu_ctx)   # the call returns
    assert short.status == 2
    assert np.array_equal(short.X[:, 0], first.X[:, 0, 1])           # node 0 is no flow
    assert np.all(np.isnan(short.X[:, 1])) and np.isnan(short.gap[0])
    again = lto.stack_guess(tau1, tof, tof, 5, tables, ctx=gpu_ctx)
    assert np.array_equal(again.X, first.X) and np.array_equal(again.status, first.status)
    assert np.array_equal(again.gap, first.gap)


def test_refusals(gpu_ctx, tables):
    tof = 10.0 * day / TU

    def code(tau1=0.75, tof1=tof, tof2=tof, n=5, orbits=tables, MU_=MU, integ=None):
        with pytest.raises(lto.LtoError) as ei:
            lto.stack_guess(tau1, tof1, tof2, n, orbits, MU=MU_, integ=integ, ctx=gpu_ctx)
        return ei.value.code

    assert code(n=1) == -1
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert code(tof1=bad) == -1
        assert code(tof2=bad) == -1
    for bad in (np.nan, np.inf, 1e6, -1e6):
        assert code(tau1=bad) == -1
    for bad in (0.0, 1.0, -0.1, np.nan):
        assert code(MU_=bad) == -1
    t0, X0, tf, Xf = tables
    assert code(orbits=(t0[:1], X0[:, :1], tf, Xf)) == -1
    assert code(orbits=(t0, X0, tf[:1], Xf[:, :1])) == -1
    assert code(integ=lto.integrator(lto.RKF78_ADAPTIVE)) == -3
    assert code(integ=lto.integrator(lto.RKF78_FIXED, steps=8)) == -3
    assert code(tau1=np.zeros(0), tof1=np.zeros(0), tof2=np.zeros(0)) == -1       # n_batch < 1
    # NULL pointers and the size guard, through the C entry itself
    fn, h = gpu_ctx.fn("stack_guess_batch"), gpu_ctx.handle
    ob = lto.DirectOrbits(*tables)
    integ = lto.integrator()
    import ctypes as C
    a = np.array([0.75]); f = np.array([tof])
    X = np.zeros((6, 5, 1), order="F"); t = np.zeros((5, 1), order="F"); tau = np.zeros((3, 1), order="F")
    st = np.zeros(1, dtype=np.int32)
    p = lambda v: v.ctypes.data_as(C.c_void_p)
    full = [h, 5, 1, MU, C.byref(ob.struct), C.byref(integ), p(a), p(f), p(f), p(X), p(t), p(tau), None, p(st)]
    assert fn(*full) == 0                                             # gap_out may be NULL
    for k in (4, 5, 6, 7, 8, 9, 10, 11, 13):
        args = list(full)
        args[k] = None
        assert fn(*args) == -2, k
    args = list(full)
    args[1], args[2] = 1 << 20, 1 << 10                               # 6 n B > 2^31 - 1: refused before anything is read
    assert fn(*args) == -1


def test_guess_feeds_the_direct_solve(gpu_ctx, tables):
    """The reference demo: the ballistic stacked guess, zero thrust, flagEnd = false, at most 100 iterations."""
    n, tau1, tof1, tof2 = _case("demo")
    X, t, tau1w, tau2 = drivers.stacked_guess(n, tof1, tof2, tau1, *tables, MU, ctx=gpu_ctx)
    assert drivers.stacked_guess.last.status == 0
    out = drivers.multiShoot_CRTBP_direct(X, np.zeros((3, n)), tau1w, tau2, t, np.zeros(3), np.zeros(3), MU, DU, TU, n, 10, 1000.0, 2000.0,
                                          *tables, False, False, 0.0, False, 100, verbose=False)
    last = drivers.multiShoot_CRTBP_direct.last
    print("direct solve from the ballistic stacked guess: status %d after %d iterations, max defect %.2e" % (
        last["status"], last["iterations"], np.abs(out[7]).max()))
    assert last["status"] == 0
    assert np.abs(out[7]).max() <= 1e-6                               # the loop's own stopping bar (direct.jl:491)


def test_multi_start_equals_the_single_starts(gpu_ctx, tables):
    tau1s = np.array([0.70, 0.75, 0.80])
    tof = 10.0 * day / TU
    args = (30, 10, 1000.0, 2000.0) + tuple(tables) + (MU, DU, TU)
    m = drivers.multiStart_direct(tau1s, tof, tof, *args, flagEnd=False, ctx=gpu_ctx)
    print("multi-start: status %s, iterations %s, cost %s, order %s" % (m["status"], m["iterations"], m["cost"], m["order"]))
    for b, tau1 in enumerate(tau1s):
        s = drivers.multiStart_direct(tau1, tof, tof, *args, flagEnd=False, ctx=gpu_ctx)
        for key in ("X", "U", "t", "dV", "defect", "tau", "tau_guess", "gap", "history"):
            assert np.array_equal(m[key][..., b], s[key][..., 0], equal_nan=True), (b, key)
        for key in ("status", "iterations", "guess_status"):
            assert m[key][b] == s[key][0], (b, key)
        assert np.array_equal(m["cost"][b], s["cost"][0], equal_nan=True)
    assert m["status"][1] == 0
    ok = np.flatnonzero(m["status"] == 0)
    assert sorted(m["order"]) == sorted(ok)
    assert np.all(np.diff(m["cost"][m["order"]]) >= 0.0)
