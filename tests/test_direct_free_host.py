"""CPU: free end points of the direct method (flagEnd = true) -- the host reference step direct_qp_dense_free against the
optimality conditions, the host end model, the mirror loop with free ends on the CPU oracle, and the new C entry points'
argument checks."""
import ctypes as C

import numpy as np
import pytest

import lowthrustopt_amd as lto
from lowthrustopt_amd import _lib, drivers, synth
from oracle import oracle as O

import direct_helpers as DH

C2 = (lto.DU / lto.TU) ** 2
ISP = 2000.0


def _free_problem(n, ns, seed, tau, shift):
    """A synthetic problem whose end nodes sit on the orbits at tau + shift: the free step wants to move the phases by ~shift."""
    X, U, T = synth.direct_problem(n, nstate=ns, seed=seed)
    X, U, t = X[:, :, 0].copy(), U[:, :, 0].copy(), T[:, 0]
    tabs = DH.tables()
    a0, af = drivers.interpEndStates(tau[0] + shift[0], tau[1] + shift[1], *tabs)
    X[:6, 0], X[:6, -1] = a0, af
    rng = np.random.default_rng(seed)
    dV1, dV2 = 1e-4 * rng.standard_normal(3), 1e-4 * rng.standard_normal(3)
    Jt, _, d = O.direct_jacobian_dual(X, U, t, 10, lto.MU, lto.DU, lto.TU, ISP)
    model = drivers.end_model(tau[0], tau[1], *tabs)
    return Jt, d, X, U, t, model, 1000.0, dV1, dV2


def _kkt_check(Jt, d, X, U, t, model, mass, dV1, dV2, beta, imp, sol):
    """Independent optimality check of a free step: feasibility, stationarity with least-squares multipliers, bound signs."""
    s0, sf, g0, gf, c0, cf = model
    dx, du, d1, d2, p1, p2, cost = sol
    ns, _, S = Jt.shape
    n = S + 1
    w = np.zeros(n)
    w[:-1] += np.diff(t) / 2
    w[1:] += np.diff(t) / 2
    nz = ns * n + 3 * n + 8
    iu, iv, ip = ns * n, ns * n + 3 * n, ns * n + 3 * n + 6
    z = np.r_[dx.T.reshape(-1), du.T.reshape(-1), d1, d2, p1, p2]
    grad = np.zeros(nz)
    grad[iu:iv] = 2 * np.repeat(w, 3) * (U + du).T.reshape(-1)
    grad[iv:ip] = 2 * C2 * np.r_[dV1 + d1, dV2 + d2]
    grad[ip], grad[ip + 1] = beta * c0 * p1, beta * cf * p2
    A, b = [], []
    for i in range(S):
        r = np.zeros((ns, nz))
        r[:, ns * i:ns * (i + 2)] = Jt[:, :2 * ns, i]
        r[:, iu + 3 * i:iu + 3 * i + 6] = Jt[:, 2 * ns:, i]
        A.append(r)
        b.append(-d[:, i])
    for k, s, g, dv, o in ((0, s0, g0, dV1, 0), (n - 1, sf, gf, dV2, 1)):
        r = np.zeros((6, nz))
        r[:, ns * k:ns * k + 6] = np.eye(6)
        r[3:, iv + 3 * o:iv + 3 * o + 3] = np.eye(3)
        r[:, ip + o] = -g
        A.append(r)
        b.append(s - X[:6, k] - np.r_[0, 0, 0, dv])
    if ns == 7:
        r = np.zeros((1, nz))
        r[0, 6] = 1
        A.append(r)
        b.append([mass - X[6, 0]])
    if not imp:
        r = np.zeros((6, nz))
        r[:, iv:ip] = np.eye(6)
        A.append(r)
        b.append(np.zeros(6))
    act = [(j, np.sign(p)) for j, p in enumerate((p1, p2)) if abs(p) == 0.1]
    for j, _ in act:
        r = np.zeros((1, nz))
        r[0, ip + j] = 1
        A.append(r)
        b.append([0.0])
    A = np.vstack(A)
    b = np.concatenate([np.atleast_1d(v) for v in b])
    ne = A.shape[0] - len(act)
    res = A[:ne] @ z - b[:ne]
    assert np.abs(res).max() <= 1e-10 * max(1.0, np.abs(b).max())                  # feasibility
    assert abs(p1) <= 0.1 and abs(p2) <= 0.1
    # stationarity: grad + A' lam = 0 in the equilibrated variables
    D = 1.0 / np.maximum(np.abs(A).max(axis=0), 1e-300)
    lam, *_ = np.linalg.lstsq((A * D[None, :]).T, -grad * D, rcond=None)
    r = (A * D[None, :]).T @ lam + grad * D
    assert np.abs(r).max() <= 1e-8 * max(1.0, np.abs(grad * D).max())
    for (j, sgn), mu in zip(act, lam[ne:]):                                          # p at +0.1: mu >= 0, at -0.1: mu <= 0
        assert sgn * mu >= -1e-8 * max(1.0, np.abs(lam).max())
    cost_ref = np.sum(w * np.sum((U + du) ** 2, axis=0)) + C2 * (np.sum((dV1 + d1) ** 2) + np.sum((dV2 + d2) ** 2)) + \
        beta * (c0 / 2 * p1 ** 2 + cf / 2 * p2 ** 2)
    assert abs(cost - cost_ref) <= 1e-10 * abs(cost_ref)
    return len(act)


CASES = [((0.3, 0.6), (0.02, -0.03)), ((0.3, 0.6), (0.4, 0.01)), ((0.2, 0.7), (-0.4, 0.4))]


@pytest.mark.parametrize("ns", [6, 7])
@pytest.mark.parametrize("imp", [False, True])
def test_dense_free_step_satisfies_kkt(ns, imp):
    """beta = 0, 1, 100 on three problems and on one whose arrival model is flat (gf = 0: p2 only pays beta): the optimum is
    interior (beta = 100), has one bound active (flat arrival) or both (beta = 0)."""
    actives = set()
    for k, (tau, shift) in enumerate(CASES + [((0.3, 0.6), (0.0, 0.0))]):
        Jt, d, X, U, t, model, mass, dV1, dV2 = _free_problem(6, ns, 11 + k, tau, shift)
        if k == len(CASES):
            model = model[:3] + (np.zeros(6),) + model[4:]
        for beta in (0.0, 1.0, 100.0):
            sol = drivers.direct_qp_dense_free(Jt, d, X, U, t, *model, beta, mass, dV1, dV2, lto.DU, lto.TU, allowImpulsive=imp)
            actives.add(_kkt_check(Jt, d, X, U, t, model, mass, dV1, dV2, beta, imp, sol))
            if not imp:
                assert np.all(sol[2] == 0) and np.all(sol[3] == 0)
    assert {0, 1} <= actives and (imp or 2 in actives)   # with impulses the end points are cheap to reach: no case at two bounds


@pytest.mark.parametrize("ns,imp", [(6, False), (7, True)])
def test_dense_free_step_with_flat_ends_is_the_frozen_step(ns, imp):
    Jt, d, X, U, t, model, mass, dV1, dV2 = _free_problem(7, ns, 3, (0.3, 0.6), (0.01, 0.01))
    s0, sf = model[0], model[1]
    x, u, v1, v2, p1, p2, cost = drivers.direct_qp_dense_free(Jt, d, X, U, t, s0, sf, np.zeros(6), np.zeros(6), 1.0, 2.0, 1.0, mass,
                                                              dV1, dV2, lto.DU, lto.TU, allowImpulsive=imp)
    hx, hu, h1, h2, hc = drivers.direct_qp_dense(Jt, d, X, U, t, s0, sf, mass, dV1, dV2, lto.DU, lto.TU, allowImpulsive=imp)
    assert p1 == 0 and p2 == 0
    for a, b in ((x, hx), (u, hu), (v1, h1), (v2, h2)):
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())
    assert abs(cost - hc) <= 1e-12 * abs(hc)


@pytest.mark.parametrize("tau1,tau2", [(0.3, 0.6), (0.02, 0.99), (0.999, 0.001), (1.03, -0.04)])
def test_host_end_model_is_the_finite_differences(tau1, tau2):
    tabs = DH.tables()
    s0, sf, g0, gf, c0, cf = drivers.end_model(tau1, tau2, *tabs)
    h = 0.05

    def s(tau, k):                                        # interpEndStates of one end, wrapped on its own
        return drivers.interpEndStates(tau, tau, *tabs)[k]
    assert np.array_equal(s0, s(tau1, 0)) and np.array_equal(sf, s(tau2, 1))
    np.testing.assert_allclose(g0, (s(tau1 + h, 0) - s(tau1 - h, 0)) / (2 * h), rtol=0, atol=1e-13)
    np.testing.assert_allclose(gf, (s(tau2 + h, 1) - s(tau2 - h, 1)) / (2 * h), rtol=0, atol=1e-13)
    assert abs(c0 - np.linalg.norm((s(tau1 + h, 0) - 2 * s(tau1, 0) + s(tau1 - h, 0)) / h ** 2)) <= 1e-12 * max(1.0, c0)
    assert abs(cf - np.linalg.norm((s(tau2 + h, 1) - 2 * s(tau2, 1) + s(tau2 - h, 1)) / h ** 2)) <= 1e-12 * max(1.0, cf)


def _loop(X, U, tau1, tau2, t, tabs, beta, maxIter, ops, n):
    return drivers.direct_loop_host(X, U, tau1, tau2, t, np.zeros(3), np.zeros(3), lto.MU, lto.DU, lto.TU, n, 10, 1000.0, ISP, *tabs,
                                    True, beta, False, maxIter, ops, verbose=False)


def _check_history(hist, iters, tau0):
    tau_prev = np.array(tau0, dtype=float)
    for k in range(iters):
        tau_k = hist[3:5, k]
        step = tau_k - tau_prev
        if k % 2 == 1:                                    # even iterations (1-based) are frozen
            assert np.all(step == 0)
        assert np.all(np.abs(step) <= 0.1 * hist[2, k] * (1 + 1e-12))
        tau_prev = tau_k


def test_mirror_loop_with_free_ends_converges_on_oracle():
    n = 8
    X, U, T = synth.direct_problem(n, seed=5)
    X, U, t = X[:, :, 0].copy(), U[:, :, 0].copy(), T[:, 0]
    tabs = DH.tables()
    s0, sf = drivers.interpEndStates(0.32, 0.58, *tabs)
    X[:6, 0], X[:6, -1] = s0, sf                          # end nodes on the orbits, away from the starting phases 0.3, 0.6
    out, last = _loop(X, U, 0.3, 0.6, t, tabs, 0.0, 30, DH.OracleDirectOps(ISP), n)
    Xo, Uo, tau1, tau2, to, dV1, dV2, defect = out
    assert last["status"] == 0 and np.abs(defect).max() <= 1e-6
    assert (tau1, tau2) != (0.3, 0.6)
    _check_history(last["history"], last["iterations"], (0.3, 0.6))
    s0n, sfn = drivers.interpEndStates(tau1, tau2, *tabs)
    # the last iteration lands on the linear end model; at convergence it is within the model's error of the orbit
    assert np.abs(Xo[:6, 0] - s0n).max() < 1e-3 and np.abs(Xo[:6, -1] - sfn).max() < 1e-3


DEMO_TAU2_OFFSET = 0.02


def test_mirror_loop_free_ends_halo_demo_preview():
    """CPU preview of the GPU demo case: the 30-node halo demo, flagEnd = true, beta = 0, tau2 offset from its stacked value."""
    X, U, t, tau1, tau2, *tabs = DH.demo().demo_problem()
    out, last = _loop(X, U, tau1, tau2 + DEMO_TAU2_OFFSET, t, tabs, 0.0, 100, DH.OracleDirectOps(ISP), 30)
    defect = out[7]
    print("free-end demo preview (oracle): status %d, %d iterations, tau = (%.9f, %.9f), cost %.6f" % (
        last["status"], last["iterations"], out[2], out[3], last["history"][1, last["iterations"] - 1]))
    assert last["status"] == 0 and np.abs(defect).max() <= 1e-6
    _check_history(last["history"], last["iterations"], (tau1, tau2 + DEMO_TAU2_OFFSET))


def test_free_entry_points_without_a_device():
    lib = lto.load_library()
    for name in ("lto_direct_end_states", "lto_direct_qp_step_free", "lto_direct_solve_free_batch", "lto_direct_solve_free"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert C.sizeof(_lib.LtoDirectEndModel) == 14 * 8
    assert C.sizeof(_lib.LtoDirectOrbits) == 2 * 4 + 4 * 8
    assert C.sizeof(_lib.LtoDirectTargets) == 19 * 8
    x = np.zeros(64)
    p = x.ctypes.data_as(C.c_void_p)
    prm = _lib.LtoDirectParams(lto.MU, lto.DU, lto.TU, ISP)
    tg = lto.direct_targets(np.zeros(6), np.zeros(6), 1000.0, np.zeros(3), np.zeros(3))
    em = lto.direct_end_model(np.zeros(6), np.zeros(6), 0.0, 0.0)
    ob = lto.DirectOrbits(*DH.tables())
    st = (C.c_int * 1)()
    assert lib.lto_direct_end_states(None, C.byref(ob.struct), 1, p, p, C.byref(em)) == _lib.LTO_ENULL
    assert lib.lto_direct_end_states(None, C.byref(ob.struct), 0, p, p, C.byref(em)) == _lib.LTO_EINVAL
    assert lib.lto_direct_qp_step_free(None, 6, 4, 1, p, p, p, 1, 10, C.byref(prm), C.byref(tg), C.byref(em), p, 1, 0, p, p, p, p,
                                       p) == _lib.LTO_ENULL
    assert lib.lto_direct_solve_free(None, 6, 4, p, p, p, 10, C.byref(prm), C.byref(ob.struct), C.byref(tg), p, 0.0, 1, 0, 10, p, p, p,
                                     p, p, p, st, None, None) == _lib.LTO_ENULL
    for ns, n in ((5, 4), (8, 4), (6, 1), (7, 0)):
        assert lib.lto_direct_qp_step_free(None, ns, n, 1, p, p, p, 1, 10, C.byref(prm), C.byref(tg), C.byref(em), p, 1, 0, p, p, p,
                                           p, p) == _lib.LTO_EINVAL
        assert lib.lto_direct_solve_free_batch(None, ns, n, 1, p, p, p, 1, 10, C.byref(prm), C.byref(ob.struct), C.byref(tg), 1, p, p,
                                               1, 0, 10, p, p, p, p, p, p, st, None, None) == _lib.LTO_EINVAL
    with pytest.raises(ValueError):
        lto.DirectOrbits(np.linspace(0, 1, 5), np.zeros((6, 4)), np.linspace(0, 1, 5), np.zeros((6, 5)))
