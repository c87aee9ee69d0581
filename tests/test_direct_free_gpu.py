"""GPU: free end points of the direct method (flagEnd = true) -- the device end model, the free-end QP step against the host
reference built from the same device Jacobian blocks, and the free-end loop (lto_direct_solve_free / _batch) on the halo demo."""

import numpy as np
import pytest

import lowthrustopt_amd as lto
from lowthrustopt_amd import drivers, synth

import direct_helpers as DH

ISP, NSTEPS = 2000.0, 10
DEMO_TAU2_OFFSET = 0.02


@pytest.mark.gpu
def test_device_end_states_match_host(gpu_ctx):
    tabs = DH.tables()
    taus = np.array([[0.3, 0.6], [0.02, 0.99], [0.999, 0.001], [1.03, -0.04], [0.0, 1.0], [0.75, 0.5]]).T
    s0, sf, g0, gf, c0, cf = lto.direct_end_states(np.asfortranarray(taus), tabs, ctx=gpu_ctx)
    for b in range(taus.shape[1]):
        h = drivers.end_model(taus[0, b], taus[1, b], *tabs)
        for dev, host in ((s0[:, b], h[0]), (sf[:, b], h[1]), (g0[:, b], h[2]), (gf[:, b], h[3])):
            assert np.abs(dev - host).max() <= 1e-12
        assert abs(c0[b] - h[4]) <= 1e-12 and abs(cf[b] - h[5]) <= 1e-12


def _free_problems(n, ns, B, seed):
    """B problems with their own grids, phases and beta; the end nodes sit on the orbits a little away from the phases."""
    X, U, T = synth.direct_problem(n, n_batch=B, nstate=ns, seed=seed)
    T = T * (1.0 + 0.1 * np.arange(B))[None, :]
    tabs = DH.tables()
    rng = np.random.default_rng(seed)
    betas = np.array([0.0, 1.0, 100.0, 0.5, 10.0])[:B]
    tg, em, host = [], [], []
    for b in range(B):
        tau = (0.2 + 0.1 * b, 0.7 - 0.05 * b)
        X[:6, 0, b], X[:6, -1, b] = drivers.interpEndStates(tau[0] + 0.03, tau[1] - 0.02, *tabs)
        dV1, dV2 = 1e-4 * rng.standard_normal(3), 1e-4 * rng.standard_normal(3)
        model = drivers.end_model(tau[0], tau[1], *tabs)
        tg.append(lto.direct_targets(model[0], model[1], 1000.0 - b, dV1, dV2))
        em.append(lto.direct_end_model(*model[2:]))
        host.append((model, 1000.0 - b, dV1, dV2))
    return np.asfortranarray(X), np.asfortranarray(U), np.asfortranarray(T), tg, em, betas, host


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [6, 7])
@pytest.mark.parametrize("imp", [False, True])
@pytest.mark.parametrize("n", [3, 17, 30])
def test_device_free_step_matches_host(gpu_ctx, ns, imp, n):
    B = 5
    X, U, T, tg, em, betas, host = _free_problems(n, ns, B, seed=n + ns)
    Jt, _, d, _ = lto.direct_jacobian_blocks(X, U, T, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, ctx=gpu_ctx)
    dX, dU, dV, p, cost = lto.direct_qp_step_free(X, U, T, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tg, em, betas, allowImpulsive=imp,
                                                  ctx=gpu_ctx)
    bounds = 0
    for b in range(B):
        model, mass, dV1, dV2 = host[b]
        hx, hu, h1, h2, p1, p2, hc = drivers.direct_qp_dense_free(Jt[..., b], d[..., b], X[..., b], U[..., b], T[:, b], *model, betas[b],
                                                                  mass, dV1, dV2, lto.DU, lto.TU, allowImpulsive=imp)
        assert DH.rel(dX[..., b], hx) <= 1e-9 and DH.rel(dU[..., b], hu) <= 1e-9
        assert np.abs(p[:, b] - [p1, p2]).max() <= 1e-9 * 0.1
        if imp:
            assert DH.rel(dV[:, b], np.r_[h1, h2]) <= 1e-9
        else:
            assert np.all(dV[:, b] == 0)
        assert abs(cost[b] - hc) <= 1e-9 * abs(hc)
        for pd, ph in zip(p[:, b], (p1, p2)):
            if abs(ph) == 0.1:                            # an active bound is exactly +-0.1 on the device as well
                assert pd == ph
                bounds += 1
    if not imp:
        assert bounds > 0


@pytest.mark.gpu
def test_device_free_step_large(gpu_ctx):
    """4 097 nodes: the free step's update is the frozen step's at the moved targets s0 + g0 p1, sf + gf p2."""
    X, U, T, tg, em, betas, host = _free_problems(4097, 7, 1, seed=3)
    X, U, T = X[..., 0], U[..., 0], T[:, 0]
    dX, dU, dV, p, cost = lto.direct_qp_step_free(X, U, T, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tg[0], em[0], 1.0, allowImpulsive=True,
                                                  ctx=gpu_ctx)
    (s0, sf, g0, gf, c0, cf), mass, dV1, dV2 = host[0]
    tgp = lto.direct_targets(s0 + g0 * p[0], sf + gf * p[1], mass, dV1, dV2)
    fx, fu, fv, fc = lto.direct_qp_step(X, U, T, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tgp, allowImpulsive=True, ctx=gpu_ctx)
    assert np.all(np.abs(p) <= 0.1)
    assert DH.rel(dX, fx) <= 1e-9 and DH.rel(dU, fu) <= 1e-9 and DH.rel(dV, fv) <= 1e-9
    assert abs(cost - (fc + 1.0 * (c0 / 2 * p[0] ** 2 + cf / 2 * p[1] ** 2))) <= 1e-9 * abs(cost)


@pytest.mark.gpu
def test_flag_end_off_is_the_frozen_solve(gpu_ctx):
    X, U, t, tau1, tau2, *tabs = DH.demo().demo_problem()
    tau = np.array([tau1, tau2 + DEMO_TAU2_OFFSET])
    s0, sf, *_ = lto.direct_end_states(tau, tabs, ctx=gpu_ctx)
    tg = lto.direct_targets(s0, sf, 1000.0, np.zeros(3), np.zeros(3))
    ref = lto.direct_solve(X, U, t, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tg, maxIter=100, ctx=gpu_ctx)
    out = lto.direct_solve_free(X, U, t, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tabs, tg, tau, 0.0, flagEnd=False, maxIter=100, ctx=gpu_ctx)
    for j_ref, j_out in ((0, 0), (1, 1), (2, 2), (3, 3), (4, 4)):
        assert np.array_equal(ref[j_ref], out[j_out])
    assert ref[5:7] == out[6:8] and np.array_equal(out[5], tau)
    k = ref[6]
    assert np.array_equal(ref[7][:, :k], out[8][:3, :k])


@pytest.mark.gpu
def test_demo_free_ends_converges_and_matches_the_mirror_loop(gpu_ctx):
    X, U, t, tau1, tau2, *tabs = DH.demo().demo_problem()
    tau_0 = (tau1, tau2 + DEMO_TAU2_OFFSET)
    args = (t, np.zeros(3), np.zeros(3), lto.MU, lto.DU, lto.TU, 30, NSTEPS, 1000.0, ISP, *tabs, False, True, 0.0, False, 100)
    Xl, Ul, t1, t2, tl, dV1, dV2, defect = drivers.multiShoot_CRTBP_direct(X, U, *tau_0, *args, verbose=False)
    lib = dict(drivers.multiShoot_CRTBP_direct.last)
    ops = drivers.HipDirectOps(lto.MU, lto.DU, lto.TU, ISP, gpu_ctx)
    out, py = drivers.direct_loop_host(X, U, *tau_0, t, np.zeros(3), np.zeros(3), lto.MU, lto.DU, lto.TU, 30, NSTEPS, 1000.0, ISP, *tabs,
                                       True, 0.0, False, 100, ops, verbose=False)
    k = lib["iterations"]
    H = lib["history"]
    print("free-end demo: %d iterations, tau = (%.9f, %.9f), cost %.6f; history\n%s" % (k, t1, t2, H[1, k - 1],
                                                                                        np.array2string(H[:, :k], precision=6)))
    assert lib["status"] == 0 and np.abs(defect).max() <= 1e-6
    assert py["status"] == 0 and py["iterations"] == k
    assert abs(t1 - out[2]) <= 1e-9 and abs(t2 - out[3]) <= 1e-9
    assert np.abs(Xl - out[0]).max() <= 1e-8
    prev = np.array(tau_0)
    for it in range(k):
        step = H[3:5, it] - prev
        if it % 2 == 1:                                   # even iterations (1-based): frozen, p = 0 exactly
            assert np.all(step == 0)
        else:
            p = step / H[2, it]
            assert np.all(np.abs(p) <= 0.1 * (1 + 1e-12))
        prev = H[3:5, it]
    assert np.array_equal(prev, [t1, t2])
    assert np.abs(H[3:5, :k] - py["history"][3:5, :k]).max() <= 1e-9


@pytest.mark.gpu
def test_multistart_batch_equals_single_solves(gpu_ctx):
    X, U, t, tau1, tau2, *tabs = DH.demo().demo_problem()
    B = 4
    taus = np.array([[tau1, tau2 + o] for o in (0.0, 0.01, 0.02, -0.01)]).T
    tg = lto.direct_targets(np.zeros(6), np.zeros(6), 1000.0, np.zeros(3), np.zeros(3))
    Xb = np.asfortranarray(np.repeat(X[:, :, None], B, axis=2))
    Ub = np.zeros((3, 30, B), order="F")
    ob = lto.DirectOrbits(*tabs)
    out_b = lto.direct_solve_free(Xb, Ub, t, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, ob, tg, np.asfortranarray(taus), 0.0, maxIter=100,
                                  ctx=gpu_ctx)
    for k in range(B):
        out_s = lto.direct_solve_free(X, np.zeros((3, 30)), t, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, ob, tg, taus[:, k], 0.0, maxIter=100,
                                      ctx=gpu_ctx)
        assert out_s[6] == out_b[6][k] and out_s[7] == out_b[7][k]
        for j in (0, 1, 4, 5):
            assert np.abs(out_s[j] - out_b[j][..., k]).max() <= 1e-12 * max(1.0, np.abs(out_s[j]).max())
