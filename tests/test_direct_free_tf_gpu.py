"""GPU: a free time of flight in the direct method's free-end step -- the device step against the dense host reference built from
the same device Jacobian blocks and tf column, a 4 097-node step against a sparse host solve, the delegation of a pinned tf, and the
free-tf loop (lto_direct_solve_free_tf / _batch) on the halo demo."""

import numpy as np
import pytest

import lowthrustopt_amd as lto
from lowthrustopt_amd import drivers, synth
from oracle import oracle as O

import direct_helpers as DH
import qp_reference as QR

ISP, NSTEPS = 2000.0, 10
DAY = lto.day / lto.TU
DEMO_TAU2_OFFSET = 0.02


def _tf_problems(n, ns, B, seed):
    """B problems with their own grids, phases, beta and tf bounds: wide, tight (p3 at +-step) and absolute bounds around tf."""
    X, U, T = synth.direct_problem(n, n_batch=B, nstate=ns, seed=seed)
    T = T * (1.0 + 0.1 * np.arange(B))[None, :]
    tabs = DH.tables()
    rng = np.random.default_rng(seed)
    betas = np.array([0.0, 1.0, 100.0, 0.5, 10.0])[:B]
    tg, em, tb, host = [], [], [], []
    for b in range(B):
        tau = (0.2 + 0.1 * b, 0.7 - 0.05 * b)
        X[:6, 0, b], X[:6, -1, b] = drivers.interpEndStates(tau[0] + 0.03, tau[1] - 0.02, *tabs)
        dV1, dV2 = 1e-4 * rng.standard_normal(3), 1e-4 * rng.standard_normal(3)
        model = drivers.end_model(tau[0], tau[1], *tabs)
        tf = T[-1, b]
        bounds = [(50.0, T[0, b] + 1e-3, tf + 100.0), (1e-5, T[0, b] + 1e-3, tf + 100.0), (1.0, tf - 1e-6, tf + 1e-6),
                  (DAY, T[0, b] + DAY, 40 * DAY), (1e-4, T[0, b] + 1e-3, tf + 1.0)][b]
        tg.append(lto.direct_targets(model[0], model[1], 1000.0 - b, dV1, dV2))
        em.append(lto.direct_end_model(*model[2:]))
        tb.append(lto.direct_tf_bounds(*bounds))
        host.append((model, 1000.0 - b, dV1, dV2, bounds))
    return np.asfortranarray(X), np.asfortranarray(U), np.asfortranarray(T), tg, em, tb, betas, host


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [6, 7])
@pytest.mark.parametrize("imp", [False, True])
@pytest.mark.parametrize("n", [3, 17, 30])
def test_device_free_tf_step_matches_host(gpu_ctx, ns, imp, n):
    B = 5
    X, U, T, tg, em, tb, betas, host = _tf_problems(n, ns, B, seed=n + ns)
    Jt, dtf, d, _ = lto.direct_jacobian_blocks(X, U, T, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, ctx=gpu_ctx)
    dX, dU, dV, p, cost = lto.direct_qp_step_free_tf(X, U, T, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tg, em, betas, tb, allowImpulsive=imp,
                                                     ctx=gpu_ctx)
    bounds = 0
    for b in range(B):
        model, mass, dV1, dV2, tfb = host[b]
        tf = T[-1, b]
        hx, hu, h1, h2, p1, p2, p3, hc = drivers.direct_qp_dense_free_tf(Jt[..., b], dtf[..., b], d[..., b], X[..., b], U[..., b], T[:, b],
                                                                         *model, betas[b], mass, dV1, dV2, lto.DU, lto.TU, tf, tfb,
                                                                         allowImpulsive=imp)
        assert DH.rel(dX[..., b], hx) <= 1e-9 and DH.rel(dU[..., b], hu) <= 1e-9
        assert np.abs(p[:2, b] - [p1, p2]).max() <= 1e-9 * 0.1
        assert abs(p[2, b] - p3) <= 1e-9 * max(tfb[0], 1e-300) or abs(p[2, b] - p3) <= 1e-9 * abs(p3)
        if imp:
            assert DH.rel(dV[:, b], np.r_[h1, h2]) <= 1e-9
        else:
            assert np.all(dV[:, b] == 0)
        assert abs(cost[b] - hc) <= 1e-9 * abs(hc)
        lo = (-0.1, -0.1, max(-tfb[0], tfb[1] - tf))
        hi = (0.1, 0.1, min(tfb[0], tfb[2] - tf))
        for j, (pd, ph) in enumerate(zip(p[:, b], (p1, p2, p3))):
            if ph == lo[j] or ph == hi[j]:                # an active bound is the bound value on the device as well, bit for bit
                assert pd == ph
                bounds += 1
    assert bounds > 0


def _sparse_fixed_p(Jt, dtf, d, X, U, t, s0, sf, mass, dV1, dV2, imp, p3, DU, TU):
    """The QP at fixed p (targets moved, defect + dtf p3): a frozen step of the sparse, refined host reference (qp_reference)."""
    ref, _ = QR.QpSystem(Jt, t, imp, (DU / TU) ** 2).frozen(d + dtf * p3, X, U, s0, sf, mass, dV1, dV2)
    return ref.dX, ref.dU


@pytest.mark.gpu
def test_device_free_tf_step_large_matches_sparse_solve(gpu_ctx):
    """4 097 nodes: with p fixed at the device's answer the step is a frozen QP; a sparse host solve of it gives dX, dU to 1e-9."""
    X, U, T, tg, em, tb, betas, host = _tf_problems(4097, 7, 4, seed=3)
    X, U, T = X[..., 3].copy(order="F"), U[..., 3].copy(order="F"), T[:, 3].copy()
    (s0, sf, g0, gf, c0, cf), mass, dV1, dV2, _ = host[3]
    tfb = (DAY, T[0] + DAY, T[-1] + 10 * DAY)            # this grid spans ~650 TU: bounds around its own tf
    dX, dU, dV, p, cost = lto.direct_qp_step_free_tf(X, U, T, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tg[3], em[3], 1.0,
                                                     lto.direct_tf_bounds(*tfb),
                                                     allowImpulsive=False, ctx=gpu_ctx)
    Jt, dtf, d, _ = lto.direct_jacobian_blocks(X, U, T, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, ctx=gpu_ctx)
    hx, hu = _sparse_fixed_p(Jt, dtf, d, X, U, T, s0 + g0 * p[0], sf + gf * p[1], mass, dV1, dV2, False, p[2], lto.DU, lto.TU)
    print("4 097 nodes: p = (%.6e, %.6e, %.6e), |dX - sparse| rel %.2e, |dU - sparse| rel %.2e" % (*p, DH.rel(dX, hx), DH.rel(dU, hu)))
    assert np.all(np.abs(p[:2]) <= 0.1) and abs(p[2]) <= tfb[0]
    assert DH.rel(dX, hx) <= 1e-9 and DH.rel(dU, hu) <= 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["step0", "flag_end0"])
def test_pinned_tf_delegates_to_the_free_end_solve(gpu_ctx, case):
    X, U, t, tau1, tau2, *tabs = DH.demo().demo_problem()
    tau = np.array([tau1, tau2 + DEMO_TAU2_OFFSET])
    tg = lto.direct_targets(np.zeros(6), np.zeros(6), 1000.0, np.zeros(3), np.zeros(3))
    flag = case != "flag_end0"
    tb = lto.direct_tf_bounds(0.0 if case == "step0" else DAY, t[0] + DAY, 40 * DAY)
    ref = lto.direct_solve_free(X, U, t, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tabs, tg, tau, 0.0, flagEnd=flag, maxIter=100, ctx=gpu_ctx)
    out = lto.direct_solve_free_tf(X, U, t, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tabs, tg, tau, 0.0, tb, flagEnd=flag, maxIter=100,
                                   ctx=gpu_ctx)
    for j in range(6):
        assert np.array_equal(ref[j], out[j])
    assert ref[6:8] == out[6:8]
    k = ref[7]
    assert np.array_equal(ref[8][:, :k], out[8][:5, :k]) and np.all(out[8][5, :k] == t[-1])


@pytest.mark.gpu
def test_demo_free_tf_converges_and_matches_the_mirror_loop(gpu_ctx):
    """30 nodes, tau2 offset 0.02, beta = 0, step 1 day: library loop against the HipDirectOps mirror loop; report the run."""
    X, U, t, tau1, tau2, *tabs = DH.demo().demo_problem()
    tau_0 = (tau1, tau2 + DEMO_TAU2_OFFSET)
    tfb = drivers.tf_bounds_default(t[0], lto.TU)
    args = (np.zeros(3), np.zeros(3), lto.MU, lto.DU, lto.TU, 30, NSTEPS, 1000.0, ISP, *tabs, False, True, 0.0, False, 100)
    Xl, Ul, t1, t2, tl, dV1, dV2, defect = drivers.multiShoot_CRTBP_direct(X, U, *tau_0, t, *args, verbose=False, tf_step=tfb[0])
    lib = dict(drivers.multiShoot_CRTBP_direct.last)
    drivers.multiShoot_CRTBP_direct(X, U, *tau_0, t, *args, verbose=False)
    pinned = dict(drivers.multiShoot_CRTBP_direct.last)
    ops = drivers.HipDirectOps(lto.MU, lto.DU, lto.TU, ISP, gpu_ctx)
    out, py = drivers.direct_loop_host(X, U, *tau_0, t, np.zeros(3), np.zeros(3), lto.MU, lto.DU, lto.TU, 30, NSTEPS, 1000.0, ISP, *tabs,
                                       True, 0.0, False, 100, ops, verbose=False, tf_bounds=tfb)
    k, H = lib["iterations"], lib["history"]
    kp, Hp = pinned["iterations"], pinned["history"]
    print("free-tf demo: status %d, %d iterations, tau = (%.9f, %.9f), tf %.6f -> %.6f days, cost %.6e; pinned tf: status %d, %d "
          "iterations, cost %.6e\nhistory (max|defect|, cost, alpha, tau1, tau2, tf [days]):\n%s" % (
              lib["status"], k, t1, t2, t[-1] / DAY, H[5, k - 1] / DAY, H[1, k - 1], pinned["status"], kp, Hp[1, kp - 1],
              np.array2string(np.vstack([H[:5, :k], H[5:, :k] / DAY]), precision=6, max_line_width=200)))
    assert py["status"] == lib["status"] and py["iterations"] == k
    assert abs(t1 - out[2]) <= 1e-9 * abs(out[2]) and abs(t2 - out[3]) <= 1e-9 * abs(out[3])
    assert abs(H[5, k - 1] - py["history"][5, k - 1]) <= 1e-9 * abs(py["history"][5, k - 1])
    prev = t[-1]                                          # tf moves on odd iterations only, by at most alpha step, within bounds
    for it in range(k):
        if it % 2 == 1:
            assert H[5, it] == prev
        assert abs(H[5, it] - prev) <= H[2, it] * tfb[0] * (1 + 1e-12)
        assert tfb[1] <= H[5, it] <= tfb[2]
        prev = H[5, it]
    tau_grid = (t - t[0]) / (t[-1] - t[0]) * 2 - 1
    assert np.array_equal(tl, t[0] + (tau_grid + 1) / 2 * (H[5, k - 1] - t[0]))
    if lib["status"] == 0:
        d_o, _ = O.direct_defect(Xl, Ul, tl, NSTEPS, lto.MU, lto.DU, lto.TU, ISP)
        assert np.abs(d_o).max() <= 1e-6


@pytest.mark.gpu
def test_multistart_over_tf_equals_single_solves(gpu_ctx):
    X, U, t, tau1, tau2, *tabs = DH.demo().demo_problem()
    tofs = (18.0, 20.0, 22.0)
    B = len(tofs)
    T = np.asfortranarray(np.stack([t[0] + (t - t[0]) * (tof * DAY) / (t[-1] - t[0]) for tof in tofs], axis=1))
    tg = lto.direct_targets(np.zeros(6), np.zeros(6), 1000.0, np.zeros(3), np.zeros(3))
    tb = lto.direct_tf_bounds(DAY, t[0] + DAY, 40 * DAY)
    Xb = np.asfortranarray(np.repeat(X[:, :, None], B, axis=2))
    Ub = np.zeros((3, 30, B), order="F")
    ob = lto.DirectOrbits(*tabs)
    tau = np.array([tau1, tau2 + DEMO_TAU2_OFFSET])
    out_b = lto.direct_solve_free_tf(Xb, Ub, T, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, ob, tg, tau, 0.0, tb, maxIter=60, ctx=gpu_ctx)
    for k in range(B):
        out_s = lto.direct_solve_free_tf(X, np.zeros((3, 30)), T[:, k], NSTEPS, lto.MU, lto.DU, lto.TU, ISP, ob, tg, tau, 0.0, tb,
                                         maxIter=60, ctx=gpu_ctx)
        print("tf start %.0f days: status %d, %d iterations, final tf %.6f days" % (tofs[k], out_s[6], out_s[7], out_s[3][-1] / DAY))
        assert out_s[6] == out_b[6][k] and out_s[7] == out_b[7][k]
        for j in (0, 1, 3, 4, 5):
            assert np.abs(out_s[j] - out_b[j][..., k]).max() <= 1e-12 * max(1.0, np.abs(out_s[j]).max())
