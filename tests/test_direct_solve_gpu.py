"""GPU: the direct method's QP step (lto_direct_qp_step, kernels_direct_qp.hip) against the host KKT solve built from the same
device Jacobian blocks, and the device loop of multiShoot_CRTBP_direct (lto_direct_solve / _batch) on the reference demo."""

import numpy as np
import pytest

import lowthrustopt_amd as lto
from lowthrustopt_amd import drivers, synth

import direct_helpers as DH
import qp_reference as QR

ISP, NSTEPS = 2000.0, 10


def _problems(n, ns, B, seed):
    """B different problems: own time grids (segment lengths scaled by 1 + 0.1 b) and own targets."""
    X, U, T = synth.direct_problem(n, n_batch=B, nstate=ns, seed=seed)
    T = T * (1.0 + 0.1 * np.arange(B))[None, :]
    rng = np.random.default_rng(seed)
    tg, tg_np = [], []
    for b in range(B):
        s0 = X[:6, 0, b] + 1e-4 * rng.standard_normal(6)
        sf = X[:6, -1, b] + 1e-4 * rng.standard_normal(6)
        dV1, dV2 = 1e-4 * rng.standard_normal(3), 1e-4 * rng.standard_normal(3)
        tg.append(lto.direct_targets(s0, sf, 1000.0 - b, dV1, dV2))
        tg_np.append((s0, sf, 1000.0 - b, dV1, dV2))
    return np.asfortranarray(X), np.asfortranarray(U), np.asfortranarray(T), tg, tg_np


def _host_qp_sparse(Jt, d, X, U, t, s0, sf, mass, dV1, dV2, imp):
    """The same KKT system as drivers.direct_qp_dense, sparse and refined (qp_reference), for the one large case."""
    ref, _ = QR.QpSystem(Jt, t, imp, (lto.DU / lto.TU) ** 2).frozen(d, X, U, s0, sf, mass, dV1, dV2)
    return ref.dX, ref.dU, ref.dV


def _check_step(Jt, d, X, U, t, tgt, imp, dX, dU, dV, cost, dense=True):
    s0, sf, mass, dV1, dV2 = tgt
    if dense:
        hx, hu, h1, h2, hc = drivers.direct_qp_dense(Jt, d, X, U, t, s0, sf, mass, dV1, dV2, lto.DU, lto.TU, allowImpulsive=imp)
        hv = np.r_[h1, h2]
        assert abs(cost - hc) <= 1e-9 * abs(hc)
    else:
        hx, hu, hv = _host_qp_sparse(Jt, d, X, U, t, s0, sf, mass, dV1, dV2, imp)
    assert DH.rel(dX, hx) <= 1e-9 and DH.rel(dU, hu) <= 1e-9
    if imp:
        assert DH.rel(dV, hv) <= 1e-9
    else:
        assert np.all(dV == 0)
    ns = X.shape[0]
    # the step satisfies the linearised defects and the end-point pins
    lin = np.einsum("rci,ci->ri", Jt[:, :ns], dX[:, :-1]) + np.einsum("rci,ci->ri", Jt[:, ns:2 * ns], dX[:, 1:]) + \
        np.einsum("rci,ci->ri", Jt[:, 2 * ns:2 * ns + 3], dU[:, :-1]) + np.einsum("rci,ci->ri", Jt[:, 2 * ns + 3:], dU[:, 1:]) + d
    scale = np.abs(d).max() + np.abs(Jt).max() * (np.abs(dX).max() + np.abs(dU).max())
    assert np.abs(lin).max() <= 1e-12 * scale
    e0 = X[:6, 0] + dX[:6, 0] + np.r_[0, 0, 0, dV1 + dV[:3]] - s0
    ef = X[:6, -1] + dX[:6, -1] + np.r_[0, 0, 0, dV2 + dV[3:]] - sf
    assert max(np.abs(e0).max(), np.abs(ef).max()) <= 1e-12 * max(1.0, np.abs(X[:6]).max())
    if ns == 7:
        assert abs(X[6, 0] + dX[6, 0] - mass) <= 1e-12 * mass


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [6, 7])
@pytest.mark.parametrize("imp", [False, True])
@pytest.mark.parametrize("n,B", [(3, 1), (17, 5), (30, 1), (257, 1), (257, 5)])
def test_device_qp_step_matches_host_kkt(gpu_ctx, ns, imp, n, B):
    X, U, T, tg, tg_np = _problems(n, ns, B, seed=n + ns)
    Jt, _, d, _ = lto.direct_jacobian_blocks(X, U, T, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, ctx=gpu_ctx)
    dX, dU, dV, cost = lto.direct_qp_step(X, U, T, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tg, allowImpulsive=imp, ctx=gpu_ctx)
    for b in range(B):
        _check_step(Jt[..., b], d[..., b], X[..., b], U[..., b], T[:, b], tg_np[b], imp, dX[..., b], dU[..., b], dV[:, b], cost[b])


@pytest.mark.gpu
def test_device_qp_step_large(gpu_ctx):
    """The one large case: 4 097 nodes (a power of two + 1: every level of the reduction carries a row)."""
    X, U, T, tg, tg_np = _problems(4097, 7, 1, seed=3)
    Jt, _, d, _ = lto.direct_jacobian_blocks(X[..., 0], U[..., 0], T[:, 0], NSTEPS, lto.MU, lto.DU, lto.TU, ISP, ctx=gpu_ctx)
    dX, dU, dV, cost = lto.direct_qp_step(X[..., 0], U[..., 0], T[:, 0], NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tg[0], allowImpulsive=True,
                                          ctx=gpu_ctx)
    _check_step(Jt, d, X[..., 0], U[..., 0], T[:, 0], tg_np[0], True, dX, dU, dV, cost, dense=False)


@pytest.mark.gpu
def test_singular_kkt_is_reported(gpu_ctx):
    """Controls without effect on the defect (G = H = 0) leave the pinned end states unreachable: the KKT system of the QP is
    singular, and the device step reports it (plan status 1, NaN outputs) instead of returning NaN silently."""
    import torch
    ns, n = 6, 2
    nvar = 2 * (ns + 3)
    dev = torch.device("cuda", 0)
    Jb = np.zeros((ns, nvar))
    Jb[:, :ns], Jb[:, ns:2 * ns] = np.eye(ns), -np.eye(ns)
    Jac = torch.tensor(Jb.T.reshape(-1, 1), dtype=torch.float64, device=dev).contiguous()       # [(col*ns+row)][1]
    defect = torch.full((ns, 1), 1e-3, dtype=torch.float64, device=dev)
    X = torch.zeros((ns, n), dtype=torch.float64, device=dev)
    U = torch.zeros((3, n), dtype=torch.float64, device=dev)
    t = torch.tensor([0.0, 0.1], dtype=torch.float64, device=dev)
    tg = lto.direct_targets(np.zeros(6), np.full(6, 0.1), 1000.0, np.zeros(3), np.zeros(3))
    tgd = torch.tensor(np.frombuffer(bytes(tg), dtype=np.float64).copy(), device=dev)
    dX, dU = torch.zeros_like(X), torch.zeros_like(U)
    dV, cost = torch.zeros(6, dtype=torch.float64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    plan = lto.DirectPlan(gpu_ctx, ns, n, 1, NSTEPS, lto.MU, lto.DU, lto.TU, ISP)
    plan.qp_step(Jac, 1, defect, 1, X, n, U, n, t, 1, tgd, dX, dU, dV, cost, stream=None)
    torch.cuda.synchronize()
    assert plan.qp_status_ptr()                       # the plan's status array exists after a step
    # finite inputs: the kernels write NaN only for a trajectory whose system they found singular
    assert torch.isnan(cost).all() and torch.isnan(dX).all() and torch.isnan(dU).all()
    plan.close()


@pytest.mark.gpu
def test_reference_direct_demo_converges(gpu_ctx):
    demo = DH.demo()
    X, U, t, tau1, tau2, a, b, c, d = demo.demo_problem()
    args = (tau1, tau2, t, np.zeros(3), np.zeros(3), lto.MU, lto.DU, lto.TU, 30, NSTEPS, 1000.0, ISP, a, b, c, d, False, False, 0.0,
            False, 100)
    Xl, Ul, *_, defect_l = drivers.multiShoot_CRTBP_direct(X, U, *args, verbose=False)
    lib = dict(drivers.multiShoot_CRTBP_direct.last)
    Xp, Up, *_, defect_p = drivers.multiShoot_CRTBP_direct(X, U, *args, ops=drivers.HipDirectOps(lto.MU, lto.DU, lto.TU, ISP, gpu_ctx),
                                                           verbose=False)
    py = dict(drivers.multiShoot_CRTBP_direct.last)
    print("direct demo: library loop %d iterations, history %s" % (lib["iterations"], np.array2string(lib["history"][:, :lib["iterations"]], precision=3)))
    assert lib["status"] == 0 and np.abs(defect_l).max() <= 1e-6
    assert py["status"] == 0 and np.abs(defect_p).max() <= 1e-6
    assert lib["iterations"] == py["iterations"]
    assert np.abs(Xl - Xp).max() <= 1e-8


@pytest.mark.gpu
def test_solve_batch_equals_single_solves(gpu_ctx):
    demo = DH.demo()
    X, U, t, tau1, tau2, a, b, c, d = demo.demo_problem()
    B = 4
    Xb = np.repeat(X[:, :, None], B, axis=2)
    Ub = np.zeros((3, 30, B))
    Tb = np.repeat(t[:, None], B, axis=1) * (1.0 + 0.05 * np.arange(B))[None, :]
    tgs = []
    for k in range(B):
        s0, sf = drivers.interpEndStates(tau1 + 0.01 * k, tau2 - 0.01 * k, a, b, c, d)
        tgs.append(lto.direct_targets(s0, sf, 1000.0, np.zeros(3), np.zeros(3)))
    out_b = lto.direct_solve(np.asfortranarray(Xb), np.asfortranarray(Ub), np.asfortranarray(Tb), NSTEPS, lto.MU, lto.DU, lto.TU, ISP,
                             tgs, maxIter=100, ctx=gpu_ctx)
    for k in range(B):
        out_s = lto.direct_solve(X, np.zeros((3, 30)), Tb[:, k], NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tgs[k], maxIter=100, ctx=gpu_ctx)
        assert out_s[5] == out_b[5][k] == 0 and out_s[6] == out_b[6][k]
        for j in (0, 1, 4):
            assert np.abs(out_s[j] - out_b[j][..., k]).max() <= 1e-12 * max(1.0, np.abs(out_s[j]).max())
    # NaN input: status 2, promptly
    Xn = X.copy()
    Xn[0, 5] = np.nan
    out = lto.direct_solve(Xn, np.zeros((3, 30)), t, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tgs[0], maxIter=100, ctx=gpu_ctx)
    assert out[5] == 2 and out[6] <= 1
