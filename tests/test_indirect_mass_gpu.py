"""The 14-dim variable-mass indirect solve on the device: the Newton step of the structured cyclic reduction (NX = 14) against
dense linear algebra on the same device STMs, the library loop against the Python mirror, the Isp -> infinity reduction to the
12-dim demo solution, a finite-Isp transfer and the batched solve.  Rows: (r, v, m, lambda_r, lambda_v, lambda_m); pinned:
XC[0:7, 0], XC[0:6, -1], XC[13, -1] = 0 (free final mass)."""
import importlib.util
import os

import numpy as np
import pytest

import bvp_reference as R
import lowthrustopt_amd as lto
from lowthrustopt_amd import drivers, synth
from lowthrustopt_amd.constants import MU, DU, TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G0 = 9.81
pytestmark = pytest.mark.gpu


def guess14(n, n_batch, seed):
    XC, T = synth.indirect_problem(n, n_batch=n_batch, seed=seed, dt_range=(0.05, 0.2))
    X14 = drivers.lift_to_mass(XC, 1000.0)
    X14[6] -= 0.01 * np.arange(n)[:, None]
    X14[13] = 0.2
    X14[13, -1] = 0.0
    return X14, T


@pytest.mark.parametrize("n_nodes,n_batch", [(2, 1), (3, 1), (30, 1), (31, 2), (200, 3)])
@pytest.mark.parametrize("adjoints_only", [False, True])
def test_device_step_vs_dense(gpu_ctx, n_nodes, n_batch, adjoints_only):
    import torch
    X14, T = guess14(n_nodes, n_batch, 41)
    prm = lto.make_params(MU, DU, TU, 0.05, 2000.0, 1.0, 1.0, 1.0)
    S, J = (n_nodes - 1) * n_batch, n_nodes * n_batch
    plan = lto.IndirectPlan(gpu_ctx, n_nodes, n_batch, prm, lto.integrator(lto.RKF78_FIXED, steps=6), ndim=14)
    X = torch.from_numpy(synth.to_soa_nodes(X14)).cuda()
    t = torch.from_numpy(np.ascontiguousarray(T.T)).cuda()
    Phi = torch.zeros(196, S, dtype=torch.float64, device="cuda")
    d = torch.zeros(14, S, dtype=torch.float64, device="cuda")
    delta = torch.full((14, J), float("nan"), dtype=torch.float64, device="cuda")
    plan.jacobian(X, J, t, n_batch, Phi, S, d, S)
    plan.newton_solve(Phi, S, d, S, delta, J, adjoints_only=adjoints_only)
    d2 = d * 0.5 + 0.01
    delta2 = torch.full((14, J), float("nan"), dtype=torch.float64, device="cuda")
    plan.newton_solve(None, 0, d2, S, delta2, J, adjoints_only=adjoints_only)
    with pytest.raises(lto.LtoError):                 # the other variant was never factored
        plan.newton_solve(None, 0, d2, S, delta2, J, adjoints_only=not adjoints_only)
    torch.cuda.synchronize()
    Pn = Phi.cpu().numpy().reshape(14, 14, n_batch, n_nodes - 1).transpose(1, 0, 3, 2)
    free = R.free_mask(14, n_nodes, adjoints_only).reshape(-1, order="F")
    for dd, de in ((d, delta), (d2, delta2)):
        dn = dd.cpu().numpy().reshape(14, n_batch, n_nodes - 1).transpose(0, 2, 1)
        den = de.cpu().numpy().reshape(14, n_batch, n_nodes).transpose(0, 2, 1)
        assert np.all(np.isfinite(den))
        for b in range(n_batch):
            x = den[:, :, b]
            assert np.all(x[R.pinned_mask(14, n_nodes)] == 0.0)
            if adjoints_only:
                assert np.all(x[0:7] == 0.0)
            Jd = lto.indirect_scatter_mass(np.asfortranarray(Pn[:, :, :, b]))
            rhs = -dn[:, :, b].reshape(-1, order="F")
            Jf = Jd[:, free]
            xv = x.reshape(-1, order="F")
            if adjoints_only:
                ref = np.linalg.lstsq(Jf, rhs, rcond=None)[0]
                res = Jf.T @ (Jf @ xv[free] - rhs)            # normal equations
                assert np.abs(res).max() < 1e-9 * max(1.0, np.abs(Jf).max() * np.abs(rhs).max())
            else:
                ref = np.linalg.solve(Jf, rhs)
                res = Jf @ xv[free] - rhs
                assert np.abs(res).max() < 1e-9 * max(1.0, np.abs(rhs).max())
            assert np.abs(xv[free] - ref).max() < 1e-7 * max(1.0, np.abs(ref).max())
    plan.close()


def test_newton_step_vs_host_step(gpu_ctx):
    n = 12
    X14, T = guess14(n, 1, 42)
    X14, t = X14[:, :, 0], T[:, 0]
    integ = lto.integrator(lto.RKF78_FIXED, steps=6)
    prm = lto.make_params(MU, DU, TU, 0.05, 2000.0, 1.0, 1.0, 1.0)
    ops = drivers.HipOps(gpu_ctx, integ)
    for adj in (False, True):
        upd, defect = lto.indirect_newton_step(X14, t, prm, integ, ctx=gpu_ctx, flag_adjointsOnly=adj)
        Phi, d = ops.stm(X14, t, prm)
        assert np.array_equal(d, defect)
        ref = drivers.optimizeTraj_OLS_mass(X14, t, d, Phi, n, prm, adj, ops)
        assert np.abs(upd - ref).max() <= 1e-9 * max(1.0, np.abs(ref).max())
        assert np.all(upd[R.pinned_mask(14, n)] == 0.0)


def consistent_problem(ctx, n=12):
    """Nodes on ONE trajectory of the device's flow at p = 1, rho = 1, lambda_m shifted to lambda_m(tf) = 0."""
    XC, T = synth.indirect_problem(n, seed=4, lam_sigma=0.1)
    t = T[:, 0]
    prm = lto.make_params(MU, DU, TU, 0.05, 2000.0, 1.0, 1.0, 1.0)
    X = np.zeros((14, n), order="F")
    X[:, 0] = drivers.lift_to_mass(XC[:, :1, 0], 1000.0)[:, 0]
    X[13, 0] = 0.4
    for k in range(n - 1):
        pair = np.asfortranarray(np.stack([X[:, k], np.zeros(14)], axis=1))
        d, _ = lto.indirect_defectCalc(pair, t[k:k + 2], prm, lto.integrator(), ctx=ctx)
        X[:, k + 1] = d[:, 0]
    X[13] -= X[13, -1]
    rng = np.random.default_rng(5)
    X0 = X.copy()
    X0[:, 1:-1] += 1e-3 * rng.standard_normal((14, n - 2)) * np.maximum(1e-3, np.abs(X[:, 1:-1]))
    X0[6, -1] += 1e-3
    X0[13, -1] = 0.7                                  # overwritten by the solver on entry
    return X, X0, t


class CountingOps(drivers.HipOps):
    iterations = 0

    def stm(self, XC, t, params):
        self.iterations += 1
        return super().stm(XC, t, params)


def test_solve_consistent_problem_device_and_mirror(gpu_ctx):
    X, X0, t = consistent_problem(gpu_ctx)
    n = X.shape[1]
    prm = lto.make_params(MU, DU, TU, 0.05, 2000.0, 1.0, 1.0, 1.0)
    Xd, dd, st, its, _ = lto.indirect_solve(X0, t, prm, None, False, 20, ctx=gpu_ctx)
    Xs, ds, st2 = drivers.multiShoot_CRTBP_indirect_mass(X0, t, MU, DU, TU, n, 2000.0, 0.05, False, False, 20, 1.0, 1.0, verbose=False)
    assert st == 0 and st2 == 0 and np.array_equal(Xs, Xd) and np.abs(dd).max() <= 1e-10
    assert np.array_equal(Xd[0:7, 0], X0[0:7, 0]) and np.array_equal(Xd[0:6, -1], X0[0:6, -1]) and Xd[13, -1] == 0.0
    scale = np.maximum(1.0, np.abs(X).max(axis=1, keepdims=True))
    assert np.abs((Xd - X) / scale).max() < 1e-8
    ops = CountingOps(gpu_ctx)
    Xm, dm, st3 = drivers.multiShoot_CRTBP_indirect_mass(X0, t, MU, DU, TU, n, 2000.0, 0.05, False, False, 20, 1.0, 1.0, ops=ops, verbose=False)
    assert st3 == 0 and ops.iterations == its
    assert np.abs((Xm - Xd) / scale).max() < 1e-9


@pytest.fixture(scope="module")
def demo_p2(gpu_ctx):
    spec = importlib.util.spec_from_file_location("halo_demo", os.path.join(ROOT, "examples", "halo_transfer_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    XC, t, defect, flag = demo.solve_p2(verbose=False)
    assert flag == 0
    return XC, t


def test_isp_to_infinity_reduces_to_the_12_dim_solution(demo_p2):
    XC, t = demo_p2
    n = XC.shape[1]
    X14 = drivers.lift_to_mass(XC, 1000.0)
    Xs, defect, st = drivers.multiShoot_CRTBP_indirect_mass(X14, t, MU, DU, TU, n, 1e12, 10.0, False, False, 20, 2.0, 1.0, verbose=False)
    assert st == 0 and np.abs(defect).max() <= 1e-10
    idx = [0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11, 12]
    scale = np.maximum(1.0, np.abs(XC).max(axis=1, keepdims=True))
    assert np.abs((Xs[idx] - XC) / scale).max() < 1e-8
    assert np.abs(Xs[6] / 1000.0 - 1.0).max() < 1e-9


@pytest.fixture(scope="module")
def finite_isp(demo_p2):
    XC, t = demo_p2
    n = XC.shape[1]
    Xs, defect, st = drivers.multiShoot_CRTBP_indirect_mass(drivers.lift_to_mass(XC, 1000.0), t, MU, DU, TU, n, 2000.0, 10.0,
                                                            False, False, 50, 2.0, 1.0, verbose=False)
    return Xs, t, defect, st


def test_finite_isp_transfer(finite_isp):
    Xs, t, defect, st = finite_isp
    assert st == 0 and np.abs(defect).max() <= 1e-10
    assert np.all(np.diff(Xs[6]) <= 0.0)
    fuel = Xs[6, 0] - Xs[6, -1]
    tf = (t[-1] - t[0]) * TU
    assert 0.0 < fuel <= 10.0 * tf / (2000.0 * G0)
    assert Xs[13, -1] == 0.0 and Xs[6, 0] == 1000.0


def test_batch_of_rho_levels_equals_single_solves(gpu_ctx, finite_isp):
    Xs, t, _, _ = finite_isp
    rhos = (1.0, 0.5, 0.25)
    prms = [lto.make_params(MU, DU, TU, 0.05, 2000.0, 1.0, 1.0, r) for r in rhos]
    XB = np.asfortranarray(np.repeat(Xs[:, :, None], 3, axis=2))
    Xb, Db, stb, itb, _ = lto.indirect_solve_batch(XB, t, prms, None, False, 6, ctx=gpu_ctx)
    for k in range(3):
        X1, D1, st1, it1, _ = lto.indirect_solve(Xs, t, prms[k], None, False, 6, ctx=gpu_ctx)
        assert np.array_equal(Xb[:, :, k], X1) and np.array_equal(Db[:, :, k], D1)
        assert stb[k] == st1 and itb[k] == it1
