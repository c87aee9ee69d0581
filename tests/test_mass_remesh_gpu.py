"""Mesh equidistribution of 14-row variable-mass solutions on the device (lto_indirect_remesh_mass_batch, k_remesh_nodes<14>;
DESIGN 4.20): the grid against the host restatement (remesh_reference.new_grid), the guess against the oracle's flow of
remesh_reference.sources, the identity, the re-solve of the exactly consistent p = 1 and p = 0 fixtures and of the device-solved
finite-Isp p = 2 transfer, the step counts, batch == singles, the refusals and the driver's return convention.

Fixtures and bars: tests/mass_dense_reference.py.  Per row relative to max(1, max |reference row|): DOP853 1e-11, RK4 x 64 1e-10 (both
against the oracle's flow by the same method from the same old node); mass row besides to max(10 e_m, 64 eps m0) kg; a re-solved
consistent problem to 1e-8 of the oracle's trajectory from node 0 (the bar of test_indirect_mass_gpu.py).

Measured on an MI355X: every grid equal to the restatement bit for bit; nodes 7.4e-15 (DOP853) and 1.7e-14 (RK4 x 64), mass row
2.3e-13 and 7.3e-12 kg (bar 1.42e-11 kg); re-solved p = 1 fixture 4.5e-12 (9 -> 9) and 3.3e-12 (9 -> 17) from the oracle's trajectory;
finite-Isp p = 2: status 0, steps max 10 -> 5, propellant 2.900192101 kg before and after, relative difference 7.5e-13.

The p = 0 fixture (costates determined up to a positive factor: a singular last system, kernels_bvp.hip bvp_final_qr14's rank rule):
9 -> 9 6.8e-12, 9 -> 17 2.1e-12, status 0 after one iteration; before that rule 18.47 (every costate x 19.47) and status 1.  DESIGN 4.20.

Every test prints its figures before it asserts (MEASURED lines)."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mass_dense_reference as M  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP16 = 16 * np.finfo(np.float64).eps


def _integ(mname):
    method, steps = M.METHODS[mname]
    return lto.integrator(method, steps=steps)


def _check_grid(t, w, t_out, n_new):
    want, _ = M.new_grid(t, w, n_new)
    err = np.abs(t_out - want).max()
    print("MEASURED grid n=%d -> %d: max |t_out - restatement| = %.3e (%.2f ulp of t_end)" % (t.size, n_new, err, err / (np.finfo(float).eps * abs(t[-1]))))
    assert t_out[0] == t[0] and t_out[-1] == t[-1]
    assert err <= ULP16 * abs(t[-1])
    assert np.all(np.diff(t_out) > 0.0)


@pytest.mark.parametrize("kind", ["reals", "integers", "counts"])
@pytest.mark.parametrize("n,n_new", M.REMESH_SHAPES)
def test_grid_matches_the_restatement(gpu_ctx, n, n_new, kind):
    k = 0 if n > 9 else (n_new + len(kind)) % len(M.SETS)
    X, t, prm = M.fixture(n, k)
    p = lto.make_params(*prm)
    rng = np.random.default_rng(7 + n_new)
    if kind == "counts":
        r = lto.indirect_remesh_mass(X, t, p, n_new=n_new, passes=1, solve=False, ctx=gpu_ctx)
        w = r.steps_before.astype(np.float64)
        assert np.all(w >= 1)
    else:
        w = rng.uniform(0.2, 9.0, n - 1) if kind == "reals" else rng.integers(1, 9, n - 1).astype(np.float64)
        r = lto.indirect_remesh_mass(X, t, p, n_new=n_new, weights=w, passes=1, solve=False, ctx=gpu_ctx)
    assert r.XC_out is None and r.XC_guess.shape == (14, n_new) and r.t_out.shape == (n_new,)
    assert np.array_equal(r.XC_guess[:, 0], X[:, 0]) and np.array_equal(r.XC_guess[:, -1], X[:, -1])
    _check_grid(np.array(t), w, r.t_out, n_new)


@pytest.mark.parametrize("k", [0, 3], ids=lambda k: M.SETS[k].name)
def test_identity(gpu_ctx, k):
    X, t, prm = M.fixture(9, k)
    r = lto.indirect_remesh_mass(X, t, lto.make_params(*prm), weights=np.ones(8), passes=1, solve=False, ctx=gpu_ctx)
    err = M.rel_rows(r.XC_guess, X)
    em = float(np.abs(r.XC_guess[6] - X[6]).max())
    print("MEASURED identity %s: max |t_out - t| = %.3e, XC_guess vs XC %.3e, mass row %.3e kg" % (M.SETS[k].name, np.abs(r.t_out - t).max(), err, em))
    assert np.abs(r.t_out - t).max() <= ULP16 * abs(t[-1])
    assert np.array_equal(r.XC_guess[:, 0], X[:, 0]) and np.array_equal(r.XC_guess[:, -1], X[:, -1])
    assert err <= M.TOL["dop853"]


@pytest.mark.parametrize("mname", ["dop853", "rk4x64"])
@pytest.mark.parametrize("n,n_new,k", M.REMESH_NODE_CASES, ids=["%dto%d-%s" % (n, m, M.SETS[k].name) for n, m, k in M.REMESH_NODE_CASES])
def test_nodes_match_the_oracle_flow(gpu_ctx, oracle, n, n_new, k, mname):
    X, t, prm = M.fixture(n, k)
    method, steps = M.METHODS[mname]
    _, e_m = M.self_errors()
    w = np.random.default_rng(3 + n_new).uniform(0.5, 4.0, n - 1)
    r = lto.indirect_remesh_mass(X, t, lto.make_params(*prm), n_new=n_new, weights=w, passes=1, integ=_integ(mname), solve=False, ctx=gpu_ctx)
    want, src, span = M.guess_expected(oracle, X, t, prm, r.t_out, method, steps)
    if prm[6] > 1:
        assert M.clamp_gap(want, prm).min() >= M.CLAMP_CLEARANCE
    zero = np.flatnonzero(span == 0.0)
    for j in zero:
        assert np.array_equal(r.XC_guess[:, j], X[:, src[j]]), j                 # bit for bit
    err = M.rel_rows(r.XC_guess, want)
    em = float(np.abs(r.XC_guess[6] - want[6]).max())
    print("MEASURED nodes %d -> %d %s %s: XC_guess vs oracle flow %.3e (bar %.0e), mass row %.3e kg (bar %.3e kg), %d zero spans"
          % (n, n_new, M.SETS[k].name, mname, err, M.TOL[mname], em, M.mass_bar(e_m), zero.size))
    assert 0 in zero and n_new - 1 in zero and src[-1] == n - 1
    assert np.all(np.isfinite(r.XC_guess))
    assert err <= M.TOL[mname]
    assert em <= M.mass_bar(e_m)


def _check_resolved(r, X, label):
    assert r.status == 0, (label, r.status)
    assert np.abs(r.defect).max() <= 1e-10
    assert np.array_equal(r.XC_out[0:7, 0], X[0:7, 0]) and np.array_equal(r.XC_out[0:6, -1], X[0:6, -1])
    assert r.XC_out[13, -1] == 0.0
    assert np.all(np.diff(r.XC_out[6]) <= 0.0)


@pytest.mark.parametrize("n_new", [9, 17])
@pytest.mark.parametrize("k", [0, 5], ids=lambda k: M.SETS[k].name)
def test_resolve_of_a_consistent_fixture(gpu_ctx, oracle, k, n_new):
    X, t, prm = M.fixture(9, k)
    r = lto.indirect_remesh_mass(X, t, lto.make_params(*prm), n_new=n_new, passes=2, maxIter=10, ctx=gpu_ctx)
    print("MEASURED re-solve %s 9 -> %d: status %d after %d iterations, max |defect| %.3e, steps max %d -> %d"
          % (M.SETS[k].name, n_new, r.status, r.iterations, np.abs(r.defect).max(), r.steps_before.max(), r.steps_after.max()))
    _check_resolved(r, X, M.SETS[k].name)
    assert r.t_out[0] == t[0] and r.t_out[-1] == t[-1]
    want = M.trajectory_expected(oracle, X, t, prm, r.t_out)
    err = M.rel_rows(r.XC_out, want)
    print("MEASURED re-solve %s 9 -> %d: XC_out against the oracle's trajectory from node 0 %.3e (bar 1e-8)" % (M.SETS[k].name, n_new, err))
    assert err < 1e-8


@pytest.fixture(scope="module")
def finite_isp():
    """The demo's p = 2 transfer lifted to 14 rows and solved on the device at Isp = 2000 s, 10 N, as
    tests/test_indirect_mass_gpu.py::finite_isp builds it."""
    spec = importlib.util.spec_from_file_location("halo_demo_mr", os.path.join(ROOT, "examples", "halo_transfer_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    XC, t, _, flag = demo.solve_p2(verbose=False)
    assert flag == 0
    n = XC.shape[1]
    Xs, defect, st = drivers.multiShoot_CRTBP_indirect_mass(drivers.lift_to_mass(XC, 1000.0), t, MU, DU, TU, n, 2000.0, 10.0,
                                                            False, False, 50, 2.0, 1.0, verbose=False)
    assert st == 0 and np.abs(defect).max() <= 1e-10
    return np.asfortranarray(Xs), np.asarray(t, dtype=np.float64)


def test_resolve_of_the_finite_isp_transfer(gpu_ctx, finite_isp):
    Xs, t = finite_isp
    r = lto.indirect_remesh_mass(Xs, t, lto.make_params(MU, DU, TU, 10.0, 2000.0, 1.0, 2.0, 1.0), passes=2, maxIter=10, ctx=gpu_ctx)
    a0 = drivers.thrust_arcs_mass(Xs, t, MU, DU, TU, 2000.0, 10.0, 2.0, 1.0, ctx=gpu_ctx)
    print("MEASURED finite-Isp p = 2: status %d after %d iterations, max |defect| %.3e, steps max %d -> %d, mean %.2f -> %.2f"
          % (r.status, r.iterations, np.abs(r.defect).max(), r.steps_before.max(), r.steps_after.max(), r.steps_before.mean(), r.steps_after.mean()))
    _check_resolved(r, Xs, "finite Isp")
    a1 = drivers.thrust_arcs_mass(r.XC_out, r.t_out, MU, DU, TU, 2000.0, 10.0, 2.0, 1.0, ctx=gpu_ctx)
    print("MEASURED finite-Isp p = 2: propellant %.9f kg -> %.9f kg, relative difference %.3e"
          % (a0["propellant_kg"], a1["propellant_kg"], abs(a1["propellant_kg"] - a0["propellant_kg"]) / a0["propellant_kg"]))
    assert r.steps_after.max() <= r.steps_before.max()


def test_two_passes_report_the_first_sweeps_counts(gpu_ctx):
    X, t, prm = M.fixture(66, 0)
    p = lto.make_params(*prm)
    r1 = lto.indirect_remesh_mass(X, t, p, passes=1, solve=False, ctx=gpu_ctx)
    r2 = lto.indirect_remesh_mass(X, t, p, passes=2, solve=False, ctx=gpu_ctx)
    print("MEASURED counts 66 nodes: before max %d mean %.2f; after one pass max %d, after two max %d"
          % (r1.steps_before.max(), r1.steps_before.mean(), r1.steps_after.max(), r2.steps_after.max()))
    assert np.array_equal(r2.steps_before, r1.steps_before)
    assert np.all(r1.steps_before >= 1) and r1.steps_after.shape == (65,)


def test_batch_equals_singles(gpu_ctx):
    XB, TB, prm_l = M.remesh_batch_problem()
    prms = [lto.make_params(*q) for q in prm_l]
    assert [q[6] for q in prm_l] == [1.0, 1.0, 0.0] and not np.array_equal(TB[:, 0], TB[:, 1])
    rb = lto.indirect_remesh_mass(XB, TB, prms, n_new=11, passes=2, maxIter=10, ctx=gpu_ctx)
    for b in range(3):
        r1 = lto.indirect_remesh_mass(XB[:, :, b], TB[:, b], prms[b], n_new=11, passes=2, maxIter=10, ctx=gpu_ctx)
        assert np.array_equal(rb.t_out[:, b], r1.t_out)
        assert np.array_equal(rb.XC_guess[:, :, b], r1.XC_guess)
        assert np.array_equal(rb.XC_out[:, :, b], r1.XC_out)
        assert rb.status[b] == r1.status == 0 and rb.iterations[b] == r1.iterations
        assert np.array_equal(rb.steps_before[:, b], r1.steps_before) and np.array_equal(rb.steps_after[:, b], r1.steps_after)


def test_refusals(gpu_ctx):
    X, t, prm = M.fixture(9, 0)
    X, t = np.asfortranarray(X), np.array(t)
    p = lto.make_params(*prm)
    n = 9

    def code(X=X, t=t, **kw):
        kw.setdefault("solve", False)
        with pytest.raises(lto.LtoError) as ei:
            lto.indirect_remesh_mass(X, t, p, ctx=gpu_ctx, **kw)
        return ei.value.code

    assert code(integ=lto.integrator(lto.RKF78_ADAPTIVE)) == -3
    assert code(integ=lto.integrator(lto.RKF78_FIXED, steps=8)) == -3
    assert code(integ=lto.integrator(lto.RK4, steps=8)) == -1                    # no counts without an adaptive integrator
    assert code(passes=0) == -1
    assert code(weights=np.ones(n - 1), passes=2) == -1
    assert code(n_new=1) == -1
    tb = t.copy()
    tb[5] = tb[4]
    assert code(t=tb) == -1
    assert code(t=t[::-1].copy()) == -1
    # the library's own checks, behind the Python layer's
    fn = gpu_ctx.fn("indirect_remesh_mass")
    integ, rk4 = lto.integrator(), lto.integrator(lto.RK4, steps=8)
    w, t_out = np.ones(n - 1), np.zeros(n)

    def call(X=X.ctypes.data, t=t.ctypes.data, prm=ctypes.byref(p), integ=ctypes.byref(integ), n_new=n, w=None, passes=1, t_out=t_out.ctypes.data):
        return fn(gpu_ctx.handle, n, X, t, prm, integ, n_new, w, passes, 0, 10, t_out, None, None, None, None, None, None, None, None)

    assert call() == 0
    assert call(integ=ctypes.byref(rk4)) == -1
    assert call(w=w.ctypes.data, passes=2) == -1
    assert call(n_new=1) == -1
    assert call(t=tb.ctypes.data) == -1
    for bad in (0.0, -2.0, np.nan, np.inf):
        wb = np.ones(n - 1)
        wb[3] = bad
        assert call(w=wb.ctypes.data) == -1
    for null in ("X", "t", "prm", "integ", "t_out"):
        assert call(**{null: None}) == -2, null
    # XC_out without status_flag
    out = np.zeros((14, n), order="F")
    assert fn(gpu_ctx.handle, n, X.ctypes.data, t.ctypes.data, ctypes.byref(p), ctypes.byref(integ), n, None, 1, 0, 10, t_out.ctypes.data,
              None, out.ctypes.data, None, None, None, None, None, None) == -2
    # the 12-row entry keeps refusing 14 rows
    with pytest.raises(lto.LtoError) as ei:
        lto.indirect_remesh(X, t, p, solve=False, ctx=gpu_ctx)
    assert ei.value.code == -3


def test_driver_return_convention(gpu_ctx):
    X, t, prm = M.fixture(9, 0)
    X, t = np.asfortranarray(X), np.array(t)
    s = M.SETS[0]
    before = X.copy()
    X1, t1, n1 = drivers.meshRefine_indirect_mass(X, t, MU, DU, TU, 9, s.isp, s.thrust, s.p, s.rho, ctx=gpu_ctx, verbose=False)
    assert n1 == 9 and X1.shape == (14, 9) and t1.shape == (9,) and not np.array_equal(t1, t)
    assert np.array_equal(X, before) and X1[13, -1] == 0.0 and np.array_equal(X1[0:7, 0], X[0:7, 0])
    X2, t2, n2 = drivers.meshRefine_indirect_mass(X, t, MU, DU, TU, 9, s.isp, s.thrust, s.p, s.rho, n_new=14, passes=1, ctx=gpu_ctx, verbose=False)
    assert n2 == 14 and X2.shape == (14, 14) and t2[0] == t[0] and t2[-1] == t[-1]
    # no iteration allowed: the loop reports status 1 and the caller's arrays come back
    X3, t3, n3 = drivers.meshRefine_indirect_mass(X, t, MU, DU, TU, 9, s.isp, s.thrust, s.p, s.rho, maxIter=0, ctx=gpu_ctx, verbose=False)
    assert n3 == 9 and np.array_equal(X3, before) and np.array_equal(t3, t)
