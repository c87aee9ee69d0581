"""GPU checks of the indirect method's mesh equidistribution (lto_indirect_remesh_batch) on the demo transfer taken
down the rho ladder (examples/halo_remesh_demo.rho_ladder): the grid against the host restatement (tests/remesh_reference.py), the
new nodes against the CPU oracle's flow, the almost-converged guess and the re-solve, the drop of the longest chain of trial steps,
the same trajectory before and after, batch == singles, the large-n path of both kernels, the driver and the refusals.

Measured figures (MI355X; each test prints its own before it asserts) are written beside the assertions that use them."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import addtime_reference as A  # noqa: E402
import remesh_reference as R  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP16 = 16 * np.finfo(np.float64).eps

# Measured on the fixture (MI355X), see the tests that use them.
GUESS_DEFECT_RATIO = 4.343      # max |defect| of the guess on the new grid / max(old max |defect|, 1e-13)
STEPS_MAX_AFTER = 8             # max trial steps per segment after two passes (before: see the fixture's docstring)
DENSE_DIFF = 2.138e-12          # rows 0-5 of the 300-point dense outputs, re-solved against input (_rel_err)
COST_DIFF = 7.598e-12           # relative difference of the costs


@pytest.fixture(scope="module")
def demo():
    spec = importlib.util.spec_from_file_location("halo_remesh_demo_t", os.path.join(ROOT, "examples", "halo_remesh_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def ladder(demo):
    """The demo's converged p = 2 transfer (solve_p2, as tests/test_add_time_gpu.py builds it), p = 1 at 0.05 N, then rho halved
    down to 1/32 on the uniform 30-node grid; the fixture level is the last one.  Its trial steps per segment (DOP853 at 1e-13, one
    defect sweep): 5 9 8 12 16 13 10 7 5 4 4 3 3 3 3 3 3 3 4 5 8 9 9 13 10 9 7 5 4 -- max 16, mean 6.79, total 197: the two lunar
    passes take four to five times the steps of the coast between them."""
    t, levels = demo.rho_ladder()
    assert levels[-1][0] == demo.RHO_TARGET, [r for r, _ in levels]
    return t, levels


@pytest.fixture(scope="module")
def fix(demo, ladder):
    t, levels = ladder
    rho, XC = levels[-1]
    return XC, t, demo.params(rho), rho


@pytest.fixture(scope="module")
def solved(fix):
    XC, t, prm, _ = fix
    return lto.indirect_remesh(XC, t, prm, passes=2, maxIter=10)


def _rel_err(a, b):
    """max over components of |a - b| / max |b| (per component row)."""
    scale = np.maximum(np.abs(b).max(axis=1, keepdims=True), 1e-300)
    return float((np.abs(a - b) / scale).max())


def _check_grid(t, w, t_out, n_new):
    want, _ = R.new_grid(t, w, n_new)
    err = np.abs(t_out - want).max()
    print("grid n=%d -> %d: max |t_out - restatement| = %.3e (%.2f ulp of t_end)" % (t.size, n_new, err, err / (np.finfo(float).eps * abs(t[-1]))))
    assert t_out[0] == t[0] and t_out[-1] == t[-1]
    assert err <= ULP16 * abs(t[-1])
    assert np.all(np.diff(t_out) > 0.0)


@pytest.mark.parametrize("n_new", [15, 30, 120])
@pytest.mark.parametrize("kind", ["reals", "integers", "counts"])
def test_grid_matches_the_restatement(fix, kind, n_new):
    XC, t, prm, _ = fix
    n = t.size
    rng = np.random.default_rng(7)
    if kind == "counts":
        r = lto.indirect_remesh(XC, t, prm, n_new=n_new, passes=1, solve=False)
        w = r.steps_before.astype(np.float64)
        assert np.all(w >= 1)
    else:
        w = rng.uniform(0.2, 9.0, n - 1) if kind == "reals" else rng.integers(1, 9, n - 1).astype(np.float64)
        r = lto.indirect_remesh(XC, t, prm, n_new=n_new, weights=w, passes=1, solve=False)
    assert r.XC_out is None and r.XC_guess.shape == (12, n_new) and r.t_out.shape == (n_new,)
    _check_grid(t, w, r.t_out, n_new)


@pytest.mark.parametrize("case", ["dop853", "rk4"])
def test_identity(fix, case):
    XC, t, prm, _ = fix
    integ = lto.integrator(lto.RK4, steps=64) if case == "rk4" else lto.integrator()
    r = lto.indirect_remesh(XC, t, prm, weights=np.ones(t.size - 1), passes=1, integ=integ, solve=False)
    err = _rel_err(r.XC_guess, XC)
    print("identity (%s): max |t_out - t| = %.3e, XC_guess vs XC %.3e" % (case, np.abs(r.t_out - t).max(), err))
    assert np.abs(r.t_out - t).max() <= ULP16 * abs(t[-1])
    assert err <= 1e-12
    assert np.array_equal(r.XC_guess[:, 0], XC[:, 0]) and np.array_equal(r.XC_guess[:, -1], XC[:, -1])


@pytest.mark.parametrize("case", ["dop853", "rk4"])
@pytest.mark.parametrize("n_new", [17, 30, 90])
def test_nodes_match_the_oracle_flow(fix, oracle, case, n_new):
    XC, t, prm, rho = fix
    integ = lto.integrator(lto.RK4, steps=64) if case == "rk4" else lto.integrator()
    method, steps = (oracle.RK4, 64) if case == "rk4" else (oracle.DOP853_ADAPTIVE, 0)
    r = lto.indirect_remesh(XC, t, prm, n_new=n_new, weights=np.random.default_rng(3).uniform(0.5, 4.0, t.size - 1), passes=1,
                            integ=integ, solve=False)
    oprm = oracle.make_params(MU, DU, TU, 0.05, 1e3, 1.0, 1.0, rho)
    src, span = R.sources(t, r.t_out)
    want = np.zeros_like(r.XC_guess)
    for k in range(n_new):
        if span[k] == 0.0:
            want[:, k] = XC[:, src[k]]
            assert np.array_equal(r.XC_guess[:, k], XC[:, src[k]])
        else:
            want[:, k], rc, _, _ = oracle.flow_state_costate(XC[:, src[k]], oprm, span[k], method, steps)
            assert rc == 0
    err = _rel_err(r.XC_guess, want)
    print("nodes (%s, n_new = %d): XC_guess vs oracle flow %.3e" % (case, n_new, err))
    assert src[-1] == t.size - 1 and span[-1] == 0.0
    assert err <= 1e-10


def test_guess_is_almost_converged_and_resolve_converges(fix, solved):
    XC, t, prm, _ = fix
    r = solved
    d_old, _ = lto.indirect_defectCalc(XC, t, prm)
    d_guess, _ = lto.indirect_defectCalc(r.XC_guess, r.t_out, prm)
    ratio = np.abs(d_guess).max() / max(np.abs(d_old).max(), 1e-13)
    print("old max |defect| %.3e, guess max |defect| on the new grid %.3e, ratio %.3f; re-solve: status %d, %d iterations, max |defect| %.3e"
          % (np.abs(d_old).max(), np.abs(d_guess).max(), ratio, r.status, r.iterations, np.abs(r.defect).max()))
    assert r.status == 0
    assert np.abs(r.defect).max() <= 1e-10
    assert np.array_equal(r.XC_out[:6, 0], XC[:6, 0]) and np.array_equal(r.XC_out[:6, -1], XC[:6, -1])
    assert r.t_out[0] == t[0] and r.t_out[-1] == t[-1]
    # measured: 1.865e-14 before, 4.343e-13 for the guess: ratio 4.343 (one Newton iteration then gives 1.38e-14)
    assert ratio <= 10 * GUESS_DEFECT_RATIO


def test_longest_chain_gets_shorter(solved):
    r = solved
    b, a = r.steps_before, r.steps_after
    print("trial steps before: max %d mean %.3f total %d; after: max %d mean %.3f total %d"
          % (b.max(), b.mean(), b.sum(), a.max(), a.mean(), a.sum()))
    print("before:", b.tolist())
    print("after: ", a.tolist())
    assert a.max() < b.max()
    # measured: max 16 / mean 6.79 / total 197 before, max 8 / mean 6.72 / total 195 after
    assert a.max() <= STEPS_MAX_AFTER + 1


def test_same_trajectory(fix, solved):
    XC, t, prm, rho = fix
    r = solved
    D0, td0 = lto.densify(XC, t, prm, 300)
    D1, td1 = lto.densify(r.XC_out, r.t_out, prm, 300)
    assert np.array_equal(td0, td1)
    diff = _rel_err(D1[:6], D0[:6])
    c0 = A.dense_cost(D0, td0, 0.05, 1.0, rho, 1e3, DU, TU)
    c1 = A.dense_cost(D1, td1, 0.05, 1.0, rho, 1e3, DU, TU)
    cd = abs(c1 - c0) / abs(c0)
    print("dense output rows 0-5: %.3e; cost %.15g -> %.15g (relative %.3e)" % (diff, c0, c1, cd))
    # measured: 2.138e-12 and 7.598e-12 (both solutions have defects <= 1e-10; the transfer passes the Moon twice)
    assert diff <= 10 * DENSE_DIFF
    assert cd <= 10 * COST_DIFF


def test_batch_equals_singles(demo, ladder):
    t, levels = ladder
    lv = levels[-3:]
    prms = [demo.params(rho) for rho, _ in lv]
    first = [lto.indirect_remesh(X, t, p, passes=1, maxIter=10) for (_, X), p in zip(lv, prms)]
    assert all(f.status == 0 for f in first)
    XB = np.asfortranarray(np.stack([f.XC_out for f in first], axis=2))
    TB = np.asfortranarray(np.stack([f.t_out for f in first], axis=1))
    assert not np.array_equal(TB[:, 0], TB[:, 1])           # every level on its own grid
    rb = lto.indirect_remesh(XB, TB, prms, passes=2, maxIter=10)
    for b in range(3):
        r1 = lto.indirect_remesh(XB[:, :, b], TB[:, b], prms[b], passes=2, maxIter=10)
        assert np.array_equal(rb.t_out[:, b], r1.t_out)
        assert np.array_equal(rb.XC_guess[:, :, b], r1.XC_guess)
        assert np.array_equal(rb.XC_out[:, :, b], r1.XC_out)
        assert np.array_equal(rb.steps_before[:, b], r1.steps_before) and np.array_equal(rb.steps_after[:, b], r1.steps_after)
        assert rb.status[b] == r1.status and rb.iterations[b] == r1.iterations
        assert np.array_equal(rb.history[b], r1.history)


@pytest.mark.parametrize("n,n_new", [(4097, 4097), (65537, 65537), (65537, 3000), (3000, 65537)])
def test_large_n_through_both_kernels(oracle, n, n_new):
    """Up to 4 096 segments the running sum lives in LDS, above in the global-memory form of the same code; the weights are reals,
    so the two forms and the restatement agree only because they sum in the same order."""
    XC, T = synth.indirect_problem(n, 1, seed=5)
    XC, t = XC[:, :, 0], T[:, 0]
    prm = lto.make_params(MU, DU, TU, 0.05, 1e3, 1.0, 1.0, 0.1)
    w = np.random.default_rng(n + n_new).uniform(0.2, 9.0, n - 1)
    r = lto.indirect_remesh(XC, t, prm, n_new=n_new, weights=w, passes=1, integ=lto.integrator(lto.RK4, steps=8), solve=False)
    _check_grid(t, w, r.t_out, n_new)
    src, span = R.sources(t, r.t_out)
    oprm = oracle.make_params(MU, DU, TU, 0.05, 1e3, 1.0, 1.0, 0.1)
    ks = np.unique(np.concatenate([[0, 1, n_new - 2, n_new - 1], np.random.default_rng(1).integers(0, n_new, 60)]))
    got, want = r.XC_guess[:, ks], np.zeros((12, ks.size))
    for j, k in enumerate(ks):
        want[:, j] = XC[:, src[k]] if span[k] == 0.0 else oracle.flow_state_costate(XC[:, src[k]], oprm, span[k], oracle.RK4, 8)[0]
    err = _rel_err(got, want)
    print("large n %d -> %d: %d sampled nodes vs oracle flow %.3e" % (n, n_new, ks.size, err))
    assert err <= 1e-10
    assert np.array_equal(r.XC_guess[:, 0], XC[:, 0]) and np.array_equal(r.XC_guess[:, -1], XC[:, -1])
    assert np.all(np.isfinite(r.XC_guess))


def test_driver_return_convention(fix):
    XC, t, _, rho = fix
    n = t.size
    before = XC.copy()
    X1, t1, n1 = drivers.meshRefine_indirect(XC, t, MU, DU, TU, n, 1e3, 0.05, 1.0, rho, verbose=False)
    assert n1 == n and X1.shape == (12, n) and t1.shape == (n,) and not np.array_equal(t1, t)
    assert np.array_equal(XC, before)
    X2, t2, n2 = drivers.meshRefine_indirect(XC, t, MU, DU, TU, n, 1e3, 0.05, 1.0, rho, n_new=45, passes=1, verbose=False)
    assert n2 == 45 and X2.shape == (12, 45) and t2[0] == t[0] and t2[-1] == t[-1]
    # no iteration allowed: the loop reports status 1 and the caller's arrays come back
    X3, t3, n3 = drivers.meshRefine_indirect(XC, t, MU, DU, TU, n, 1e3, 0.05, 1.0, rho, maxIter=0, verbose=False)
    assert n3 == n and np.array_equal(X3, before) and np.array_equal(t3, t)


def test_refusals(fix):
    XC, t, prm, _ = fix
    n = t.size

    def code(XC=XC, t=t, **kw):
        kw.setdefault("solve", False)
        with pytest.raises(lto.LtoError) as ei:
            lto.indirect_remesh(XC, t, prm, **kw)
        return ei.value.code

    XC14 = np.vstack([XC[:6], np.full((1, n), 1e3), XC[6:], np.zeros((1, n))])
    assert code(XC=XC14) == -3
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
    # the library's own checks of the weights, behind the Python layer's
    ctx = lto.default_context()
    for bad in (0.0, -2.0, np.nan, np.inf):
        w = np.ones(n - 1)
        w[3] = bad
        t_out = np.zeros(n)
        integ = lto.integrator()
        rc = ctx.fn("indirect_remesh")(ctx.handle, 12, n, XC.ctypes.data, np.ascontiguousarray(t).ctypes.data, ctypes.byref(prm), ctypes.byref(integ), n,
                                       w.ctypes.data, 1, 0, 10, t_out.ctypes.data, None, None, None, None, None, None, None, None)
        assert rc == -1
