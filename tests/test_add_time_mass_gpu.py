"""GPU checks of addTimeFinal for the 14-row variable-mass system (lto_indirect_add_time_mass_batch): the snap onto the
arrival orbit, the Isp -> infinity reduction to lto_indirect_add_time at a frozen 1000 kg, the finite-Isp transfer end to end with
its propellant curve, batch == singles bit for bit, the drivers' conventions and the refusals.  The kernels' shapes, the tail and
the cost branches are in test_add_time_mass_shapes_gpu.py, the CPU side in test_add_time_mass_host.py.

Bars.  Isp = 1e30 against the 12-row call: the dense samples of the two systems differ by at most e = max(1e-11, 10 e_inf)
per row (mass_dense_reference.e_inf: the oracle's 14-row flow at Isp = 1e30 against its 12-row flow), and the re-mesh maps a sample
error e to at most Lambda e at a node (addtime_mass_reference.spline_norm(200, 30), test_add_time_mass_host.py), so the guesses agree
to Lambda e per row; the re-solved trajectories to 1e-8 of the row scale and the mass to 1e-9 relative, the bars of
test_indirect_mass_gpu.py's reduction.  Finite Isp: propellant against drivers.thrust_arcs_mass within 10 e_dm relative
(thrust_mass_reference.bars).

Every test prints its figures before it asserts (MEASURED lines)."""
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import addtime_mass_reference as AM  # noqa: E402
import addtime_reference as R  # noqa: E402
import mass_dense_reference as M  # noqa: E402
import thrust_mass_reference as TM  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU, day  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
THRUST, ISP, M0 = 10.0, 2000.0, 1000.0
N_DESIRED = 200
EPS = np.finfo(np.float64).eps
DTS = np.array([0.25, 0.5, 1.0]) * day / TU


def _params(isp=ISP, p=2.0, rho=1.0):
    return lto.make_params(MU, DU, TU, THRUST, isp, 1.0, p, rho)


@pytest.fixture(scope="module")
def p2():
    """The demo's converged p = 2 transfer (examples/halo_transfer_demo.solve_p2) and the arrival table."""
    spec = importlib.util.spec_from_file_location("halo_demo_addtime_mass", os.path.join(ROOT, "examples", "halo_transfer_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    XC, t, defect, flag = mod.solve_p2(seed=0, verbose=False)
    assert flag == 0
    tab = synth.halo_orbits()[1]
    times = np.linspace(0.0, 1.0, tab.shape[1])
    return np.asfortranarray(XC), np.asarray(t, dtype=np.float64), times, np.asfortranarray(tab[:6])


@pytest.fixture(scope="module")
def finite_isp(p2):
    """That transfer lifted to 14 rows and solved on the device at Isp = 2000 s, 10 N, as tests/test_mass_remesh_gpu.py builds it."""
    XC, t, times, tab = p2
    n = XC.shape[1]
    Xs, defect, st = drivers.multiShoot_CRTBP_indirect_mass(drivers.lift_to_mass(XC, M0), t, MU, DU, TU, n, ISP, THRUST, False, False, 50,
                                                            2.0, 1.0, verbose=False)
    assert st == 0 and np.abs(defect).max() <= 1e-10
    return np.asfortranarray(Xs), t, times, tab


@pytest.fixture(scope="module")
def solved(finite_isp):
    Xs, t, times, tab = finite_isp
    return lto.indirect_add_time_mass(Xs, t, _params(), times, tab, DTS, n_desired=N_DESIRED, maxIter=10)


def _candidates(times, tab):
    taus = np.arange(1001) / 1000.0
    _, S, _, _, _, _ = lto.direct_end_states(np.vstack([taus, taus]), (times, tab, times, tab))   # the device's s(tau_j)
    return np.array(S)


@pytest.mark.parametrize("case", ["dop853", "rk4"])
def test_snap_matches_the_restatement(finite_isp, case):
    """The assertions of test_add_time_gpu.py::test_remesh_and_snap_match_the_restatement on rows 0..5 of the last node and tau."""
    Xs, t, times, tab = finite_isp
    n = t.size
    integ = lto.integrator(lto.RK4, steps=64) if case == "rk4" else lto.integrator()
    dts = np.array([0.25, 0.5, 1.0, 2.0]) * day / TU
    r = lto.indirect_add_time_mass(Xs, t, _params(), times, tab, dts, n_desired=N_DESIRED, integ=integ, solve=False)
    assert r.XC_out is None and r.XC_guess.shape == (14, n, 4)
    S = _candidates(times, tab)
    for k, dt in enumerate(dts):
        G = r.XC_guess[:, :, k]
        XCe, te = AM.extended14(Xs, t, dt)
        XCd, td = lto.densify_mass(XCe, te, _params(), N_DESIRED, integ)
        tau = r.tau[k]
        assert tau * 1000.0 == np.round(tau * 1000.0)
        _, sf, _, _, _, _ = lto.direct_end_states([tau, tau], (times, tab, times, tab))
        assert np.abs(G[:6, -1] - sf).max() <= 1e-15 * max(1.0, np.abs(sf).max())
        j, d = R.find_tau_from_samples(S, XCd[:6, -1])
        jd = int(round(tau * 1000.0))
        assert jd == j or abs(d[jd] - d[j]) <= 1e-15, (jd, j, d[jd], d[j])
        assert G[6, -1] == XCd[6, -1]                                 # the mass of the last node stays the spline's end sample
        assert np.all(G[7:, -1] == 0.0)


def test_isp_to_infinity_is_the_12_row_call(p2):
    XC, t, times, tab = p2
    X14 = drivers.lift_to_mass(XC, M0)
    lam = AM.spline_norm(N_DESIRED, t.size)
    bar = lam * max(1e-11, 10.0 * M.e_inf())
    prm12 = lto.make_params(MU, DU, TU, THRUST, M0, 1.0, 2.0, 1.0)
    r12 = lto.indirect_add_time(XC, t, prm12, times, tab, DTS, n_desired=N_DESIRED, maxIter=10)
    r14 = lto.indirect_add_time_mass(X14, t, _params(isp=1e30), times, tab, DTS, n_desired=N_DESIRED, maxIter=10)
    S = _candidates(times, tab)
    assert np.array_equal(r14.t_out, r12.t_out)
    for k, dt in enumerate(DTS):
        G14, G12 = r14.XC_guess[:, :, k], r12.XC_guess[:, :, k]
        same_tau = r14.tau[k] == r12.tau[k]
        if not same_tau:                                              # two candidates all but equally far from the unsnapped end
            XCd, _ = lto.densify_mass(*AM.extended14(X14, t, dt), _params(isp=1e30), N_DESIRED)
            _, d = R.find_tau_from_samples(S, XCd[:6, -1])
            j14, j12 = int(round(r14.tau[k] * 1000.0)), int(round(r12.tau[k] * 1000.0))
            print("MEASURED Isp = 1e30 dt %.3f TU: tau %.3f against %.3f, distances %.17g and %.17g" % (dt, r14.tau[k], r12.tau[k], d[j14], d[j12]))
            assert abs(d[j14] - d[j12]) <= 2.0 * bar
        cols = slice(None) if same_tau else slice(0, -1)
        e_guess = max(M.rel_rows(G14[:6, cols], G12[:6, cols]), M.rel_rows(G14[7:13], G12[6:12]))
        e_mass = float(np.abs(G14[6] - M0).max())
        print("MEASURED Isp = 1e30 dt %.3f TU: guess rows 0..5, 7..12 against the 12-row guess %.3e (bar %.3e = Lambda %.4f x e), "
              "mass row within %.3e kg of 1000 (bar %.3e)" % (dt, e_guess, bar, lam, e_mass, 4.0 * EPS * M0))
        assert e_guess <= bar
        assert np.all(G14[13] == 0.0)
        assert e_mass <= 4.0 * EPS * M0
        X14o, X12o = r14.XC_out[:, :, k], r12.XC_out[:, :, k]
        scale = np.maximum(1.0, np.abs(X12o).max(axis=1, keepdims=True))
        e_out = float(np.abs((X14o[M.IDX12] - X12o) / scale).max())
        e_m = float(np.abs(X14o[6] / M0 - 1.0).max())
        print("MEASURED Isp = 1e30 dt %.3f TU: status %d / %d after %d / %d iterations, rows against the 12-row result %.3e (bar 1e-8), "
              "mass %.3e relative (bar 1e-9), propellant %.3e kg, cost %.9f against %.9f"
              % (dt, r14.status[k], r12.status[k], r14.iterations[k], r12.iterations[k], e_out, e_m, r14.propellant[k], r14.cost[k], r12.cost[k]))
        assert r14.status[k] == r12.status[k]
        assert e_out < 1e-8 and e_m < 1e-9
        assert r14.propellant[k] == 0.0 or abs(r14.propellant[k]) < 4.0 * EPS * M0


def test_finite_isp_end_to_end(finite_isp, solved):
    Xs, t, times, tab = finite_isp
    r = solved
    _, _, bdm = TM.bars()
    print("MEASURED finite Isp: base propellant %.9f kg over %.4f TU" % (Xs[6, 0] - Xs[6, -1], t[-1] - t[0]))
    for k, dt in enumerate(DTS):
        X = r.XC_out[:, :, k]
        arcs = drivers.thrust_arcs_mass(X, r.t_out[:, k], MU, DU, TU, ISP, THRUST, 2.0, 1.0)
        rel = abs(r.propellant[k] - arcs["propellant_kg"]) / arcs["propellant_kg"]
        print("MEASURED finite Isp dt %.2f day (tof %.4f TU): status %d after %d iterations, max |defect| %.3e, tau %.3f, propellant %.9f kg "
              "(thrust_arcs_mass %.9f, relative %.3e, bar %.1e), cost %.9f DU/TU" % (dt * TU / day, r.t_out[-1, k] - r.t_out[0, k], r.status[k],
              r.iterations[k], np.abs(r.defect[:, :, k]).max(), r.tau[k], r.propellant[k], arcs["propellant_kg"], rel, bdm, r.cost[k]))
    for k, dt in enumerate(DTS):
        X = r.XC_out[:, :, k]
        assert r.status[k] == 0, (k, r.iterations[k], r.history[k])
        assert np.abs(r.defect[:, :, k]).max() <= 1e-10, (k, r.history[k])
        assert np.array_equal(X[0:7, 0], Xs[0:7, 0])                  # pins, bit for bit
        assert np.array_equal(X[0:6, -1], r.XC_guess[0:6, -1, k])
        _, sf, _, _, _, _ = lto.direct_end_states([r.tau[k], r.tau[k]], (times, tab, times, tab))
        assert np.abs(X[:6, -1] - sf).max() <= 1e-15 * max(1.0, np.abs(sf).max())
        assert X[13, -1] == 0.0
        assert np.all(np.diff(X[6]) <= 0.0)
        assert r.t_out[-1, k] == t[-1] + dt
        assert r.propellant[k] > 0.0 and r.propellant[k] == Xs[6, 0] - X[6, -1]
        arcs = drivers.thrust_arcs_mass(X, r.t_out[:, k], MU, DU, TU, ISP, THRUST, 2.0, 1.0)
        assert abs(r.propellant[k] - arcs["propellant_kg"]) <= bdm * arcs["propellant_kg"]
        assert r.cost[k] > 0.0


def test_batch_equals_singles(finite_isp):
    Xs, t, times, tab = finite_isp
    dts = np.linspace(0.25, 2.0, 8) * day / TU
    rb = lto.indirect_add_time_mass(Xs, t, _params(), times, tab, dts, n_desired=N_DESIRED, maxIter=10)
    for k, dt in enumerate(dts):
        r1 = lto.indirect_add_time_mass(Xs, t, _params(), times, tab, [dt], n_desired=N_DESIRED, maxIter=10)
        assert np.array_equal(rb.XC_guess[:, :, k], r1.XC_guess[:, :, 0])
        assert np.array_equal(rb.XC_out[:, :, k], r1.XC_out[:, :, 0])
        assert rb.status[k] == r1.status[0] and rb.iterations[k] == r1.iterations[0]
        assert np.array_equal(rb.history[k], r1.history[0])
        assert rb.tau[k] == r1.tau[0]
        assert rb.propellant[k] == r1.propellant[0] and rb.cost[k] == r1.cost[0]


def test_driver_return_convention(finite_isp):
    Xs, t, times, tab = finite_isp
    n = t.size
    before = Xs.copy()
    dt = 0.5 * day / TU
    X_new, t_new = drivers.addTimeFinal_mass(Xs, t, dt, MU, DU, TU, n, ISP, THRUST, 2.0, 1.0, times, tab, maxIter=10, verbose=False)
    assert X_new.shape == (14, n) and t_new[-1] == t[-1] + dt
    assert not np.array_equal(X_new, Xs) and X_new[13, -1] == 0.0 and np.array_equal(X_new[0:7, 0], Xs[0:7, 0])
    assert np.array_equal(Xs, before)                            # the caller's array is not changed
    # one iteration cannot converge a re-meshed guess: the original arrays come back, end costates included
    X_same, t_same = drivers.addTimeFinal_mass(Xs, t, day / TU, MU, DU, TU, n, ISP, THRUST, 2.0, 1.0, times, tab, maxIter=1, verbose=False)
    assert np.array_equal(X_same, before) and np.array_equal(t_same, t)


def test_tf_sweep_mass(finite_isp):
    Xs, t, times, tab = finite_isp
    dts = DTS[:2]
    out = drivers.tf_sweep_mass(Xs, t, dts, MU, DU, TU, ISP, THRUST, 2.0, 1.0, times, tab)
    assert np.array_equal(out["status"], [0, 0]) and out["XC"].shape == (14, t.size, 2)
    np.testing.assert_array_equal(out["tof"], (t[-1] + dts) - t[0])
    assert np.all(out["max_defect"] <= 1e-10) and np.all(out["cost"] > 0.0)
    assert np.all(out["propellant_kg"] > 0.0)
    assert np.array_equal(out["mass_final_kg"], out["XC"][6, -1, :])
    assert np.array_equal(out["propellant_kg"], Xs[6, 0] - out["mass_final_kg"])


def test_refusals(p2, finite_isp):
    XC, _, _, _ = p2
    Xs, t, times, tab = finite_isp
    n = t.size
    dt = [0.5 * day / TU]

    def code(**kw):
        args = dict(XC=Xs, t=t, params=_params(), Xf_times=times, Xf_states=tab, dts=dt, n_desired=N_DESIRED, solve=False)
        args.update(kw)
        with pytest.raises(lto.LtoError) as ei:
            lto.indirect_add_time_mass(**args)
        return ei.value.code

    assert code(integ=lto.integrator(lto.RKF78_ADAPTIVE)) == -3
    assert code(integ=lto.integrator(lto.RKF78_FIXED, steps=8)) == -3
    assert code(dts=[0.0]) == -1
    assert code(dts=[-0.1]) == -1
    assert code(dts=[np.nan]) == -1
    assert code(dts=[np.inf]) == -1
    assert code(n_desired=3) == -1
    for bad, node in ((0.0, 0), (-3.0, n // 2), (np.nan, n - 1)):
        Xb = Xs.copy(order="F")
        Xb[6, node] = bad
        assert code(XC=Xb) == -1, (bad, node)
    # 12 rows: the Python layers refuse before any library call
    with pytest.raises(ValueError):
        lto.indirect_add_time_mass(XC, t, _params(), times, tab, dt, solve=False)
    with pytest.raises(ValueError):
        drivers.addTimeFinal_mass(XC, t, dt[0], MU, DU, TU, n, ISP, THRUST, 2.0, 1.0, times, tab, verbose=False)
    with pytest.raises(ValueError):
        drivers.tf_sweep_mass(XC, t, dt, MU, DU, TU, ISP, THRUST, 2.0, 1.0, times, tab)
    # the 12-row entry keeps refusing 14 rows
    with pytest.raises(lto.LtoError) as ei:
        lto.indirect_add_time(Xs, t, lto.make_params(MU, DU, TU, THRUST, M0, 1.0, 2.0, 1.0), times, tab, dt, n_desired=N_DESIRED, solve=False)
    assert ei.value.code == -3
