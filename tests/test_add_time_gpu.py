"""GPU checks of addTimeFinal on the device (lto_indirect_add_time_batch): the re-mesh and the snap onto the arrival
orbit against the host restatement (tests/addtime_reference.py) fed by the library's own densify, the ballistic coast along the
arrival halo, the fixed-end re-solve from the demo's converged p = 2 transfer, batch == singles, the cost, the driver's return
convention and the refusals."""
import importlib.util
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import addtime_reference as R  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU, day  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASS, THRUST = 1e3, 10.0
N_DESIRED = 200


@pytest.fixture(scope="module")
def p2():
    """The demo's converged p = 2 transfer (examples/halo_transfer_demo.solve_p2) and the arrival table."""
    spec = importlib.util.spec_from_file_location("halo_demo_addtime", os.path.join(ROOT, "examples", "halo_transfer_demo.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    XC, t, defect, flag = mod.solve_p2(seed=0, verbose=False)
    assert flag == 0
    tab = synth.halo_orbits()[1]
    times = np.linspace(0.0, 1.0, tab.shape[1])
    return np.asfortranarray(XC), np.asarray(t, dtype=np.float64), times, np.asfortranarray(tab[:6])


def _params(p=2.0, rho=1.0):
    return lto.make_params(MU, DU, TU, THRUST, MASS, 1.0, p, rho)


def _rel_err(a, b):
    """max over components of |a - b| / max |b| (per component row)."""
    scale = np.maximum(np.abs(b).max(axis=1, keepdims=True), 1e-300)
    return float((np.abs(a - b) / scale).max())


@pytest.mark.parametrize("case", ["dop853_p2", "rk4_p2", "dop853_p1"])
def test_remesh_and_snap_match_the_restatement(p2, case):
    XC, t, times, tab = p2
    n = t.size
    integ = lto.integrator(lto.RK4, steps=64) if case.startswith("rk4") else lto.integrator()
    prm = _params(1.0, 1.0) if case.endswith("p1") else _params()
    dts = np.array([0.25, 0.5, 1.0, 2.0]) * day / TU
    r = lto.indirect_add_time(XC, t, prm, times, tab, dts, n_desired=N_DESIRED, integ=integ, solve=False)
    assert r.XC_out is None and r.XC_guess.shape == (12, n, 4)
    taus = np.arange(1001) / 1000.0
    _, S, _, _, _, _ = lto.direct_end_states(np.vstack([taus, taus]), (times, tab, times, tab))   # the device's s(tau_j)
    for k, dt in enumerate(dts):
        G = r.XC_guess[:, :, k]
        XCe, te = R.extended(XC, t, dt)
        XCd, td = lto.densify(XCe, te, prm, N_DESIRED, integ)
        want, t_new = R.remesh(XCd, td, n)
        assert np.array_equal(r.t_out[:, k], t_new)
        assert r.t_out[-1, k] == t[-1] + dt
        assert np.array_equal(G[:, 0], XC[:, 0])                  # bit for bit
        assert np.all(G[6:, -1] == 0.0)
        assert _rel_err(G[:, :-1], want[:, :-1]) < 1e-12
        assert _rel_err(G[6:, -1:], want[6:, -1:]) < 1e-12
        tau = r.tau[k]
        assert tau * 1000.0 == np.round(tau * 1000.0)
        _, sf, _, _, _, _ = lto.direct_end_states([tau, tau], (times, tab, times, tab))
        assert np.abs(G[:6, -1] - sf).max() <= 1e-15 * max(1.0, np.abs(sf).max())
        j, d = R.find_tau_from_samples(S, XCd[:6, -1])
        jd = int(round(tau * 1000.0))
        assert jd == j or abs(d[jd] - d[j]) <= 1e-15, (jd, j, d[jd], d[j])


def test_end_coasts_along_the_arrival_halo(p2):
    XC, t, times, tab = p2
    dts = np.array([0.1, 0.25, 0.5, 0.75, 1.0]) * day / TU
    r = lto.indirect_add_time(XC, t, _params(), times, tab, dts, n_desired=N_DESIRED, solve=False)
    tau0, _ = R.find_tau(times, tab, XC[:6, -1])
    for k, dt in enumerate(dts):
        want = (tau0 + dt / (99 * synth.HALO_DT[1])) % 1.0
        err = abs(r.tau[k] - want)
        assert min(err, 1.0 - err) <= 2e-3, (dt, r.tau[k], want)


@pytest.fixture(scope="module")
def solved(p2):
    XC, t, times, tab = p2
    dts = np.array([0.25, 0.5, 1.0]) * day / TU
    return dts, lto.indirect_add_time(XC, t, _params(), times, tab, dts, n_desired=N_DESIRED, maxIter=10)


def test_end_to_end_resolve_converges(p2, solved):
    XC, t, times, tab = p2
    dts, r = solved
    for k in range(dts.size):
        hist = r.history[k]
        assert r.status[k] == 0, (k, r.iterations[k], hist)
        assert np.abs(r.defect[:, :, k]).max() <= 1e-10, (k, hist)
        _, sf, _, _, _, _ = lto.direct_end_states([r.tau[k], r.tau[k]], (times, tab, times, tab))
        assert np.abs(r.XC_out[:6, -1, k] - sf).max() <= 1e-15 * max(1.0, np.abs(sf).max())
        assert np.array_equal(r.XC_out[:6, 0, k], XC[:6, 0])
        assert r.t_out[-1, k] == t[-1] + dts[k]


def test_cost_matches_numpy(solved):
    dts, r = solved
    for k in range(dts.size):
        XCd, td = lto.densify(r.XC_out[:, :, k], r.t_out[:, k], _params(), N_DESIRED)
        want = R.dense_cost(XCd, td, THRUST, 2.0, 1.0, MASS, DU, TU)
        assert abs(r.cost[k] - want) <= 1e-12 * abs(want), (r.cost[k], want)
        assert r.cost[k] > 0.0


def test_batch_equals_singles(p2):
    XC, t, times, tab = p2
    dts = np.linspace(0.25, 2.0, 8) * day / TU
    rb = lto.indirect_add_time(XC, t, _params(), times, tab, dts, n_desired=N_DESIRED, maxIter=10)
    for k, dt in enumerate(dts):
        r1 = lto.indirect_add_time(XC, t, _params(), times, tab, [dt], n_desired=N_DESIRED, maxIter=10)
        assert np.array_equal(rb.XC_guess[:, :, k], r1.XC_guess[:, :, 0])
        assert np.array_equal(rb.XC_out[:, :, k], r1.XC_out[:, :, 0])
        assert rb.status[k] == r1.status[0] and rb.iterations[k] == r1.iterations[0]
        assert np.array_equal(rb.history[k], r1.history[0])
        assert rb.tau[k] == r1.tau[0]


def test_driver_return_convention(p2):
    XC, t, times, tab = p2
    n = t.size
    before = XC.copy()
    dt = 0.5 * day / TU
    XC_new, t_new = drivers.addTimeFinal(XC, t, dt, MU, DU, TU, n, MASS, THRUST, 2.0, 1.0, times, tab, maxIter=10, verbose=False)
    assert XC_new.shape == (12, n) and t_new[-1] == t[-1] + dt
    assert not np.array_equal(XC_new, XC)
    assert np.array_equal(XC, before)                            # the caller's array is not changed
    # one iteration cannot converge a re-meshed guess: the original arrays come back, end costates included
    XC_same, t_same = drivers.addTimeFinal(XC, t, day / TU, MU, DU, TU, n, MASS, THRUST, 2.0, 1.0, times, tab, maxIter=1, verbose=False)
    assert np.array_equal(XC_same, before) and np.array_equal(t_same, t)


def test_tf_sweep(p2):
    XC, t, times, tab = p2
    dts = np.array([0.25, 0.5]) * day / TU
    out = drivers.tf_sweep(XC, t, dts, MU, DU, TU, MASS, THRUST, 2.0, 1.0, times, tab)
    assert np.array_equal(out["status"], [0, 0])
    np.testing.assert_array_equal(out["tof"], (t[-1] + dts) - t[0])
    assert np.all(out["max_defect"] <= 1e-10) and np.all(out["cost"] > 0.0)


def test_refusals(p2):
    XC, t, times, tab = p2
    dt = [0.5 * day / TU]

    def code(**kw):
        args = dict(XC=XC, t=t, params=_params(), Xf_times=times, Xf_states=tab, dts=dt, n_desired=N_DESIRED, solve=False)
        args.update(kw)
        with pytest.raises(lto.LtoError) as ei:
            lto.indirect_add_time(**args)
        return ei.value.code

    XC14 = np.vstack([XC[:6], np.full((1, t.size), MASS), XC[6:], np.zeros((1, t.size))])
    assert code(XC=XC14) == -3
    assert code(integ=lto.integrator(lto.RKF78_ADAPTIVE)) == -3
    assert code(integ=lto.integrator(lto.RKF78_FIXED, steps=8)) == -3
    assert code(dts=[0.0]) == -1
    assert code(dts=[-0.1]) == -1
    assert code(dts=[np.nan]) == -1
    assert code(dts=[np.inf]) == -1
    assert code(n_desired=3) == -1
