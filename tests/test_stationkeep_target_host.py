"""CPU checks for the target-point station-keeping calls: the independent reference
(tests/stationkeep_target_reference.py) against itself -- the symplectic identity, the composition of its STMs, the monodromy matrix
of the packaged orbits, the minimum property of the law, the gains loops against numpy -- and against itself at a looser tolerance:
for every quantity the GPU tests (tests/test_stationkeep_target_gpu.py) compare, its own spread between (rtol, atol) = (1e-13,
1e-14) and (1e-12, 1e-13) has to stay below a tenth of the bound the device is held to, each bound being ten times the spread seen,
rounded up to a power of ten (the rule of DESIGN 4.29).  Then the vetting of the Monte Carlo the drivers' GPU test flies, and the
argument checks of the Python layer.

Flights under this law are a class of their own beside LAW / FREE / RK4 of tests/test_stationkeep_host.py, because the feedback
decides how far a difference is amplified: the target-point law feeds the whole deviation back, not one component of it."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import manifold_reference as MR  # noqa: E402
import stationkeep_reference as SR  # noqa: E402
import stationkeep_target_reference as TR  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, hotpath, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402

# ---- the bounds of tests/test_stationkeep_target_gpu.py, each ten times the reference's own spread, rounded up to a power of ten
GPU_X = 1e-10            # X_out, absolute, DU and DU/TU                                               spread 2.1e-12
GPU_X_TGT = 1e-8         # X_tgt: up to 1.8 periods from state0 along an orbit with lambda_u ~ 1500    spread 2.3e-10
GPU_PHI = 1e-8           # Phi, relative to the largest entry of its 6 x 6 block                       spread 9.2e-10
GPU_G = 1e-9             # G from the device's Phi against G from the reference's, relative to max |G|  spread 9.5e-11
GPU_RK4_X = 1e-5         # RK4 x 400 per span against DOP853, in the reference: X_out                  spread 1.3e-7
GPU_RK4_X_TGT = 1e-4     # ... X_tgt                                                                   spread 7.1e-6
GPU_RK4_PHI = 1e-3       # ... Phi, relative                                                           spread 2.9e-5
RK4_STEPS = 400
# flights under the target-point law: (x_final, dev_r, dev_v, dv_hist, dv_total, dev_final), absolute, DU and DU/TU
GPU_TARGET = dict(x=1e-11, dev_r=1e-11, dev_v=1e-11, hist=1e-11, total=1e-11, dev_final=1e-11)   # spread 5.7e-13 2.1e-13 6.3e-13 4.2e-13 8.9e-13 5.6e-13
# the Monte Carlo at 20 revolutions, from tests/golden/stationkeep_target_mc.json: (dv_total, x_final, dev_final)
GPU_TARGET_MC = dict(total=1e-10, x=1e-11, dev_final=1e-10)     # spread 2.6e-12 9.9e-13 1.1e-12
# dv_total per run of the same Monte Carlo under the DEVICE's law against the reference's flights under the reference's law, DU/TU.
# Not a spread but a first-order estimate: the laws differ by GPU_X in X_ref and by GPU_G max |G| in every entry of G.  A burn c =
# G (x - X_ref + nav) then moves by at most |G|_F sqrt(6) GPU_X + sqrt(18) GPU_G max |G| |d| with max |G| = 2.6 (|G|_F <= sqrt(18)
# max |G| = 11) and |d| <= 3e-5 (4 km, 1 cm/s and the navigation error): 2.7e-9 + 3.3e-13.  The closed loop holds a difference instead
# of growing it (that is what the law is for), but a moved burn moves the later deviations and with them the later burns; a factor 4
# for that, over 80 burns: 80 x 4 x 2.7e-9 = 8.7e-7, rounded up.  dv_total itself is about 5e-4.
GPU_TARGET_MC_LAW = 1e-6

# ---- the Monte Carlo of the drivers' GPU test, vetted in the reference by tests/golden/gen_stationkeep_target_mc.py
MONTE_CARLO = dict(n_rev=20, n_runs=16, inj_sigma_r_km=1.0, inj_sigma_v_ms=0.01, nav_sigma_r_km=0.1, nav_sigma_v_ms=0.001,
                   exe_sigma_frac=0.01, exe_sigma_ms=1e-4, r_lost_km=5000.0, seed=3)
MC_MARGIN = 100.0        # the reference's largest deviation under the law stays this factor below r_lost

KM, MS = DU, DU / TU * 1e3
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stationkeep_target_mc.json")


@pytest.fixture(scope="module")
def orbits():
    return MR.packaged_orbits(synth.halo_orbits(), MU)


def monte_carlo_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def rel_block(a, b):
    """max |a - b| of Phi [6 x 6 x ...] relative to the largest entry of each 6 x 6 block of b, the largest over the blocks."""
    return float((np.abs(a - b).max(axis=(0, 1)) / np.abs(b).max(axis=(0, 1))).max())


# ------------------------------------------------------------------------------------------------------ 1. the reference's own STMs
@pytest.mark.parametrize("k", [0, 1])
def test_reference_stms_are_symplectic(orbits, k):
    """Phi^T S Phi = S with S of DESIGN 4.29; the residual scales with |Phi|^2 times the integration error."""
    s = TR.stms(orbits, [k], TR.TAUS3, TR.HORIZONS, MU)
    worst = 0.0
    for j in range(3):
        for h in range(2):
            Phi = s.Phi[:, :, h, j, 0]
            res = np.abs(Phi.T @ SR.S @ Phi - SR.S).max() / np.abs(Phi).max() ** 2
            worst = max(worst, res)
    print("orbit %d: |Phi^T S Phi - S| / max |Phi|^2 <= %.2e" % (k + 1, worst))
    assert worst <= GPU_PHI


def test_reference_stms_compose(orbits):
    """Phi(0.5 P, 0) = Phi(0.5 P, 0.25 P) Phi(0.25 P, 0)."""
    a = TR.stms(orbits, [0], (0.0,), (0.25, 0.5), MU)
    b = TR.stms(orbits, [0], (0.25,), (0.25,), MU)
    whole = a.Phi[:, :, 1, 0, 0]
    parts = b.Phi[:, :, 0, 0, 0] @ a.Phi[:, :, 0, 0, 0]
    d = np.abs(whole - parts).max() / np.abs(whole).max()
    print("composition over 0.25 P + 0.25 P: %.2e relative, the point at phase 0.25 both ways %.2e"
          % (d, np.abs(a.X_tgt[:, 0, 0, 0] - b.X[:, 0, 0]).max()))
    assert d <= GPU_PHI and np.abs(a.X_tgt[:, 0, 0, 0] - b.X[:, 0, 0]).max() <= GPU_X
    assert np.abs(a.X_tgt[:, 1, 0, 0] - b.X_tgt[:, 0, 0, 0]).max() <= GPU_X


@pytest.mark.parametrize("k", [0, 1])
def test_reference_stm_over_one_period_is_the_monodromy_matrix(orbits, k):
    s = TR.stms(orbits, [k], (0.0,), (1.0,), MU)
    M = orbits[k][2]
    d = np.abs(s.Phi[:, :, 0, 0, 0] - M).max() / np.abs(M).max()
    print("orbit %d: Phi(P, 0) against the packaged M (99 spans): %.2e relative" % (k + 1, d))
    assert d <= GPU_PHI
    assert np.array_equal(s.X[:, 0, 0], orbits[k][0])                       # tau = 0 flies nothing


# --------------------------------------------------------------------------------------------------------------- 2. the law itself
def test_the_law_minimises_the_cost(orbits):
    """J(G dx + steps along each axis) >= J(G dx) for random dx: the loops' G is the minimiser."""
    rng = np.random.RandomState(5)
    for k in (0, 1):
        L = TR.law(orbits, k, TR.TAUS3, MU)
        for j in range(3):
            Phi, G = L.Phi[:, :, :, j], L.G[:, :, j]
            for _ in range(5):
                dx = rng.standard_normal(6) * np.array([1e-5] * 3 + [1e-4] * 3)
                dv = G @ dx
                J0 = TR.cost(Phi, TR.Q, (1.0, 1.0), dx, dv)
                for axis in range(3):
                    for step in (1e-3, -1e-3, 1e-1, -1e-1):
                        e = np.zeros(3)
                        e[axis] = step * np.linalg.norm(dv)
                        assert TR.cost(Phi, TR.Q, (1.0, 1.0), dx, dv + e) >= J0


@pytest.mark.parametrize("q,r", [(TR.Q, (1.0, 1.0)), (1e-4, (0.5, 2.0)), (0.0, (1.0, 0.0))])
def test_gains_loops_against_numpy(orbits, q, r):
    """The loops' G against numpy.linalg.solve, to round-off times cond(H)."""
    eps = np.finfo(float).eps
    for k in (0, 1):
        s = TR.stms(orbits, [k], TR.TAUS3, TR.HORIZONS, MU)
        G, pivot, status = TR.gains(s.Phi[..., 0], q, r)
        assert np.all(status == 0) and np.all(pivot > 0.0) and np.all(pivot <= 1.0)
        for j in range(3):
            H, N = TR.normal_matrices(s.Phi[:, :, :, j, 0], q, r)
            ref = -np.linalg.solve(H, N)
            cond = np.linalg.cond(H)
            d = np.abs(G[:, :, j] - ref).max() / np.abs(ref).max()
            print("orbit %d phase %.2f q %.0e: cond(H) %.1e, pivot %.1e, loops against numpy %.1e" % (k + 1, TR.TAUS3[j], q, cond, pivot[j], d))
            assert d <= 50.0 * eps * cond


def test_gains_loops_flag_bad_records():
    rng = np.random.RandomState(6)
    Phi = rng.standard_normal((6, 6, 2, 4))
    Phi[2, 3, 1, 1] = np.nan
    Phi[:3, 3:, :, 2] = 0.0                                     # B = 0 in every block: H = q I
    G, pivot, status = TR.gains(Phi, 0.0, (1.0, 1.0))
    assert list(status) == [0, 2, 3, 0]
    assert np.all(np.isnan(G[:, :, 1:3])) and np.all(np.isnan(pivot[1:3])) and np.all(np.isfinite(G[:, :, [0, 3]]))
    G1, _, status1 = TR.gains(Phi, 1.0, (1.0, 1.0))
    assert list(status1) == [0, 2, 0, 0] and np.all(G1[:, :, 2] == 0.0)      # B = 0 with q > 0: N = 0, no burn


# ------------------------------------------------------------------------------------- 3. the spreads behind the device's bounds
def test_stm_spread_is_a_tenth_of_the_gpu_bounds(orbits):
    ks, taus = [0, 1], (0.0,) + TR.TAUS3
    a = TR.stms(orbits, ks, taus, TR.HORIZONS, MU)
    b = TR.stms(orbits, ks, taus, TR.HORIZONS, MU, *TR.LOOSE)
    dx, dxt = np.abs(a.X - b.X).max(), np.abs(a.X_tgt - b.X_tgt).max()
    dphi = rel_block(b.Phi, a.Phi)
    Ga, Gb = TR.gains(a.Phi, TR.Q, (1.0, 1.0))[0], TR.gains(b.Phi, TR.Q, (1.0, 1.0))[0]
    dg = np.abs(Ga - Gb).max() / np.abs(Ga).max()
    print("spread between the tolerances: X %.2e, X_tgt %.2e, Phi %.2e (relative), G %.2e (relative)" % (dx, dxt, dphi, dg))
    assert dx <= 0.1 * GPU_X and dxt <= 0.1 * GPU_X_TGT and dphi <= 0.1 * GPU_PHI and dg <= 0.1 * GPU_G


def test_rk4_spread_is_a_tenth_of_the_gpu_bounds(orbits):
    """RK4 with 400 steps per span against DOP853 at 1e-13, in the reference."""
    a = TR.stms(orbits, [0, 1], TR.TAUS3, TR.HORIZONS, MU)
    b = TR.stms(orbits, [0, 1], TR.TAUS3, TR.HORIZONS, MU, rk4_steps=RK4_STEPS)
    dx, dxt = np.abs(a.X - b.X).max(), np.abs(a.X_tgt - b.X_tgt).max()
    dphi = rel_block(b.Phi, a.Phi)
    print("RK4 x %d against DOP853: X %.2e, X_tgt %.2e, Phi %.2e (relative)" % (RK4_STEPS, dx, dxt, dphi))
    assert dx <= 0.1 * GPU_RK4_X and dxt <= 0.1 * GPU_RK4_X_TGT and dphi <= 0.1 * GPU_RK4_PHI


def _spread(name, c, bounds):
    a = SR.fly(("target", name, "tight"), c, MU)
    b = SR.fly(("target", name, "loose"), c, MU, rtol=TR.LOOSE[0], atol=TR.LOOSE[1])
    d = dict(x=np.abs(a.x_final - b.x_final).max(), dev_r=np.nanmax(np.abs(a.dev[0] - b.dev[0])),
             dev_v=np.nanmax(np.abs(a.dev[1] - b.dev[1])), hist=np.nanmax(np.abs(a.dv_hist - b.dv_hist)),
             total=np.abs(a.dv_total - b.dv_total).max(), dev_final=np.abs(a.dev_final - b.dev_final).max())
    print("%-28s " % name + " ".join("%s %.2e" % kv for kv in d.items()))
    assert np.array_equal(a.n_burn, b.n_burn) and np.array_equal(a.status, b.status) and np.all(a.status == 0)
    for k, v in d.items():
        assert v <= 0.1 * bounds[k], (name, k, v)


@pytest.mark.parametrize("per_run", [False, True])
def test_flight_spread_is_a_tenth_of_the_gpu_bounds(orbits, per_run):
    """3 runs x 3 uneven phases x 2 revolutions under the target-point law, nav and exe given: the flights of the GPU test."""
    _spread("target-point %d" % per_run, TR.case(orbits, MU, 3, 2, True, per_run), GPU_TARGET)


# ------------------------------------------------------------------------------------------------ 4. the vetted Monte Carlo
def test_monte_carlo_is_vetted(orbits):
    """tests/golden/stationkeep_target_mc.json (gen_stationkeep_target_mc.py): under the reference's target-point law no run is
    lost and the largest deviation stays a factor MC_MARGIN below r_lost, so that no run of the device's can be near the threshold;
    without a law every run is lost; the spread of the reference between its tolerances is a tenth of the Monte Carlo's bounds.
    One run of each kind is flown again here to check that the file belongs to this reference and these draws."""
    g = monte_carlo_golden()
    m = MONTE_CARLO
    assert g["monte_carlo"] == m
    n_upd = 4 * m["n_rev"]
    law, loose, free = g["law"], g["loose"], g["free"]
    worst = max(law["dev_r_max"]) * KM
    dv_year = np.array(law["dv_total"]) * MS / (m["n_rev"] * orbits[0][1] * TU / 86400.0 / 365.25)
    print("target-point law, reference: largest deviation %.2f km, dv per year %.2f (median) %.2f (max) m/s; without a law lost at %s"
          % (worst, np.median(dv_year), dv_year.max(), free["lost_at"]))
    assert all(s == 0 for s in law["status"]) and all(n == n_upd for n in law["n_burn"])
    assert worst * MC_MARGIN <= m["r_lost_km"]
    assert all(s == 1 for s in free["status"]) and all(0 < u < n_upd for u in free["lost_at"])
    assert loose["status"] == law["status"] and loose["n_burn"] == law["n_burn"]
    spread = dict(total=np.abs(np.array(law["dv_total"]) - np.array(loose["dv_total"])).max(),
                  x=np.abs(np.array(law["x_final"]) - np.array(loose["x_final"])).max(),
                  dev_final=np.abs(np.array(law["dev_final"]) - np.array(loose["dev_final"])).max())
    print("spread between the tolerances over 20 revolutions: " + " ".join("%s %.2e" % kv for kv in spread.items()))
    for k, v in spread.items():
        assert v <= 0.1 * GPU_TARGET_MC[k], (k, v)
    L = TR.law(orbits, 0, TR.TAUS4, MU)
    inj, nav, exe = drivers.stationkeep_draws(m["n_runs"], n_upd, m["inj_sigma_r_km"], m["inj_sigma_v_ms"], m["nav_sigma_r_km"],
                                              m["nav_sigma_v_ms"], m["exe_sigma_frac"], m["exe_sigma_ms"], m["seed"], DU, TU)
    b = 5
    r = SR.flight(MU, L.X_ref, L.dt, L.G, L.X_ref[:, 0] + inj[:, b], 2, nav[:, :8, b], exe[:, :8, b], r_lost=m["r_lost_km"] / KM)
    assert r.status == 0 and np.nanmax(r.dev[0]) <= law["dev_r_max"][b]
    r0 = SR.flight(MU, L.X_ref, L.dt, 0.0 * L.G, L.X_ref[:, 0] + inj[:, b], m["n_rev"], nav[:, :, b], exe[:, :, b],
                   r_lost=m["r_lost_km"] / KM)
    assert r0.status == 1 and r0.lost_at == free["lost_at"][b]


# ------------------------------------------------------------------------------------------------------------ 5. the Python layer
def test_hotpath_rejects_malformed_input_before_any_library_call(monkeypatch):
    monkeypatch.setattr(hotpath, "default_context", lambda: pytest.fail("the library was reached"))
    s0, per, tau, hz = np.zeros(6), 3.0, [0.0, 0.5], [0.5, 1.0]
    cases = [dict(state0=np.zeros(5)), dict(state0=np.zeros((6, 0))), dict(state0=np.zeros((6, 2)), period=np.ones(3)), dict(tau=[]),
             dict(tau=[0.1, np.nan]), dict(tau=[np.inf]), dict(horizons=[]), dict(horizons=[0.0, 1.0]), dict(horizons=[-0.5]),
             dict(horizons=[0.5, 0.5]), dict(horizons=[1.0, 0.5]), dict(horizons=[0.5, np.inf]), dict(horizons=[np.nan]),
             dict(MU=0.0), dict(MU=1.0), dict(integ=lto.integrator(lto.RKF78_ADAPTIVE)), dict(integ=lto.integrator(lto.RK4, steps=0)),
             dict(state0=np.zeros((6, 1 << 14)), tau=np.zeros(1 << 12), horizons=[0.5, 1.0])]
    for kw in cases:
        a = dict(state0=s0, period=per, tau=tau, horizons=hz)
        a.update(kw)
        with pytest.raises(ValueError):
            hotpath.halo_stm(**a)
    Phi = np.zeros((6, 6, 2, 3))
    for bad in (np.zeros((6, 6)), np.zeros((6, 5, 2, 3)), np.zeros((6, 6, 0, 3)), np.zeros((6, 6, 2, 3, 1, 1))):
        with pytest.raises(ValueError):
            hotpath.stationkeep_target_gains(bad)
    for kw in (dict(q=-1e-3), dict(q=np.inf), dict(q=np.nan), dict(r=[1.0]), dict(r=[1.0, -1.0]), dict(r=[0.0, 0.0]), dict(r=[1.0, np.nan]),
               dict(r=[1.0, np.inf]), dict(sing_tol=-1e-3), dict(sing_tol=1.0), dict(sing_tol=np.nan)):
        with pytest.raises(ValueError):
            hotpath.stationkeep_target_gains(Phi, **kw)


def test_driver_with_stubbed_calls(monkeypatch):
    """drivers.target_point_gains: two calls, the phases as wrapped, the spans of stationkeep_spans, a StationGains that
    drivers.stationkeep takes; a status other than 0 raises."""
    calls = []
    rng = np.random.RandomState(8)
    X, G = rng.standard_normal((6, 3)), rng.standard_normal((3, 6, 3))

    def stm(state0, period, tau, horizons, MU=None, integ=None, ctx=None):
        calls.append("stm")
        t = np.asarray(tau, dtype=float)
        st = np.zeros(3, dtype=np.int32)
        st[1] = 2 if period < 0 else 0
        return hotpath.HaloStm(X, np.zeros((6, 6, len(horizons), 3)), None, t - np.floor(t), np.asarray(horizons), None, None, st)

    def tg(Phi, q, r, sing_tol, ctx=None):
        calls.append(("gains", Phi.shape, q, r, sing_tol))
        return hotpath.StationkeepTargetGains(G, np.ones(3), np.array([0, 0, 3 if q == 0.0 else 0], dtype=np.int32))

    monkeypatch.setattr(hotpath, "halo_stm", stm)
    monkeypatch.setattr(hotpath, "stationkeep_target_gains", tg)
    orbit = (np.zeros(6), 2.0, np.eye(6))
    g = drivers.target_point_gains(orbit, taus=[1.1, 0.35, -0.2], horizons=(0.25, 0.5, 1.5), q=0.5, weights=(1.0, 2.0, 3.0))
    assert calls == ["stm", ("gains", (6, 6, 3, 3), 0.5, (1.0, 2.0, 3.0), 1e-12)]
    assert isinstance(g, drivers.StationGains) and g.W is None and g.alpha is None and g.lam is None
    assert np.allclose(g.tau, [0.1, 0.35, 0.8]) and np.array_equal(g.dt, drivers.stationkeep_spans(g.tau, 2.0))
    assert np.array_equal(g.X_ref, X) and g.G is G
    with pytest.raises(ValueError):
        drivers.target_point_gains((np.zeros(6), -2.0, np.eye(6)), taus=[0.1, 0.35, 0.8])
    with pytest.raises(ValueError):
        drivers.target_point_gains(orbit, taus=[0.1, 0.35, 0.8], q=0.0)
    with pytest.raises(ValueError):
        drivers.target_point_gains(orbit, n_man=0)


def test_library_exports_both_entry_points_and_keeps_its_version():
    lib = lto.load_library()
    assert hasattr(lib, "lto_halo_stm_batch") and hasattr(lib, "lto_stationkeep_target_gains_batch")
    assert lib.lto_version() == 102
