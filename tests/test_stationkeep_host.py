"""CPU checks for the station-keeping calls: the identity behind the Floquet-mode law, the independent reference
(tests/stationkeep_reference.py) against itself at a looser tolerance -- for every quantity the GPU tests
(tests/test_stationkeep_gpu.py) compare, its own spread between (rtol, atol) = (1e-13, 1e-14) and (1e-12, 1e-13) has to stay below
a tenth of the bound the device is held to, each bound being ten times the spread seen, rounded up to a power of ten -- the vetting
of the threshold cases, the drivers' bookkeeping with a stubbed flight, and the library's symbols.

Three classes of flight, because the feedback decides how far a difference is amplified: LAW (the Floquet-mode law: the amplified
part of any difference is removed at every burn), FREE (no law, a law that is not ours, or a law held back by the dead band and the
clip: differences grow with the unstable mode) and RK4 (400 steps per span against DOP853: the truncation error of the fixed-step
method, which device and host share)."""
import os
import sys

import numpy as np
import pytest
from scipy.integrate import solve_ivp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import manifold_reference as MR  # noqa: E402
import stationkeep_reference as SR  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, hotpath, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU, day  # noqa: E402

# ---- the bounds of tests/test_stationkeep_gpu.py, absolute, in DU and DU/TU: (x_final, dev_r, dev_v, dv_hist, dv_total, dev_final)
GPU_LAW = dict(x=1e-10, dev_r=1e-11, dev_v=1e-10, hist=1e-11, total=1e-11, dev_final=1e-10)    # spread 3.4e-12 4.9e-13 1.2e-12 3.8e-13 8.0e-13 3.6e-12
GPU_FREE = dict(x=1e-9, dev_r=1e-10, dev_v=1e-9, hist=1e-10, total=1e-10, dev_final=1e-9)      # spread 5.1e-11 7.0e-12 1.9e-11 1.8e-12 2.3e-12 6.7e-11
GPU_RK4 = dict(x=1e-8, dev_r=1e-8, dev_v=1e-8, hist=1e-8, total=1e-8, dev_final=1e-8)          # spread 8.0e-10 1.7e-10 2.7e-10 1.5e-10 1.5e-10 9.1e-10
RK4_STEPS = 400
RANDOM_GAIN = 0.02

# ---- the vetted threshold cases (test_threshold_cases_are_vetted): no commanded |c| within a factor 2 of DV_MIN or DV_MAX, no |d_r|
# within a factor 2 of R_LOST, in the reference
THRESHOLD_SEED, THRESHOLD_SCALES, DV_MIN, DV_MAX = 1, (1e-4, 1.0, 1e2), 2.2e-7, 1.4e-4
LOST_SEED, R_LOST = 2, 4.9e-4

# ---- the Monte Carlo of the drivers' GPU test (test_monte_carlo_draws_are_vetted: without a law the reference loses every run)
MONTE_CARLO = dict(n_rev=3, n_runs=64, inj_sigma_r_km=10.0, inj_sigma_v_ms=0.1, nav_sigma_r_km=0.3, nav_sigma_v_ms=0.003,
                   exe_sigma_frac=0.01, exe_sigma_ms=1e-4, r_lost_km=5000.0, seed=3)

KM, MS = DU, DU / TU * 1e3


@pytest.fixture(scope="module")
def orbits():
    return MR.packaged_orbits(synth.halo_orbits(), MU)


def threshold_case(orbits):
    return SR.case(orbits, MU, 3, 3, 1, True, False, seed=THRESHOLD_SEED, scales=THRESHOLD_SCALES)


def lost_case(orbits):
    c = SR.case(orbits, MU, 3, 3, 2, False, False, seed=LOST_SEED)
    return c._replace(G=np.zeros_like(c.G))


def test_S_is_conserved_by_the_variational_flow():
    """A^T S + S A = 0 at random states: Phi^T S Phi = S for every state-transition matrix."""
    rng = np.random.RandomState(3)
    for _ in range(20):
        x = np.concatenate([rng.uniform(-1.5, 1.5, 3), rng.uniform(-1.0, 1.0, 3)])
        A = SR.variational_matrix(x, MU)
        r = np.abs(A.T @ SR.S + SR.S @ A).max()
        assert r <= 4.0 * np.finfo(float).eps * np.abs(A).max()


def _stm(state0, span, MU):
    Phi = np.empty((6, 6))
    for c in range(6):
        w = np.concatenate([state0, np.eye(6)[c]])
        if span > 0.0:
            w = solve_ivp(MR.rhs12(MU), (0.0, span), w, method="DOP853", rtol=MR.RTOL, atol=MR.ATOL).y[:, -1]
        Phi[:, c] = w[6:]
    return Phi


@pytest.mark.parametrize("k", [0, 1])
def test_S_v_s_is_a_left_eigenvector_of_the_monodromy_matrix_at_every_phase(orbits, k):
    """w = S v_s(tau) against M(tau) = Phi(tau) M Phi(tau)^-1, lambda_u and v_s(0) from the 50-digit solve of M.  The residual is
    that of M (5e-11 at phase 0) times what the similarity transform adds."""
    s, P, M = orbits[k]
    e = MR.eig_pair(M)
    L = SR.law(orbits, k, SR.TAUS3, MU)
    worst = 0.0
    for tau, V in [(0.0, np.stack([e.v_u, e.v_s], axis=1))] + [(t, L.V[:, :, j]) for j, t in enumerate(SR.TAUS3)]:
        Phi = _stm(s, tau * P, MU)
        Mt = Phi @ M @ np.linalg.inv(Phi)
        w = SR.S @ V[:, 1]
        res = np.abs(w @ Mt - e.lam_u * w).max() / np.abs(w).max() / abs(e.lam_u)
        print("orbit %d, phase %.2f: |w^T M - lambda_u w^T| / (lambda_u max |w|) = %.2e, w . v_u = %.3f" % (k + 1, tau, res, w @ V[:, 0]))
        worst = max(worst, res)
    assert worst < 1e-8


def test_the_law_zeroes_the_unstable_component(orbits):
    """W . (dx + (0, G dx)) = 0 to round-off for random dx, W . v_u = 1, and G dx is the shortest such velocity change."""
    rng = np.random.RandomState(4)
    for k in (0, 1):
        L = SR.law(orbits, k, SR.TAUS3, MU)
        for j in range(3):
            W, G = L.W[:, j], L.G[:, :, j]
            assert abs(W @ L.V[:, 0, j] - 1.0) < 1e-14
            for _ in range(10):
                dx = rng.standard_normal(6)
                dv = G @ dx
                after = dx + np.concatenate([np.zeros(3), dv])
                assert abs(W @ after) <= 1e-13 * np.abs(W).max() * np.abs(dx).max()
                assert abs(np.linalg.norm(dv) - abs(W @ dx) / np.linalg.norm(W[3:])) <= 1e-12 * np.linalg.norm(dv)


def test_controlled_against_uncontrolled(orbits):
    """Packaged orbit 1, four burns per revolution, 1 km and 1 cm/s off (along (1, 1, 1) in both).  Measured: controlled, six
    revolutions: largest deviation 20.2 km, 5.3 mm/s in all; with the navigation errors of SR.draws(seed 5) 98.3 km and 0.279 m/s;
    uncontrolled 149 km after one revolution, 6 745 km after two.  Margins: a factor 3."""
    L = SR.law(orbits, 0, (0.0, 0.25, 0.5, 0.75), MU)
    inj = np.array([1.0 / KM / np.sqrt(3.0)] * 3 + [0.01 / MS / np.sqrt(3.0)] * 3)
    x0 = L.X_ref[:, 0] + inj
    r = SR.flight(MU, L.X_ref, L.dt, L.G, x0, 6)
    print("controlled: largest deviation %.1f km, %.2f mm/s in %d burns" % (r.dev[0].max() * KM, r.dv_total * MS * 1e3, r.n_burn))
    assert r.status == 0 and r.n_burn == 24
    assert r.dev[0].max() * KM < 3.0 * 20.2 and r.dv_total * MS < 3.0 * 5.3e-3
    _, nav, _ = SR.draws(1, 24, 5)
    rn = SR.flight(MU, L.X_ref, L.dt, L.G, x0, 6, nav=nav[:, :, 0])
    print("with navigation errors: largest deviation %.1f km, %.3f m/s" % (rn.dev[0].max() * KM, rn.dv_total * MS))
    assert rn.dev[0].max() * KM < 3.0 * 98.3 and rn.dv_total * MS < 3.0 * 0.279
    r0 = SR.flight(MU, L.X_ref, L.dt, 0.0 * L.G, x0, 3)
    print("uncontrolled: %.0f km after one revolution, %.0f km after two" % (r0.dev[0, 4] * KM, r0.dev[0, 8] * KM))
    assert r0.dev[0, 4] * KM > 149.0 / 3.0 and r0.dev[0, 8] * KM > 6745.0 / 3.0
    assert r0.n_burn == 12 and r0.dv_total == 0.0           # a zero command is a burn of zero size when there is no dead band


def _spread(name, c, bounds, loose=None, **kw):
    a = SR.fly((name, "tight"), c, MU, **kw)
    b = SR.fly((name, "other"), c, MU, **(loose if loose is not None else dict(rtol=SR.LOOSE[0], atol=SR.LOOSE[1], **kw)))
    d = dict(x=np.abs(a.x_final - b.x_final).max(), dev_r=np.nanmax(np.abs(a.dev[0] - b.dev[0])),
             dev_v=np.nanmax(np.abs(a.dev[1] - b.dev[1])), hist=np.nanmax(np.abs(a.dv_hist - b.dv_hist)),
             total=np.abs(a.dv_total - b.dv_total).max(), dev_final=np.abs(a.dev_final - b.dev_final).max())
    print("%-28s " % name + " ".join("%s %.2e" % kv for kv in d.items()))
    assert np.array_equal(a.n_burn, b.n_burn) and np.array_equal(a.status, b.status) and np.array_equal(a.lost_at, b.lost_at)
    assert np.array_equal(np.isnan(a.dev), np.isnan(b.dev)) and np.array_equal(np.isnan(a.dv_hist), np.isnan(b.dv_hist))
    for k, v in d.items():
        assert v <= 0.1 * bounds[k], (name, k, v)


@pytest.mark.parametrize("per_run", [False, True])
@pytest.mark.parametrize("errors", [False, True])
def test_law_spread_is_a_tenth_of_the_gpu_bounds(orbits, per_run, errors):
    _spread("law %d %d" % (per_run, errors), SR.case(orbits, MU, 8, 3, 2, errors, per_run), GPU_LAW)


def test_one_burn_spread_is_a_tenth_of_the_gpu_bounds(orbits):
    _spread("law, one burn", SR.case(orbits, MU, 8, 1, 2, True, True), GPU_LAW)


def test_free_spread_is_a_tenth_of_the_gpu_bounds(orbits):
    c = SR.case(orbits, MU, 8, 3, 2, True, True)
    _spread("no law", c._replace(G=np.zeros_like(c.G)), GPU_FREE)
    _spread("random law", SR.case(orbits, MU, 8, 3, 2, True, True, random_gain=RANDOM_GAIN), GPU_FREE)
    _spread("thresholds", threshold_case(orbits), GPU_FREE, dv_min=DV_MIN, dv_max=DV_MAX)
    _spread("lost", lost_case(orbits), GPU_FREE, r_lost=R_LOST)


@pytest.mark.parametrize("per_run", [False, True])
def test_rk4_spread_is_a_tenth_of_the_gpu_bounds(orbits, per_run):
    """RK4 with 400 steps per span against DOP853 at 1e-13, in the reference."""
    _spread("rk4 %d" % per_run, SR.case(orbits, MU, 3, 3, 2, True, per_run), GPU_RK4, loose=dict(rk4_steps=RK4_STEPS))


def test_threshold_cases_are_vetted(orbits):
    """No commanded |c| within a factor 2 of DV_MIN or DV_MAX and no |d_r| within a factor 2 of R_LOST, so that no threshold can flip
    between host and device; at least one burn skipped, one clipped, one neither; every uncontrolled run lost, not all at once."""
    def clear(vals, thr):
        v = vals[np.isfinite(vals)]
        return bool(np.all((v < 0.5 * thr) | (v > 2.0 * thr)))
    r = SR.fly(("thresholds", "tight"), threshold_case(orbits), MU, dv_min=DV_MIN, dv_max=DV_MAX)
    print("commanded |c|:\n%s\napplied:\n%s" % (r.cmd.T, r.dv_hist.T))
    assert clear(r.cmd, DV_MIN) and clear(r.cmd, DV_MAX)
    skipped, clipped = r.cmd < DV_MIN, r.cmd > DV_MAX
    assert skipped.any() and clipped.any() and (~skipped & ~clipped).any()
    assert np.all(r.dv_hist[skipped] == 0.0) and np.array_equal(r.n_burn, (~skipped).sum(axis=0))
    assert np.all(r.status == 0)
    lost = SR.fly(("lost", "tight"), lost_case(orbits), MU, r_lost=R_LOST)
    print("uncontrolled |d_r|:\n%s\nlost at %s" % (lost.dev[0].T, lost.lost_at))
    assert clear(lost.dev[0], R_LOST)
    assert np.all(lost.status == 1) and len(set(lost.lost_at.tolist())) > 1 and np.all(lost.lost_at > 0)
    for b, u in enumerate(lost.lost_at):
        assert np.all(np.isfinite(lost.dev[:, :u + 1, b])) and np.all(np.isnan(lost.dev[:, u + 1:, b]))
        assert np.all(np.isfinite(lost.dv_hist[:u, b])) and np.all(np.isnan(lost.dv_hist[u:, b]))


def test_monte_carlo_draws_are_vetted(orbits):
    """The uncontrolled runs of MONTE_CARLO are all lost within three revolutions: a run leaves the orbit as fast as its injection
    error has a component along the unstable mode, W . dx.  The three runs with the smallest component are flown by the reference
    without a law and are lost at least two updates before the end (measured: all three at update 8 of 12, the component 17 to 21
    km against a median of 388 km), so no run of the draws can stay."""
    m = MONTE_CARLO
    L = SR.law(orbits, 0, (0.0, 0.25, 0.5, 0.75), MU)
    inj, nav, exe = drivers.stationkeep_draws(m["n_runs"], 4 * m["n_rev"], m["inj_sigma_r_km"], m["inj_sigma_v_ms"], m["nav_sigma_r_km"],
                                              m["nav_sigma_v_ms"], m["exe_sigma_frac"], m["exe_sigma_ms"], m["seed"], DU, TU)
    comp = np.abs(L.W[:, 0] @ inj) * KM
    for b in np.argsort(comp)[:3]:
        r = SR.flight(MU, L.X_ref, L.dt, 0.0 * L.G, L.X_ref[:, 0] + inj[:, b], m["n_rev"], nav[:, :, b], exe[:, :, b],
                      r_lost=m["r_lost_km"] / KM)
        print("run %d: component %.1f km (median %.0f km), lost at update %d" % (b, comp[b], np.median(comp), r.lost_at))
        assert r.status == 1 and r.lost_at <= 4 * m["n_rev"] - 3


def test_spans_wrap_round():
    P = 2.5
    assert np.allclose(drivers.stationkeep_spans([0.1, 0.35, 0.8], P), [0.25 * P, 0.45 * P, 0.3 * P], rtol=1e-15, atol=0.0)
    assert np.array_equal(drivers.stationkeep_spans([0.4], P), [P])
    assert abs(drivers.stationkeep_spans(np.arange(4) / 4.0, P).sum() - P) < 1e-15
    assert np.array_equal(drivers.stationkeep_spans([0.1, 0.35, 0.8], P), SR.spans([0.1, 0.35, 0.8], P))
    for bad in ([0.5, 0.2], [0.2, 0.2], [1.0], [-0.1, 0.3], [np.nan]):
        with pytest.raises(ValueError):
            drivers.stationkeep_spans(bad, P)


def test_draws_are_reproducible_and_in_units():
    inj, nav, exe = drivers.stationkeep_draws(2000, 3, 2.0, 0.05, 0.3, 0.003, 0.01, 0.001, 7, DU, TU)
    inj2, nav2, exe2 = drivers.stationkeep_draws(2000, 3, 2.0, 0.05, 0.3, 0.003, 0.01, 0.001, 7, DU, TU)
    assert np.array_equal(inj, inj2) and np.array_equal(nav, nav2) and np.array_equal(exe, exe2)
    assert inj.shape == (6, 2000) and nav.shape == (6, 3, 2000) and exe.shape == (4, 3, 2000)
    assert np.all(inj[:, 0] != 0.0)                                     # no nominal run: every run is disturbed
    for got, want in ((inj[:3].std() * KM, 2.0), (inj[3:].std() * MS, 0.05), (nav[:3].std() * KM, 0.3), (nav[3:].std() * MS, 0.003),
                      (exe[0].std(), 0.01), (exe[1:].std() * MS, 0.001)):
        assert abs(got / want - 1.0) < 0.05
    a, n0, x0 = drivers.stationkeep_draws(2000, 3, 2.0, 0.05, None, None, None, None, 7, DU, TU)
    assert n0 is None and x0 is None and np.array_equal(a, inj)          # a stream does not move when another sigma changes
    _, n1, _ = drivers.stationkeep_draws(2000, 3, 5.0, 0.05, 0.3, 0.003, None, None, 7, DU, TU)
    assert np.array_equal(n1, nav)


def test_driver_bookkeeping_with_a_stubbed_flight(monkeypatch):
    """Units, time flown, the per-year scaling, the lost share and the percentiles of drivers.stationkeep around a flight that is
    not flown."""
    n_man, n_rev, B = 3, 2, 5
    n_upd = n_man * n_rev
    rng = np.random.RandomState(9)
    g = drivers.StationGains(np.array([0.1, 0.35, 0.8]), rng.standard_normal((6, n_man)), np.array([0.5, 1.0, 0.75]),
                             rng.standard_normal((3, 6, n_man)), None, None, None)
    dv_total = np.array([1e-5, 2e-5, 3e-5, 4e-5, 5e-5])
    status = np.array([0, 0, 1, 0, 0], dtype=np.int32)
    lost_at = np.array([-1, -1, 4, -1, -1], dtype=np.int32)
    dev = np.abs(rng.standard_normal((2, n_upd, B))) * 1e-5
    dev[:, 5:, 2] = np.nan
    seen = {}

    def stub(X_ref, dt, G, x0, n_rev_, nav=None, exe=None, dv_min=0.0, dv_max=0.0, r_lost=0.0, MU=None, integ=None, ctx=None):
        seen.update(X_ref=X_ref, dt=dt, G=G, x0=x0, n_rev=n_rev_, nav=nav, exe=exe, dv_min=dv_min, dv_max=dv_max, r_lost=r_lost)
        return hotpath.StationkeepFlight(np.zeros((6, B)), dv_total, np.full(B, n_upd, dtype=np.int32), dev, np.zeros((n_upd, B)),
                                         np.ones((2, B)) * 1e-6, None, None, status, lost_at)

    monkeypatch.setattr(hotpath, "stationkeep_flight", stub)
    out = drivers.stationkeep(None, n_rev, B, 2.0, 0.05, nav_sigma_r_km=0.3, nav_sigma_v_ms=0.003, dv_min_ms=0.01, dv_max_ms=2.0,
                              r_lost_km=5000.0, seed=3, gains=g)
    inj, nav, exe = drivers.stationkeep_draws(B, n_upd, 2.0, 0.05, 0.3, 0.003, None, None, 3, DU, TU)
    assert np.array_equal(seen["x0"], g.X_ref[:, :1] + inj) and np.array_equal(seen["nav"], nav) and seen["exe"] is None and exe is None
    assert seen["n_rev"] == n_rev and seen["G"] is g.G
    assert abs(seen["dv_min"] * MS - 0.01) < 1e-15 and abs(seen["dv_max"] * MS - 2.0) < 1e-12 and abs(seen["r_lost"] * KM - 5000.0) < 1e-9
    full = 2.0 * 2.25 * TU / day
    t_days = np.array([full, full, (2.25 + 0.5) * TU / day, full, full])       # lost at update 4: one revolution and one span
    assert np.allclose(out["t_days"], t_days, rtol=1e-15)
    assert np.allclose(out["dv_ms"], dv_total * MS, rtol=1e-15)
    assert np.allclose(out["dv_per_year_ms"], dv_total * MS / t_days * 365.25, rtol=1e-14)
    assert out["lost_share"] == 0.2
    assert np.allclose(out["dev_r_km"][:, 0], dev[0, :, 0] * KM) and np.allclose(out["dev_v_ms"][:, 1], dev[1, :, 1] * MS)
    ok = status == 0
    for q in (50, 95, 99):
        assert out["percentiles"]["dv_ms"][q] == float(np.percentile(out["dv_ms"][ok], q))
        assert out["percentiles"]["dv_per_year_ms"][q] == float(np.percentile(out["dv_per_year_ms"][ok], q))
        assert out["percentiles"]["dev_r_km"][q] == float(np.percentile(np.max(dev[0] * KM, axis=0)[ok], q))


def test_hotpath_rejects_malformed_input_before_any_library_call(monkeypatch):
    monkeypatch.setattr(hotpath, "default_context", lambda: pytest.fail("the library was reached"))
    V = np.zeros((6, 2, 3))
    for bad in (np.zeros((6, 3)), np.zeros((5, 2, 3)), np.zeros((6, 2, 0))):
        with pytest.raises(ValueError):
            hotpath.stationkeep_gains(bad)
    for tol in (-1e-3, 1.0, np.nan):
        with pytest.raises(ValueError):
            hotpath.stationkeep_gains(V, sing_tol=tol)
    X, T, G, x0 = np.zeros((6, 3)), np.ones(3), np.zeros((3, 6, 3)), np.zeros((6, 4))
    cases = [dict(X_ref=np.zeros((5, 3))), dict(dt=np.ones(2)), dict(dt=np.array([1.0, 0.0, 1.0])), dict(dt=np.array([1.0, np.inf, 1.0])),
             dict(G=np.zeros((3, 6, 2))), dict(x0=np.zeros((5, 4))), dict(n_rev=0), dict(nav=np.zeros((6, 5, 4))),
             dict(exe=np.zeros((3, 6, 4))), dict(dv_min=-1.0), dict(dv_max=np.inf), dict(r_lost=np.nan),
             dict(X_ref=np.zeros((6, 3, 2)), dt=np.ones((3, 2)), G=np.zeros((3, 6, 3, 2))),
             dict(integ=lto.integrator(lto.RKF78_ADAPTIVE)), dict(integ=lto.integrator(lto.RK4, steps=0))]
    for kw in cases:
        a = dict(X_ref=X, dt=T, G=G, x0=x0, n_rev=2)
        a.update(kw)
        with pytest.raises(ValueError):
            hotpath.stationkeep_flight(**a)


def test_library_exports_both_entry_points_and_keeps_its_version():
    lib = lto.load_library()
    assert hasattr(lib, "lto_stationkeep_gains_batch") and hasattr(lib, "lto_stationkeep_flight_batch")
    assert lib.lto_version() == 102
