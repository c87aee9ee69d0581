"""CPU: the guidance reference held to itself, and the host arithmetic of the guidance wrappers and drivers."""
import ctypes

import numpy as np
import pytest

import lowthrustopt_amd as lto
import guidance_reference as G
from lowthrustopt_amd import _lib, drivers, hotpath
from lowthrustopt_amd.constants import DU, TU

ENTRIES = ("lto_guidance_gains_batch", "lto_guidance_gains", "lto_guided_flight_batch", "lto_guided_flight")


@pytest.mark.parametrize("fx", G.REGULAR_FIX, ids=lambda f: "s%d_n%d_p%g%s" % (f.seed, f.n, f.p, "_back" if f.td < 0 else ""))
def test_recurrence_against_the_product_formula(fx):
    """The float64 recurrence against K_k = -Phi_xl(tf, tk)^-1 Phi_xx(tf, tk) from the longdouble product of the segment STMs,
    relative to max |K_k|: bar 1e-12 (measured <= 2.2e-14); every pivot ratio far above the default sing_tol."""
    Phi = G.fix_phi(fx)
    K64, piv = G.recurrence(Phi, np.float64)
    Kp = G.product_gains(Phi)
    rel = np.max(np.abs(K64 - Kp), axis=(0, 1)) / np.max(np.abs(Kp), axis=(0, 1))
    print("MEASURED recurrence vs product %s: %.2e, smallest pivot ratio %.2e" % (fx, float(rel.max()), piv.min()))
    assert float(rel.max()) < 1e-12
    assert piv.min() > 1e-3


@pytest.mark.parametrize("fx", G.SINGULAR_FIX, ids=lambda f: "s%d_p%g_rho%g" % (f.seed, f.p, f.rho))
def test_singular_fixtures_are_singular_on_the_last_segment(fx):
    _, piv = G.recurrence(G.fix_phi(fx), np.float64)
    print("MEASURED last-segment pivot ratio %s: %.2e" % (fx, piv[-1]))
    assert piv[-1] < 1e-13


def test_longdouble_solver_against_numpy():
    rng = np.random.default_rng(3)
    M, R = rng.standard_normal((6, 6)), rng.standard_normal((6, 6))
    X, ratio = G.lu_solve(M, R)
    assert np.max(np.abs(X.astype(np.float64) - np.linalg.solve(M, R))) < 1e-12
    assert 0.0 < ratio <= 1.0


def test_numpy_rhs_is_the_oracles():
    from oracle import oracle as O
    for fx in (G.P2_FIX[0], G.P1_FIX, G.P15_FIX, G.P0_FIX[0], G.BACK_FIX):
        XC, _ = G.fix_extremal(fx)
        prm = G.fix_prm(fx)
        for k in (0, fx.n - 1):
            d, um = G.rhs13(XC[:, k], prm)
            ref = O.rhs_state_costate(XC[:, k], np.array(prm))
            assert np.max(np.abs(d - ref)) <= 1e-13 * max(1.0, np.max(np.abs(ref)))
            assert um >= 0.0


@pytest.mark.parametrize("fx", G.P2_FIX + G.SMALL_FIX + (G.BACK_FIX,), ids=lambda f: "s%d_n%d%s" % (f.seed, f.n, "_back" if f.td < 0 else ""))
def test_guided_miss_is_second_order_in_the_start_error(fx):
    """One update at node 0 with the reference's own gains: halving the start error quarters the miss, ratios inside [3.8, 4.2];
    open loop (the nominal's first costate kept) it halves, ratios inside [1.8, 2.2]."""
    XC, t = G.fix_extremal(fx)
    K, prm = G.fix_gains(fx), G.fix_prm(fx)
    r1, r2, miss = G.miss_ratios(fx, lambda x0, every: G.fly(XC, t, K, x0, prm, every).x_final, fx.n)
    print("MEASURED guided miss ratios %s: %.3f %.3f (misses %s)" % (fx, r1, r2, miss))
    assert 3.8 < r1 < 4.2 and 3.8 < r2 < 4.2
    o1, o2, _ = G.miss_ratios(fx, lambda x0, every: G.fly(XC, t, K, x0, prm, every).x_final, 0)
    assert 1.8 < o1 < 2.2 and 1.8 < o2 < 2.2


def test_update_at_every_node_holds_the_arrival_state():
    """The 33-node, 4 TU extremal: a start error of 1e-4 misses by thousandths open loop and by far less than the start error with
    an update at every node."""
    fx = G.LONG_FIX
    XC, t = G.fix_extremal(fx)
    x0 = XC[:6, 0] + G.start_error(fx, 1e-4)
    open_loop = np.linalg.norm(G.fly(XC, t, G.fix_gains(fx), x0, G.fix_prm(fx), 0).x_final - XC[:6, -1])
    guided = np.linalg.norm(G.fly(XC, t, G.fix_gains(fx), x0, G.fix_prm(fx), 1).x_final - XC[:6, -1])
    print("MEASURED 4 TU fixture, start error 1e-4: open loop %.2e, update at every node %.2e" % (open_loop, guided))
    assert open_loop > 1e-4 and guided < 1e-9


def test_rk4_reference_float64_against_longdouble():
    fx = G.P2_FIX[0]
    XC, t = G.fix_extremal(fx)
    x0 = XC[:6, 0] + G.start_error(fx, 1e-3)
    lo = G.fly_rk4(XC, t, G.fix_gains(fx), x0, G.fix_prm(fx), 3, 2, dtype=np.float64)
    hi = G.fly_rk4(XC, t, G.fix_gains(fx), x0, G.fix_prm(fx), 3, 2, dtype=np.longdouble)
    assert float(np.max(np.abs(lo[0] - hi[0]))) < 1e-12 and abs(float(lo[1] - hi[1])) < 1e-12


def test_binding_table_and_library_export_the_four_entries():
    lib = ctypes.CDLL(lto.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert len(_lib.SIGNATURES["lto_guidance_gains_batch"][1]) == 14
    assert len(_lib.SIGNATURES["lto_guided_flight_batch"][1]) == 21
    for name in ("guidance_gains", "guided_flight", "GuidanceGains", "GuidedFlight", "guided_updates"):
        assert hasattr(lto, name)
    for name in ("neighbouring_gains", "fly_guided", "dispersion_guided", "guided_nav"):
        assert hasattr(drivers, name)


def test_update_counts():
    assert hotpath.guided_updates(9, 0) == 0
    assert hotpath.guided_updates(9, 1) == 8
    assert hotpath.guided_updates(9, 3) == 3          # nodes 0, 3, 6
    assert hotpath.guided_updates(9, 7) == 2          # nodes 0, 7
    assert hotpath.guided_updates(9, 8) == 1
    assert hotpath.guided_updates(9, 100) == 1
    assert hotpath.guided_updates(2, 1) == 1
    for n in (2, 3, 9, 30):
        for every in (1, 2, 3, 5, 29, 64):
            assert hotpath.guided_updates(n, every) == len([k for k in range(n - 1) if k % every == 0]) == G.n_updates(n, every)
    with pytest.raises(ValueError):
        hotpath.guided_updates(9, -1)


def test_wrapper_refuses_bad_shapes_without_a_device():
    XC, t = G.fix_extremal(G.P2_FIX[0])
    K, prm = G.fix_gains(G.P2_FIX[0]), G.fix_prm(G.P2_FIX[0])
    x0 = np.zeros((6, 3))
    with pytest.raises(ValueError):
        hotpath.guided_flight(XC, t, K, np.zeros((7, 3)), prm)
    with pytest.raises(ValueError):
        hotpath.guided_flight(np.repeat(XC[:, :, None], 2, axis=2), t, K, x0, prm)          # two nominals, three starts
    with pytest.raises(ValueError):
        hotpath.guided_flight(XC, t[:-1], K, x0, prm)
    with pytest.raises(ValueError):
        hotpath.guided_flight(XC, t, K[:, :, :-1], x0, prm)
    with pytest.raises(ValueError):
        hotpath.guided_flight(XC, t, K, x0, prm, update_every=3, nav=np.zeros((6, 2, 3)))  # three updates, two given
    with pytest.raises(ValueError):
        hotpath.guided_flight(XC, t, K, x0, prm, update_every=-1)
    with pytest.raises(ValueError):
        hotpath.guided_flight(XC, t, K, x0, [prm, prm])
    with pytest.raises(ValueError):
        drivers.fly_guided(None, np.zeros((14, 9)), t, prm)
    with pytest.raises(ValueError):
        drivers.fly_guided(None, XC, t[:-1], prm)
    with pytest.raises(ValueError):
        drivers.fly_guided(None, XC, t, prm, n_guid=1)
    with pytest.raises(ValueError):
        drivers.dispersion_guided(None, np.zeros((14, 9)), t, prm, 4, 1.0, 1.0, 0)
    with pytest.raises(ValueError):
        drivers.dispersion_guided(None, XC, t, prm, 4, 1.0, 1.0, 0, nav_sigma_r_km=1.0)


def test_dispersion_guided_draws_the_starts_of_dispersion(monkeypatch):
    """Both drivers get their starts from dispersion_starts with the same arguments, sample 0 undisturbed; the navigation errors
    have the units of the starts and none for sample 0."""
    XC, t = G.fix_extremal(G.P2_FIX[0])
    prm = G.fix_prm(G.P2_FIX[0])
    seen = {}

    def fake_fly_control(ctx, XC_all, t_TU, p, x0, *a, **k):
        seen["open"] = np.array(x0)
        B = x0.shape[1]
        return dict(status=np.zeros(B, dtype=np.int32), miss_r_km=np.zeros(B), miss_v_ms=np.zeros(B))

    def fake_fly_guided(ctx, XC_all, t_TU, p, x0, n_guid, update_every, nav, integ):
        seen["guided"], seen["nav"] = np.array(x0), nav
        B = x0.shape[1]
        return dict(status=np.zeros(B, dtype=np.int32), miss_r_km=np.zeros(B), miss_v_ms=np.zeros(B), dv_excess_ms=np.arange(B) * 1.0)
    monkeypatch.setattr(drivers, "fly_control", fake_fly_control)
    monkeypatch.setattr(drivers, "fly_guided", fake_fly_guided)
    a = drivers.dispersion(None, XC, t, prm, 17, 1.0, 0.01, 5)
    b = drivers.dispersion_guided(None, XC, t, prm, 17, 1.0, 0.01, 5, update_every=3, nav_sigma_r_km=0.5, nav_sigma_v_ms=0.02,
                                  nav_seed=9)
    assert np.array_equal(seen["open"], seen["guided"]) and np.array_equal(a["x0"], b["x0"])
    assert np.array_equal(b["x0"][:, 0], XC[:6, 0])
    assert np.array_equal(b["x0"], drivers.dispersion_starts(XC[:6, 0], 17, 1.0, 0.01, 5, DU, TU))
    nav = seen["nav"]
    assert nav.shape == (6, 3, 17) and not nav[:, :, 0].any()
    assert np.array_equal(nav, drivers.guided_nav(3, 17, 0.5, 0.02, 9, DU, TU))
    ref = np.random.default_rng(9).standard_normal((6, 3, 17))
    assert np.allclose(nav[0:3, :, 1:], ref[0:3, :, 1:] * 0.5 / DU, rtol=1e-15)
    assert np.allclose(nav[3:6, :, 1:], ref[3:6, :, 1:] * 0.02 / 1e3 * TU / DU, rtol=1e-15)
    assert sorted(b["percentiles"]) == ["dv_excess_ms", "miss_r_km", "miss_v_ms"]
    assert b["percentiles"]["dv_excess_ms"][50] == 8.0
    assert sorted(b["percentiles"]["miss_r_km"]) == [50, 95, 99]
