"""CPU: the 14-row guidance reference held to itself -- every fixture is admitted here before a device test leans on it -- and the
host arithmetic of the _mass guidance wrappers and drivers."""
import ctypes

import numpy as np
import pytest

import lowthrustopt_amd as lto
import guidance_reference as G
import guidance_mass_reference as GM
from lowthrustopt_amd import _lib, drivers, hotpath
from lowthrustopt_amd.constants import DU, TU

ENTRIES = ("lto_guidance_gains_mass_batch", "lto_guidance_gains_mass", "lto_guided_flight_mass_batch", "lto_guided_flight_mass")


@pytest.mark.parametrize("fx", GM.REGULAR_FIX, ids=GM.fix_id)
def test_recurrence_against_the_product_formula(fx):
    """The float64 recurrence against K_k = -Psi[P, 7:14]^-1 Psi[P, 0:7] from the longdouble product of the segment STMs, relative
    to max |K_k|: bar 1e-12 (measured <= 1.3e-14); every pivot ratio at least 100 sing_tol (measured >= 6.5e-5)."""
    Phi = GM.fix_phi(fx)
    K64, piv = GM.recurrence(Phi, np.float64)
    Kp = GM.product_gains(Phi)
    rel = np.max(np.abs(K64 - Kp), axis=(0, 1)) / np.max(np.abs(Kp), axis=(0, 1))
    print("MEASURED 14-row recurrence vs product %s: %.2e, smallest pivot ratio %.2e" % (GM.fix_id(fx), float(rel.max()), piv.min()))
    assert float(rel.max()) <= 1e-12
    assert piv.min() >= 100.0 * GM.SING_TOL


@pytest.mark.parametrize("fx", GM.SINGULAR_FIX, ids=GM.fix_id)
def test_singular_fixtures_are_singular_on_the_last_segment(fx):
    """p = 0, p = 1 with a sharp switch and a p = 3 law clamped throughout: the last segment's ratio is at most sing_tol / 100
    (measured 2.8e-15 .. 6.8e-13)."""
    _, piv = GM.recurrence(GM.fix_phi(fx), np.float64)
    print("MEASURED 14-row last-segment pivot ratio %s: %.2e" % (GM.fix_id(fx), piv[-1]))
    assert piv[-1] <= GM.SING_TOL / 100.0


def test_dip_fixture_has_its_smallest_ratio_at_an_inner_node():
    """DIP_FIX's ratio at DIP_NODE is below 0.8 x every later node's and 0.8 x every node's of DIP_NEIGHBOUR (measured 0.035 against
    0.049 and 0.065): room for a sing_tol between them."""
    piv = GM.recurrence(GM.fix_phi(GM.DIP_FIX), np.float64)[1]
    nb = GM.recurrence(GM.fix_phi(GM.DIP_NEIGHBOUR), np.float64)[1]
    k = GM.DIP_NODE
    print("MEASURED dip fixture: ratio %.3e at node %d, later nodes >= %.3e, neighbour >= %.3e" % (piv[k], k, piv[k + 1:].min(), nb.min()))
    assert piv[k] < 0.8 * min(piv[k + 1:].min(), nb.min()) and piv[k] >= 100.0 * GM.SING_TOL


def test_last_segment_rule_takes_row_6_from_d_and_c():
    """One segment: K = -M^-1 N holds the rows P = {0..5, 13} of Phi [I; K] at zero."""
    Phi = GM.fix_phi(GM.SMALL_FIX[0])
    K, _ = GM.recurrence(Phi, np.longdouble)
    dy = np.asarray(Phi[:, :, 0], dtype=np.longdouble) @ np.vstack([np.eye(7, dtype=np.longdouble), K[:, :, 0]])
    assert float(np.max(np.abs(dy[GM.P_ROWS]))) < 1e-14 * float(np.max(np.abs(dy)))
    assert float(np.max(np.abs(dy[6]))) > 1e-3                                # the final mass is free


def test_numpy_rhs_is_the_oracles():
    from oracle import oracle as O
    for fx in (GM.P2_FIX[0], GM.P1_FIX, GM.P15_FIX, GM.P0_FIX[0], GM.BACK_FIX, GM.CLAMP3_FIX):
        XC, _ = GM.fix_extremal(fx)
        prm = GM.fix_prm(fx)
        for k in (0, XC.shape[1] - 1):
            d, um = GM.rhs15(XC[:, k], prm)
            ref = O.rhs_state_costate_mass(XC[:, k], np.array(prm))
            assert np.max(np.abs(d - ref)) <= 1e-13 * max(1.0, np.max(np.abs(ref))), (fx, k)
            assert um >= 0.0 and abs(um - GM.umag14(XC[:, k], prm)) <= 1e-15 * max(1.0, um)


@pytest.mark.parametrize("fx", GM.NINE_P2, ids=GM.fix_id)
def test_guided_miss_is_second_order_in_the_start_error(fx):
    """One update at node 0 with the reference's own gains: halving the start error (mass error included) quarters the (r, v) miss,
    ratios inside [3.8, 4.2]; open loop it halves, ratios inside [1.8, 2.2]."""
    XC, t = GM.fix_extremal(fx)
    K, prm = GM.fix_gains(fx), GM.fix_prm(fx)
    r1, r2, miss = GM.miss_ratios(fx, lambda x0, every: GM.fly(XC, t, K, x0, prm, every).x_final, fx.n)
    print("MEASURED 14-row guided miss ratios %s: %.3f %.3f (misses %s)" % (GM.fix_id(fx), r1, r2, miss))
    assert 3.8 < r1 < 4.2 and 3.8 < r2 < 4.2
    o1, o2, _ = GM.miss_ratios(fx, lambda x0, every: GM.fly(XC, t, K, x0, prm, every).x_final, 0)
    print("MEASURED 14-row open-loop miss ratios %s: %.3f %.3f" % (GM.fix_id(fx), o1, o2))
    assert 1.8 < o1 < 2.2 and 1.8 < o2 < 2.2


@pytest.mark.parametrize("fx", (GM.P2_FIX[0], GM.P1_FIX, GM.P15_FIX), ids=GM.fix_id)
def test_isp_infinity_reduces_to_the_12_row_gains(fx):
    """Isp = 1e30: the mass stays where it is, bit for bit, and K[0:6, 0:6] is the 12-row gain of the same fixture.  Bar: the larger
    of 1e-12 and 10 x the float64-against-longdouble difference of the two recurrences, relative to max |K_k| of the 12-row gain."""
    XC, _ = GM.fix_extremal(fx, 1e30)
    assert np.all(XC[6] == GM.M0)
    Phi14, Phi12 = GM.fix_phi(fx, 1e30), G.fix_phi(fx)
    K14 = GM.recurrence(Phi14, np.longdouble)[0].astype(np.float64)
    K12 = np.asarray(G.fix_gains(fx))
    _, _, e14 = GM.gain_bars(Phi14)
    _, _, e12 = G.gain_bars(Phi12)
    bar = max(1e-12, 10.0 * max(float(e14.max()), float(e12.max())))
    rel = np.max(np.abs(K14[0:6, 0:6] - K12), axis=(0, 1)) / np.max(np.abs(K12), axis=(0, 1))
    print("MEASURED Isp = inf %s: K[0:6, 0:6] against the 12-row gains %.2e (bar %.1e)" % (GM.fix_id(fx), float(rel.max()), bar))
    assert float(rel.max()) <= bar


def test_rk4_reference_float64_against_longdouble():
    fx = GM.P2_FIX[0]
    XC, t = GM.fix_extremal(fx)
    x0 = XC[:7, 0] + GM.start_error(fx, 1e-3)
    lo = GM.fly_rk4(XC, t, GM.fix_gains(fx), x0, GM.fix_prm(fx), 3, 2, dtype=np.float64)
    hi = GM.fly_rk4(XC, t, GM.fix_gains(fx), x0, GM.fix_prm(fx), 3, 2, dtype=np.longdouble)
    assert float(np.max(np.abs(lo[0] - hi[0]) / GM.X_SCALE)) < 1e-12 and abs(float(lo[1] - hi[1])) < 1e-12


def test_binding_table_and_library_export_the_four_entries():
    lib = ctypes.CDLL(lto.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.SIGNATURES
        assert hasattr(lib, name)
    assert len(_lib.SIGNATURES["lto_guidance_gains_mass_batch"][1]) == 13
    assert len(_lib.SIGNATURES["lto_guided_flight_mass_batch"][1]) == 20
    for name in ("guidance_gains_mass", "guided_flight_mass"):
        assert hasattr(lto, name)
    for name in ("neighbouring_gains_mass", "fly_guided_mass", "dispersion_guided_mass", "guided_nav_mass"):
        assert hasattr(drivers, name)


def test_wrapper_refuses_bad_shapes_without_a_device():
    XC, t = GM.fix_extremal(GM.P2_FIX[0])
    K, prm = GM.fix_gains(GM.P2_FIX[0]), GM.fix_prm(GM.P2_FIX[0])
    x0 = np.zeros((7, 3))
    with pytest.raises(ValueError):
        hotpath.guidance_gains_mass(np.zeros((12, 9)), t, prm)
    with pytest.raises(ValueError):
        hotpath.guidance_gains_mass(XC, t, prm[:4] + (0.0,) + prm[5:])                        # Isp = 0
    with pytest.raises(ValueError):
        hotpath.guided_flight_mass(XC, t, K, np.zeros((6, 3)), prm)
    with pytest.raises(ValueError):
        hotpath.guided_flight_mass(XC[GM.IDX12], t, K, x0, prm)                               # a 12-row nominal
    with pytest.raises(ValueError):
        hotpath.guided_flight_mass(np.repeat(XC[:, :, None], 2, axis=2), t, K, x0, prm)      # two nominals, three starts
    with pytest.raises(ValueError):
        hotpath.guided_flight_mass(XC, t[:-1], K, x0, prm)
    with pytest.raises(ValueError):
        hotpath.guided_flight_mass(XC, t, K[:6, :6], x0, prm)
    with pytest.raises(ValueError):
        hotpath.guided_flight_mass(XC, t, K, x0, prm, update_every=3, nav=np.zeros((6, 3, 3)))  # six rows
    with pytest.raises(ValueError):
        hotpath.guided_flight_mass(XC, t, K, x0, prm, update_every=-1)
    with pytest.raises(ValueError):
        drivers.fly_guided_mass(None, np.zeros((12, 9)), t, prm)
    with pytest.raises(ValueError):
        drivers.fly_guided_mass(None, XC, t, prm, n_guid=1)
    with pytest.raises(ValueError):
        drivers.dispersion_guided_mass(None, np.zeros((12, 9)), t, prm, 4, 1.0, 1.0, 0)
    with pytest.raises(ValueError):
        drivers.dispersion_guided_mass(None, XC, t, prm, 4, 1.0, 1.0, 0, nav_sigma_v_ms=1.0)


def test_dispersion_guided_mass_draws_the_starts_of_dispersion(monkeypatch):
    """The starts are those `dispersion` makes for a 14-row solution, sample 0 undisturbed and the mass row left alone; the mass
    errors of the starts and of the navigation come from seeds of their own and leave the other draws as they are."""
    XC, t = GM.fix_extremal(GM.P2_FIX[0])
    prm = GM.fix_prm(GM.P2_FIX[0])
    seen = {}

    def fake_fly_control(ctx, XC_all, t_TU, p, x0, *a, **k):
        seen["open"] = np.array(x0)
        B = x0.shape[1]
        return dict(status=np.zeros(B, dtype=np.int32), miss_r_km=np.zeros(B), miss_v_ms=np.zeros(B))

    def fake_fly_guided_mass(ctx, XC_all, t_TU, p, x0, n_guid, update_every, nav, integ):
        seen["guided"], seen["nav"] = np.array(x0), nav
        B = x0.shape[1]
        return dict(status=np.zeros(B, dtype=np.int32), miss_r_km=np.zeros(B), miss_v_ms=np.zeros(B), dv_excess_ms=np.arange(B) * 1.0,
                    propellant_excess_kg=np.arange(B) * 0.5)
    monkeypatch.setattr(drivers, "fly_control", fake_fly_control)
    monkeypatch.setattr(drivers, "fly_guided_mass", fake_fly_guided_mass)
    a = drivers.dispersion(None, XC, t, prm, 17, 1.0, 0.01, 5)
    b = drivers.dispersion_guided_mass(None, XC, t, prm, 17, 1.0, 0.01, 5, update_every=3)
    assert np.array_equal(seen["open"], seen["guided"]) and np.array_equal(a["x0"], b["x0"]) and seen["nav"] is None
    assert np.array_equal(b["x0"][:, 0], XC[:7, 0]) and np.all(b["x0"][6] == GM.M0)
    assert np.array_equal(b["x0"], drivers.dispersion_starts(XC[:7, 0], 17, 1.0, 0.01, 5, DU, TU))
    c = drivers.dispersion_guided_mass(None, XC, t, prm, 17, 1.0, 0.01, 5, update_every=3, nav_sigma_r_km=0.5, nav_sigma_v_ms=0.02,
                                       nav_seed=9, sigma_m_kg=2.0, m_seed=21, nav_sigma_m_kg=0.25, nav_m_seed=33)
    assert np.array_equal(c["x0"][0:6], b["x0"][0:6]) and c["x0"][6, 0] == GM.M0
    assert np.allclose(c["x0"][6, 1:] - GM.M0, 2.0 * np.random.default_rng(21).standard_normal(17)[1:], rtol=0, atol=1e-12)
    nav = seen["nav"]
    assert nav.shape == (7, 3, 17) and not nav[:, :, 0].any()
    assert np.array_equal(nav[0:6], drivers.guided_nav(3, 17, 0.5, 0.02, 9, DU, TU))
    assert np.array_equal(nav[6], drivers.guided_nav_mass(3, 17, 0.25, 33))
    assert np.allclose(nav[6, :, 1:], 0.25 * np.random.default_rng(33).standard_normal((3, 17))[:, 1:], rtol=1e-15)
    d = drivers.dispersion_guided_mass(None, XC, t, prm, 17, 1.0, 0.01, 5, update_every=3, nav_sigma_m_kg=0.25, nav_m_seed=33)
    assert not seen["nav"][0:6].any() and np.array_equal(seen["nav"][6], nav[6]) and np.array_equal(d["x0"], b["x0"])
    assert sorted(c["percentiles"]) == ["dv_excess_ms", "miss_r_km", "miss_v_ms", "propellant_excess_kg"]
    assert c["percentiles"]["dv_excess_ms"][50] == 8.0 and c["percentiles"]["propellant_excess_kg"][50] == 4.0
    assert sorted(c["percentiles"]["propellant_excess_kg"]) == [50, 95, 99]
