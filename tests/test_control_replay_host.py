"""CPU: the reference of the control replay held to itself (tests/replay_reference.py), the order of the spline replay, the binding
table and the pure-numpy parts of the drivers.  No device."""
import numpy as np
import pytest

import lowthrustopt_amd as lto
import replay_reference as R
from lowthrustopt_amd import _lib, drivers, hotpath, synth
from lowthrustopt_amd.constants import MU, DU, TU


def test_numpy_rhs_is_the_oracles_rows():
    """Rows 0..5 of oracle.rhs_state_costate and rows 0..6 of oracle.rhs_state_costate_mass, lambda_v handed in: 1e-14."""
    from oracle import oracle as O
    rng = np.random.default_rng(5)
    worst = 0.0
    for p, rho in ((0.0, 1.0), (1.0, 0.1), (1.0, 0.01), (1.5, 1.0), (2.0, 1.0)):
        for thrust in (0.05, 1.0, 10.0):
            for td in (1.0, -1.0):
                y = 0.3 * rng.standard_normal(12)
                y[0] += 1.0
                prm = R.prm_tuple(thrust, p, rho, td)
                d, _ = R.rhs(y[:6], y[9:12], prm)
                worst = max(worst, float(np.max(np.abs(d - O.rhs_state_costate(y, np.array(prm))[:6]))))
                y14 = np.concatenate([y[:6], [900.0], y[6:], [0.3]])
                prm14 = R.prm_tuple(thrust, p, rho, td, R.ISP)
                d, _ = R.rhs(y14[:7], y14[10:13], prm14)
                worst = max(worst, float(np.max(np.abs(d - O.rhs_state_costate_mass(y14, np.array(prm14))[:7]))))
    print("MEASURED numpy rhs against the oracle's rows: %.3e" % worst)
    assert worst <= 1e-14
    # lambda_v = 0: no thrust
    d, um = R.rhs(np.array([1.0, 0.1, 0.0, 0.0, 0.1, 0.0]), np.zeros(3), R.prm_tuple(10.0, 2.0, 1.0))
    assert um == 0.0 and np.all(np.isfinite(d))


def test_thomas_moments_are_scipys_natural_spline():
    """The numpy Thomas solve against scipy.interpolate.CubicSpline(bc_type="natural") on every fixture's history, at 1e-13 of
    max|lambda_v|: the spline's values (at the knots and inside every interval), and the moments in the units of the values,
    M h^2 / 6 -- what a moment contributes to the spline.  The raw second derivatives are held to the same figure where the knots
    are 1/16 TU and more apart; on the 65-knot fixtures (h = 1/128 TU) a second derivative amplifies the rounding of the data by
    24 / h^2 = 4e5, so two correct solves may differ by 1e-11 of max|lambda_v| there and the raw comparison says nothing."""
    from scipy.interpolate import CubicSpline
    worst = 0.0
    for fx in list(R.CLASS_FIX.values()) + list(R.LANE_FIX):
        _, lamv, _ = R.fix_problem(fx)
        tk = np.linspace(0.0, fx.tof, fx.n_knots)
        h = fx.tof / (fx.n_knots - 1)
        M = R.spline_moments(lamv, h)
        cs = CubicSpline(tk, lamv, axis=1, bc_type="natural")
        scale = float(np.max(np.abs(lamv)))
        e_raw = float(np.max(np.abs(M - cs(tk, 2)))) / scale
        e_m = e_raw * h * h / 6.0
        e_v = 0.0
        for i in range(fx.n_knots - 1):
            lam = R.interval_cubic(lamv, M, i, h)
            for s in (0.0, 0.3 * h, h):
                e_v = max(e_v, float(np.max(np.abs(lam(s) - cs(tk[i] + s)))) / scale)
        worst = max(worst, e_m, e_v, e_raw if h >= 1.0 / 16.0 else 0.0)
        assert M[:, 0].tolist() == [0.0] * 3 and M[:, -1].tolist() == [0.0] * 3
        assert e_m <= 1e-13 and e_v <= 1e-13, (fx, e_m, e_v)
        assert h < 1.0 / 16.0 or e_raw <= 1e-13, (fx, e_raw)
    print("MEASURED moments and values against scipy's natural spline, of max|lambda_v|: %.3e" % worst)


def test_reference_held_to_itself():
    """Both determinations of every fixture; at most one in eight left out and every class of group B keeps one."""
    for group in (R.LANE_FIX, tuple(R.CLASS_FIX.values())):
        adm = R.admitted(group)
        assert len(group) - len(adm) <= len(group) // 8
    for cls in R.CLASSES:
        assert any(R.fix_e_ref(fx)[0] for name, fx in R.CLASS_FIX.items() if name.startswith(cls)), cls
    worst = {0.5: 0.0, 1.0: 0.0}
    for name, fx in list(R.CLASS_FIX.items()) + [("lane%d" % k, f) for k, f in enumerate(R.LANE_FIX)]:
        ok, e_x, e_dv = R.fix_e_ref(fx)
        if not ok:
            continue
        print("MEASURED e_ref %-18s final state %.3e, dv rel %.3e" % (name, e_x, e_dv))
        worst[fx.tof] = max(worst[fx.tof], e_x)
        assert e_x <= 1e-9 and e_dv <= 1e-8          # two determinations that agree no better measure nothing
    print("MEASURED e_ref, largest: 0.5 TU %.3e, 1 TU %.3e" % (worst[0.5], worst[1.0]))


def test_rk4_reference_float64_against_longdouble():
    worst = 0.0
    for name in ("p2_k4_1", "p1_rho01_k9_05", "m_p2_k9_05"):
        for steps in (1, 2, 16):
            ref, e = R.fix_rk4(R.CLASS_FIX[name], steps)
            worst = max(worst, e)
            assert np.all(np.isfinite(ref.x_final)) and e <= 1e-11
    print("MEASURED e_rk4, largest: %.3e" % worst)


def test_replay_of_an_extremal_is_third_order_in_the_knots():
    """One extremal of the 12-row oracle flow from node 0 of synth.indirect_problem(4, seed=3) over 1 TU (p = 2, 10 N): its
    lambda_v at the knots replayed from its own start, against its own end.  Each doubling of the knots cuts the miss by 8 (the
    end layer of the natural end conditions): miss(65) <= miss(17) / 16, a margin of 4 on the expected 64."""
    from oracle import oracle as O
    prm = R.prm_tuple(10.0, 2.0, 1.0)
    XC, _ = synth.indirect_problem(4, seed=3)
    y0 = np.array(XC[:, 0, 0])
    miss = {}
    for m in (17, 65):
        lamv = np.empty((3, m))
        y = y0.copy()
        lamv[:, 0] = y[9:12]
        for k in range(1, m):
            y, rc, _, _ = O.flow_state_costate(y, np.array(prm), 1.0 / (m - 1), O.DOP853_ADAPTIVE, 0, 1e-13, 1e-13)
            assert rc == 0
            lamv[:, k] = y[9:12]
        fl = R.fly(y0[:6], lamv, 0.0, 1.0, prm)
        assert fl.ok
        miss[m] = float(np.max(np.abs(fl.x_final - y[:6])))
    print("MEASURED replay miss: 17 knots %.3e, 65 knots %.3e" % (miss[17], miss[65]))
    assert miss[65] <= miss[17] / 16.0


def test_binding_table_and_mirror():
    assert {"lto_control_replay_batch", "lto_control_replay"} <= set(_lib.SIGNATURES)
    assert len(_lib.SIGNATURES["lto_control_replay_batch"][1]) == 19 and len(_lib.SIGNATURES["lto_control_replay"][1]) == 16
    assert callable(hotpath.control_replay) and callable(lto.control_replay)
    assert callable(drivers.fly_control) and callable(drivers.dispersion)
    assert lto.load_library().lto_version() == 102


def test_mirror_refuses_bad_shapes_without_a_device():
    prm = lto.make_params(MU, DU, TU, 10.0, 1e3, 1.0, 2.0, 1.0)
    with pytest.raises(ValueError):
        lto.control_replay(np.zeros((6, 2)), np.zeros((2, 9)), 0.0, 1.0, prm)            # lamv rows
    with pytest.raises(ValueError):
        lto.control_replay(np.zeros((6, 4)), np.zeros((3, 9, 2)), 0.0, 1.0, prm)         # neither one history nor B
    with pytest.raises(ValueError):
        lto.control_replay(np.zeros((6, 4)), np.zeros((3, 9)), 0.0, 1.0, [prm, prm])     # neither one parameter set nor B


def test_sample_knots():
    assert hotpath.replay_sample_knots(9, 0).tolist() == []
    assert hotpath.replay_sample_knots(9, 1).tolist() == list(range(9))
    assert hotpath.replay_sample_knots(9, 3).tolist() == [0, 3, 6, 8]
    assert hotpath.replay_sample_knots(9, 8).tolist() == [0, 8]
    assert hotpath.replay_sample_knots(9, 14).tolist() == [0, 8]
    assert hotpath.replay_sample_knots(9, 4).tolist() == [0, 4, 8]


def test_dispersion_draw_and_units():
    x = np.array([1.1, 0.02, -0.03, 0.01, 0.2, -0.01])
    a = drivers.dispersion_starts(x, 500, 1.0, 0.01, 7, DU, TU)
    b = drivers.dispersion_starts(x, 500, 1.0, 0.01, 7, DU, TU)
    c = drivers.dispersion_starts(x, 500, 1.0, 0.01, 8, DU, TU)
    assert a.shape == (6, 500) and np.array_equal(a, b) and not np.array_equal(a, c)
    assert np.array_equal(a[:, 0], x)                                  # sample 0 is the undisturbed start, bit for bit
    d = a - x[:, None]
    # 1 km and 1 cm/s per axis: the sample deviations in physical units (1 497 values each: a few per cent of scatter)
    assert abs(np.std(d[0:3, 1:]) * DU - 1.0) < 0.1
    assert abs(np.std(d[3:6, 1:]) * DU / TU * 1e3 - 0.01) < 0.001
    x7 = np.append(x, 1000.0)
    a7 = drivers.dispersion_starts(x7, 16, 1.0, 0.01, 7, DU, TU)
    assert np.all(a7[6] == 1000.0) and np.array_equal(a7[:6], drivers.dispersion_starts(x, 16, 1.0, 0.01, 7, DU, TU))
    # misses: 3-4-0 km in position, 0.1 m/s in one velocity axis, 2 kg
    xt = x7.copy()
    xf = np.stack([xt, xt + np.array([3.0 / DU, 4.0 / DU, 0.0, 0.0, 0.1 / 1e3 * TU / DU, 0.0, -2.0])], axis=1)
    ms = drivers.replay_misses(xf, xt, DU, TU)
    assert ms["miss_r_km"][0] == 0.0 and ms["miss_v_ms"][0] == 0.0 and ms["miss_m_kg"][0] == 0.0
    assert abs(ms["miss_r_km"][1] - 5.0) < 1e-9 and abs(ms["miss_v_ms"][1] - 0.1) < 1e-12 and ms["miss_m_kg"][1] == -2.0
    assert "miss_m_kg" not in drivers.replay_misses(xf[:6], xt[:6], DU, TU)
