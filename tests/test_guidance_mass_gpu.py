"""Neighbouring-extremal guidance of 14-row variable-mass solutions on the device (k_guidance_gains<7>, k_guided_flight<7>)
against tests/guidance_mass_reference.py, whose fixtures tests/test_guidance_mass_host.py admits: A the gains against the longdouble
recurrence on the device's own Phi, batches and singular fixtures, B the flight fed the reference's gains, C first-order optimality
end to end, D refusals and poisoned lanes, E a converged transfer, and the Isp = infinity reduction to the 12-row gains."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

import lowthrustopt_amd as lto
import guidance_reference as G
import guidance_mass_reference as GM
from lowthrustopt_amd import drivers
from lowthrustopt_amd.constants import MU, DU, TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_id = GM.fix_id


# ------------------------------------------------------------------------------------------------------------- A, gains
def _check_gains(label, g, Phi_dev, fx=None):
    K_ref, bar, e_ref = GM.gain_bars(Phi_dev)
    scale = np.max(np.abs(K_ref), axis=(0, 1))
    err = np.max(np.abs(g.K - K_ref), axis=(0, 1)) / scale
    _, piv_ref = GM.recurrence(Phi_dev, np.float64)
    e_piv = float(np.max(np.abs(g.pivot - piv_ref) / piv_ref))
    line = "MEASURED 14-row gains %s: largest relative error %.3e (bar there %.1e, e_ref %.1e), pivot ratio rel %.1e, smallest %.2e" % (
        label, float(err.max()), float(bar[int(np.argmax(err / bar))]), float(e_ref.max()), e_piv, float(g.pivot.min()))
    if fx is not None:
        Ko = GM.fix_gains(fx)
        line += "; end to end against the oracle-Phi gains %.3e (reported)" % float(
            np.max(np.max(np.abs(g.K - Ko), axis=(0, 1)) / np.max(np.abs(Ko), axis=(0, 1))))
    print(line)
    assert g.status == 0, label
    assert np.all(err <= bar), (label, err, bar)
    assert e_piv < 1e-9, label


@pytest.mark.gpu
@pytest.mark.parametrize("fx", GM.REGULAR_FIX, ids=_id)
def test_gains_against_the_longdouble_recurrence(gpu_ctx, fx):
    XC, t = GM.fix_extremal(fx)
    prm = GM.fix_prm(fx)
    g = lto.guidance_gains_mass(XC, t, prm, ctx=gpu_ctx)
    assert g.K.shape == (7, 7, fx.n - 1) and g.pivot.shape == (fx.n - 1,)
    Phi, _ = lto.indirect_stm(XC, t, lto.make_params(*prm), ctx=gpu_ctx)
    assert Phi.shape == (14, 14, fx.n - 1)
    _check_gains(_id(fx), g, Phi, fx)


@pytest.mark.gpu
def test_gains_rk4(gpu_ctx):
    fx = GM.P2_FIX[3]
    XC, t = GM.fix_extremal(fx)
    integ = lto.integrator(lto.RK4, steps=64)
    g = lto.guidance_gains_mass(XC, t, GM.fix_prm(fx), integ, ctx=gpu_ctx)
    Phi, _ = lto.indirect_stm(XC, t, lto.make_params(*GM.fix_prm(fx)), integ, ctx=gpu_ctx)
    _check_gains("RK4 x 64 " + _id(fx), g, Phi, fx)


NINE = GM.P2_FIX + (GM.BACK_FIX, GM.P1_FIX, GM.P15_FIX)   # the regular fixtures of nine nodes: three classes, three grids
_GAIN_SINGLES = {}


def _gain_single(ctx, fx):
    if fx not in _GAIN_SINGLES:
        XC, t = GM.fix_extremal(fx)
        g = lto.guidance_gains_mass(XC, t, GM.fix_prm(fx), ctx=ctx)
        _GAIN_SINGLES[fx] = (g.K.copy(), g.pivot.copy(), g.status)
    return _GAIN_SINGLES[fx]


def _stack(fixtures):
    XC = np.asfortranarray(np.stack([GM.fix_extremal(f)[0] for f in fixtures], axis=2))
    t = np.asfortranarray(np.stack([GM.fix_extremal(f)[1] for f in fixtures], axis=1))
    return XC, t, [GM.fix_prm(f) for f in fixtures]


@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, 64, 65])
def test_gain_batches_are_their_single_calls(gpu_ctx, B):
    """Per-trajectory grids and parameters (n_tgrids = n_prm = B), three control-law classes in one batch: every trajectory's
    gains, pivot ratios and status are those of its single call, bit for bit."""
    fixtures = [NINE[(3 * b + b // 11) % len(NINE)] for b in range(B)]
    XC, t, prms = _stack(fixtures)
    g = lto.guidance_gains_mass(XC, t, prms, ctx=gpu_ctx)
    assert g.K.shape == (7, 7, 8, B) and np.all(g.status == 0)
    for b, fx in enumerate(fixtures):
        K1, p1, s1 = _gain_single(gpu_ctx, fx)
        assert np.array_equal(g.K[:, :, :, b], K1) and np.array_equal(g.pivot[:, b], p1) and g.status[b] == s1, (b, fx)


@pytest.mark.gpu
def test_gain_batch_of_short_trajectories(gpu_ctx):
    """2, 3 and 5 nodes."""
    for fx in GM.SMALL_FIX:
        XC, t = GM.fix_extremal(fx)
        one = lto.guidance_gains_mass(XC, t, GM.fix_prm(fx), ctx=gpu_ctx)
        XB = np.asfortranarray(np.repeat(XC[:, :, None], 5, axis=2))
        g = lto.guidance_gains_mass(XB, t, GM.fix_prm(fx), ctx=gpu_ctx)        # one grid, one parameter set
        assert g.K.shape == (7, 7, fx.n - 1, 5) and np.all(g.status == 0)
        for b in range(5):
            assert np.array_equal(g.K[:, :, :, b], one.K) and np.array_equal(g.pivot[:, b], one.pivot)


@pytest.mark.gpu
@pytest.mark.parametrize("fx", GM.SINGULAR_FIX, ids=_id)
def test_singular_fixtures_get_status_3_alone(gpu_ctx, fx):
    left, right = GM.P2_FIX[1], GM.P15_FIX
    XC, t, prms = _stack([left, fx, right])
    g = lto.guidance_gains_mass(XC, t, prms, ctx=gpu_ctx)
    print("MEASURED 14-row singular %s: last-segment pivot ratio %.2e" % (_id(fx), g.pivot[-1, 1]))
    assert list(g.status) == [0, 3, 0]
    assert g.pivot[-1, 1] < 1e-10 and np.all(np.isnan(g.pivot[:-1, 1]))
    assert np.all(np.isnan(g.K[:, :, :, 1]))
    for b, nb in ((0, left), (2, right)):
        K1, p1, _ = _gain_single(gpu_ctx, nb)
        assert np.array_equal(g.K[:, :, :, b], K1) and np.array_equal(g.pivot[:, b], p1)


@pytest.mark.gpu
def test_a_pivot_below_sing_tol_ends_the_sweep_at_its_node(gpu_ctx):
    """sing_tol placed between the ratio of DIP_FIX's node 2 and those of all its later nodes and of the neighbour: NaN gains from
    that node down, the later ones bit for bit what they are under the default, the neighbour untouched."""
    XC, t, prms = _stack([GM.DIP_FIX, GM.DIP_NEIGHBOUR])
    ok = lto.guidance_gains_mass(XC, t, prms, ctx=gpu_ctx)
    assert list(ok.status) == [0, 0]
    piv, k = ok.pivot[:, 0], GM.DIP_NODE
    above = min(piv[k + 1:].min(), ok.pivot[:, 1].min())
    assert piv[k] < 0.8 * above, (piv, ok.pivot[:, 1])
    tol = float(np.sqrt(piv[k] * above))
    g = lto.guidance_gains_mass(XC, t, prms, sing_tol=tol, ctx=gpu_ctx)
    assert list(g.status) == [3, 0]
    assert np.all(np.isnan(g.K[:, :, :k + 1, 0])) and np.array_equal(g.K[:, :, k + 1:, 0], ok.K[:, :, k + 1:, 0])
    assert g.pivot[k, 0] == piv[k] and np.all(np.isnan(g.pivot[:k, 0])) and np.array_equal(g.pivot[k + 1:, 0], piv[k + 1:])
    assert np.array_equal(g.K[:, :, :, 1], ok.K[:, :, :, 1]) and np.array_equal(g.pivot[:, 1], ok.pivot[:, 1])


# ------------------------------------------------------------------------------------------------------------ B, flight
def _start(fx, size=1e-3):
    return GM.fix_extremal(fx)[0][:7, 0] + GM.start_error(fx, size)


def _check_flight(label, r, bars):
    ref = bars.ref
    e_x = float(np.max(np.abs(r.x_final - ref.x_final) / GM.X_SCALE))
    e_lam = float(np.max(np.abs(r.lam_final - ref.lam_final)))
    e_dv = abs(r.dv - bars.dv) / abs(bars.dv)
    print("MEASURED 14-row flight %s: |x - ref| %.3e (mass row / m0; bar %.1e, e_ref %.1e), dv rel %.3e (bar %.1e), |lam - ref| %.3e "
          "(bar %.1e), m_f %.6f kg" % (label, e_x, bars.bar_x, bars.e_x, e_dv, bars.bar_dv, e_lam, bars.bar_lam, r.x_final[6]))
    assert r.status == 0, label
    assert np.all(np.abs(r.x_final - ref.x_final) / GM.X_SCALE <= bars.bar_x), label
    assert e_dv <= bars.bar_dv, label
    assert np.all(np.abs(r.lam_final - ref.lam_final) <= bars.bar_lam), label


FLIGHT_CASES = ([(GM.P2_FIX[0], e) for e in (0, 1, 3, 8, 100)] + [(GM.P1_FIX, 1), (GM.P15_FIX, 3), (GM.BACK_FIX, 1), (GM.P0_FIX[0], 0)])


@pytest.mark.gpu
@pytest.mark.parametrize("fx,every", FLIGHT_CASES, ids=lambda v: _id(v) if isinstance(v, tuple) else "every%d" % v)
def test_flight_against_the_reference(gpu_ctx, fx, every):
    XC, t = GM.fix_extremal(fx)
    prm = GM.fix_prm(fx)
    K = GM.fix_gains(fx) if every > 0 else np.zeros((7, 7, fx.n - 1))          # p = 0 has no gains and needs none
    x0 = _start(fx)
    r = lto.guided_flight_mass(XC, t, K, x0, prm, every, with_nodes=True, ctx=gpu_ctx)
    _check_flight("%s every %d" % (_id(fx), every), r, GM.flight_bars(XC, t, K, x0, prm, every))
    assert np.array_equal(r.nodes[:, 0], x0) and np.array_equal(r.nodes[:, -1], r.x_final)
    if every == 0:
        # the plain 14-row flow from (x0, lambda_nom,0) in ONE span
        y0 = np.concatenate([x0, XC[7:14, 0]])
        a, b = GM.flow14(y0, prm, fx.tof, 1e-13)[0], GM.flow14(y0, prm, fx.tof, 1e-12)[0]
        bar = max(1e-12, 10.0 * float(np.max(np.abs(a[:7] - b[:7]) / GM.X_SCALE)))
        err = np.abs(r.x_final - a[:7]) / GM.X_SCALE
        print("MEASURED 14-row flight %s open loop against one span: %.3e (bar %.1e)" % (_id(fx), float(err.max()), bar))
        assert np.all(err <= bar)


@pytest.mark.gpu
def test_flight_with_navigation_errors(gpu_ctx):
    """Navigation errors on all seven measured rows, 0.1 kg on the mass."""
    fx = GM.P2_FIX[1]
    XC, t = GM.fix_extremal(fx)
    K, prm = GM.fix_gains(fx), GM.fix_prm(fx)
    nav = 1e-4 * np.random.default_rng(5).standard_normal((7, 3))
    nav[6] *= 1e3
    x0 = _start(fx)
    r = lto.guided_flight_mass(XC, t, K, x0, prm, 3, nav, ctx=gpu_ctx)
    _check_flight("%s every 3 with nav" % _id(fx), r, GM.flight_bars(XC, t, K, x0, prm, 3, nav))
    clean = lto.guided_flight_mass(XC, t, K, x0, prm, 3, ctx=gpu_ctx)
    assert np.max(np.abs(clean.x_final[:6] - r.x_final[:6])) > 1e-6            # the errors were applied
    zero = lto.guided_flight_mass(XC, t, K, x0, prm, 3, np.zeros((7, 3)), ctx=gpu_ctx)
    assert np.array_equal(zero.x_final, clean.x_final) and zero.dv == clean.dv
    # ... the mass row's among them.  The unclamped p = 2 law does not see the mass; the p = 1 law's thrust is cT / m
    f1 = GM.P1_FIX
    X1, t1 = GM.fix_extremal(f1)
    only_m = np.zeros((7, 3))
    only_m[6] = nav[6]
    rm = lto.guided_flight_mass(X1, t1, GM.fix_gains(f1), _start(f1), GM.fix_prm(f1), 3, only_m, ctx=gpu_ctx)
    _check_flight("%s every 3 with mass nav only" % _id(f1), rm, GM.flight_bars(X1, t1, GM.fix_gains(f1), _start(f1), GM.fix_prm(f1), 3, only_m))
    clean1 = lto.guided_flight_mass(X1, t1, GM.fix_gains(f1), _start(f1), GM.fix_prm(f1), 3, ctx=gpu_ctx)
    assert np.max(np.abs(clean1.x_final[:6] - rm.x_final[:6])) > 1e-9


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [1, 2, 16])
def test_flight_rk4(gpu_ctx, steps):
    """Against the longdouble restatement of the algorithm, bar 1e-12 (the mass row relative to m0)."""
    fx = GM.P2_FIX[0]
    XC, t = GM.fix_extremal(fx)
    K, prm, x0 = GM.fix_gains(fx), GM.fix_prm(fx), _start(fx)
    hi = GM.fly_rk4(XC, t, K, x0, prm, 3, steps, dtype=np.longdouble)
    r = lto.guided_flight_mass(XC, t, K, x0, prm, 3, integ=lto.integrator(lto.RK4, steps=steps), ctx=gpu_ctx)
    e_x = float(np.max(np.abs(r.x_final - hi[0].astype(np.float64)) / GM.X_SCALE))
    e_dv = abs(r.dv - float(hi[1]))
    print("MEASURED 14-row flight RK4 x %d: |x - longdouble| %.3e (mass row / m0), dv %.3e (bar 1e-12)" % (steps, e_x, e_dv))
    assert r.status == 0 and r.accepted == 8 * steps and r.rejected == 0
    assert e_x <= 1e-12 and e_dv <= 1e-12


LANE_FIX = GM.P2_FIX[:5] + (GM.BACK_FIX, GM.P1_FIX, GM.P15_FIX)
_FLIGHT_SINGLES = {}


def _lane_problem(own, j):
    """Template j: under its own nominal, or fixture j's start error on the nominal of fixture 0."""
    fn = LANE_FIX[j] if own else LANE_FIX[0]
    x0 = GM.fix_extremal(fn)[0][:7, 0] + GM.start_error(LANE_FIX[j], 1e-4 * (j + 1))
    return fn, x0


def _flight_single(ctx, own, j):
    if (own, j) not in _FLIGHT_SINGLES:
        fn, x0 = _lane_problem(own, j)
        XC, t = GM.fix_extremal(fn)
        r = lto.guided_flight_mass(XC, t, GM.fix_gains(fn), x0, GM.fix_prm(fn), 3, with_nodes=True, ctx=ctx)
        assert r.status == 0
        _FLIGHT_SINGLES[(own, j)] = r
    return _FLIGHT_SINGLES[(own, j)]


@pytest.mark.gpu
@pytest.mark.parametrize("own", [False, True], ids=["nom1", "nomB"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 129])
def test_flight_lanes_are_their_single_calls(gpu_ctx, B, own):
    """n_nom = 1 and n_nom = B (own nominal, gains, grid and parameters, three classes in one batch): every lane bit for bit its
    single call; node 0 is the start and the last node x_final, bit for bit."""
    js = [(5 * b + b // 8) % len(LANE_FIX) for b in range(B)]
    x0 = np.asfortranarray(np.stack([_lane_problem(own, j)[1] for j in js], axis=1))
    if own:
        XC, t, prms = _stack([LANE_FIX[j] for j in js])
        K = np.asfortranarray(np.stack([GM.fix_gains(LANE_FIX[j]) for j in js], axis=3))
    else:
        (XC, t), K, prms = GM.fix_extremal(LANE_FIX[0]), GM.fix_gains(LANE_FIX[0]), GM.fix_prm(LANE_FIX[0])
    r = lto.guided_flight_mass(XC, t, K, x0, prms, 3, with_nodes=True, ctx=gpu_ctx)
    assert r.x_final.shape == (7, B) and r.nodes.shape == (7, 9, B) and np.all(r.status == 0)
    assert np.array_equal(r.nodes[:, 0, :], x0) and np.array_equal(r.nodes[:, -1, :], r.x_final)
    for b, j in enumerate(js):
        s = _flight_single(gpu_ctx, own, j)
        assert np.array_equal(r.x_final[:, b], s.x_final) and np.array_equal(r.lam_final[:, b], s.lam_final) and r.dv[b] == s.dv, b
        assert np.array_equal(r.nodes[:, :, b], s.nodes) and r.accepted[b] == s.accepted and r.rejected[b] == s.rejected, b


# ---------------------------------------------------------------------------------------- C, first-order optimality
@pytest.mark.gpu
@pytest.mark.parametrize("fx", GM.NINE_P2, ids=_id)
def test_device_gains_and_flight_quarter_the_miss(gpu_ctx, fx):
    """Device gains, device flight, one update at node 0: halving the start error (the mass error with it) quarters the (r, v) miss
    (ratios inside [3.8, 4.2]); the open-loop flight from the same starts halves it (ratios inside [1.8, 2.2])."""
    XC, t = GM.fix_extremal(fx)
    prm = GM.fix_prm(fx)
    gains = drivers.neighbouring_gains_mass(gpu_ctx, XC, t, prm)
    assert gains["ok"]
    x0 = np.asfortranarray(np.stack([XC[:7, 0] + GM.start_error(fx, s) for s in (2e-3, 1e-3, 5e-4)], axis=1))
    for every, lo, hi in ((fx.n, 3.8, 4.2), (0, 1.8, 2.2)):
        r = lto.guided_flight_mass(XC, t, gains["K"], x0, prm, every, ctx=gpu_ctx)
        assert np.all(r.status == 0)
        miss = np.linalg.norm(r.x_final[:6] - XC[:6, -1:], axis=0)
        r1, r2 = miss[0] / miss[1], miss[1] / miss[2]
        line = "MEASURED 14-row %s %s: miss ratios %.3f %.3f" % (_id(fx), "one update" if every else "open loop", r1, r2)
        if every:
            dl = np.abs(r.lam_final[6] - XC[13, -1])
            line += "; lambda_m(tf) deviation ratios %.3f %.3f (reported)" % (dl[0] / dl[1], dl[1] / dl[2])
        print(line)
        assert lo < r1 < hi and lo < r2 < hi


# ------------------------------------------------------------------------------------------------ D, refusals and poison
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _raw_gains(ctx, n=9, B=2, n_tgrids=1, n_prm=1, integ=None, sing_tol=1e-10, null=(), pad=0, t=None):
    fx = GM.P2_FIX[0]
    XC, tt = GM.fix_extremal(fx)
    nn, Bn = max(n, 2), max(B, 1)
    X = np.asfortranarray(np.repeat(np.asarray(XC)[:, :nn, None], Bn, axis=2))
    tg = np.asfortranarray(np.repeat((np.asarray(tt)[:nn] if t is None else np.asarray(t, dtype=float))[:, None], max(n_tgrids, 1), axis=1))
    prms = (lto.LtoParams * max(n_prm, 1))(*[lto.make_params(*GM.fix_prm(fx))] * max(n_prm, 1))
    integ = integ or lto.integrator()
    out = dict(K=np.full(49 * (nn - 1) * Bn + pad, -7.0), pivot=np.full((nn - 1) * Bn + pad, -7.0),
               status=np.full(Bn + pad, -7, dtype=np.int32))
    a = {k: (None if k in null else v) for k, v in out.items()}
    rc = ctx.lib.lto_guidance_gains_mass_batch(ctx.handle, n, B, None if "XC" in null else _p(X), None if "t" in null else _p(tg),
                                               n_tgrids, None if "prm" in null else prms, n_prm,
                                               None if "integ" in null else C.byref(integ), sing_tol, _p(a["K"]), _p(a["pivot"]),
                                               _p(a["status"]))
    return rc, out


def _raw_flight(ctx, n=9, B=3, n_nom=1, n_prm=1, every=3, integ=None, null=(), pad=0, t=None, with_nav=True):
    fx = GM.P2_FIX[0]
    XC, tt = GM.fix_extremal(fx)
    nn, Bn, nm = max(n, 2), max(B, 1), max(n_nom, 1)
    X = np.asfortranarray(np.repeat(np.asarray(XC)[:, :nn, None], nm, axis=2))
    K = np.asfortranarray(np.repeat(np.asarray(GM.fix_gains(fx))[:, :, :nn - 1, None], nm, axis=3))
    tg = np.asfortranarray(np.repeat((np.asarray(tt)[:nn] if t is None else np.asarray(t, dtype=float))[:, None], nm, axis=1))
    x0 = np.asfortranarray(np.stack([XC[:7, 0] + GM.start_error(fx, 1e-4 * (b + 1)) for b in range(Bn)], axis=1))
    n_upd = GM.n_updates(nn, every) if every > 0 else 0
    nav = np.asfortranarray(1e-5 * np.random.default_rng(2).standard_normal((7, max(n_upd, 1), Bn)))
    prms = (lto.LtoParams * max(n_prm, 1))(*[lto.make_params(*GM.fix_prm(fx))] * max(n_prm, 1))
    integ = integ or lto.integrator()
    out = dict(x_final=np.full(7 * Bn + pad, -7.0), lam_final=np.full(7 * Bn + pad, -7.0), dv=np.full(Bn + pad, -7.0),
               nodes=np.full(7 * nn * Bn + pad, -7.0), accepted=np.full(Bn + pad, -7, dtype=np.int32),
               rejected=np.full(Bn + pad, -7, dtype=np.int32), status=np.full(Bn + pad, -7, dtype=np.int32))
    a = {k: (None if k in null else v) for k, v in out.items()}
    rc = ctx.lib.lto_guided_flight_mass_batch(ctx.handle, n, B, None if "XC" in null else _p(X), None if "t" in null else _p(tg),
                                              None if "K" in null else _p(K), n_nom, None if "x0" in null else _p(x0), every,
                                              _p(nav) if with_nav and "nav" not in null else None, None if "prm" in null else prms,
                                              n_prm, None if "integ" in null else C.byref(integ), _p(a["x_final"]), _p(a["lam_final"]),
                                              _p(a["dv"]), _p(a["nodes"]), _p(a["accepted"]), _p(a["rejected"]), _p(a["status"]))
    return rc, out


@pytest.mark.gpu
def test_refusals(gpu_ctx):
    down = np.linspace(0.0, 0.5, 9)
    down[4] = down[3]
    others = (lto.integrator(lto.RKF78_FIXED, steps=4), lto.integrator(lto.RKF78_ADAPTIVE))
    # gains
    assert _raw_gains(gpu_ctx)[0] == 0
    for name in ("XC", "t", "prm", "integ", "K", "status"):
        assert _raw_gains(gpu_ctx, null=(name,))[0] == -2, name
    assert gpu_ctx.lib.lto_guidance_gains_mass_batch(None, 9, 1, None, None, 1, None, 1, None, 1e-10, None, None, None) == -2
    for kw in (dict(n=1), dict(B=0), dict(t=down), dict(t=down[::-1].copy()), dict(n_tgrids=0), dict(n_tgrids=3, B=2), dict(n_prm=0),
               dict(n_prm=3, B=2), dict(sing_tol=0.0), dict(sing_tol=1.0), dict(sing_tol=-1e-3), dict(sing_tol=float("nan"))):
        assert _raw_gains(gpu_ctx, **kw)[0] == -1, kw
    for integ in others:
        assert _raw_gains(gpu_ctx, integ=integ)[0] == -3
    assert _raw_gains(gpu_ctx, n=2)[0] == 0
    # flight
    assert _raw_flight(gpu_ctx)[0] == 0
    for name in ("XC", "t", "K", "x0", "prm", "integ", "x_final", "dv", "status"):
        assert _raw_flight(gpu_ctx, null=(name,))[0] == -2, name
    assert gpu_ctx.lib.lto_guided_flight_mass_batch(None, 9, 1, None, None, None, 1, None, 1, None, None, 1, None, None, None, None,
                                                    None, None, None, None) == -2
    for kw in (dict(n=1), dict(B=0), dict(t=down), dict(n_nom=0), dict(n_nom=2, B=3), dict(n_prm=0), dict(n_prm=2, B=3),
               dict(every=-1)):
        assert _raw_flight(gpu_ctx, **kw)[0] == -1, kw
    for integ in others:
        assert _raw_flight(gpu_ctx, integ=integ)[0] == -3
    assert _raw_flight(gpu_ctx, n=2, every=1)[0] == 0 and _raw_flight(gpu_ctx, every=0)[0] == 0
    # the 12-row entries still send 14 rows away, and the Python mirror raises what the library answers
    XC, t = GM.fix_extremal(GM.P2_FIX[0])
    with pytest.raises(lto.LtoError) as ei:
        lto.guidance_gains(XC, t, GM.fix_prm(GM.P2_FIX[0]), ctx=gpu_ctx)
    assert ei.value.code == -3
    with pytest.raises(lto.LtoError) as ei:
        lto.guidance_gains_mass(XC, t, GM.fix_prm(GM.P2_FIX[0]), lto.integrator(lto.RKF78_ADAPTIVE), ctx=gpu_ctx)
    assert ei.value.code == -3


@pytest.mark.gpu
def test_outputs_stay_inside_their_extents_and_optional_ones_may_be_null(gpu_ctx):
    rc, full = _raw_gains(gpu_ctx, B=3, pad=5)
    assert rc == 0 and np.all(full["status"][:3] == 0)
    for k, n in (("K", 49 * 8 * 3), ("pivot", 8 * 3), ("status", 3)):
        assert np.all(full[k][n:] == -7) and not np.any(full[k][:n] == -7), k
    rc, part = _raw_gains(gpu_ctx, B=3, pad=5, null=("pivot",))
    assert rc == 0 and np.array_equal(part["K"], full["K"]) and np.all(part["pivot"] == -7)
    for n_nom in (1, 3):
        rc, full = _raw_flight(gpu_ctx, B=3, n_nom=n_nom, pad=5)
        assert rc == 0 and np.all(full["status"][:3] == 0)
        for k, n in (("x_final", 21), ("lam_final", 21), ("dv", 3), ("nodes", 7 * 9 * 3), ("accepted", 3), ("rejected", 3), ("status", 3)):
            assert np.all(full[k][n:] == -7) and not np.any(full[k][:n] == -7), k
        rc, part = _raw_flight(gpu_ctx, B=3, n_nom=n_nom, pad=5, null=("lam_final", "nodes", "accepted", "rejected"))
        assert rc == 0
        for k in ("x_final", "dv", "status"):
            assert np.array_equal(part[k], full[k]), k
        for k in ("lam_final", "nodes", "accepted", "rejected"):
            assert np.all(part[k] == -7), k
    # the one-trajectory entries are the batch entries at B = 1
    fx = GM.P2_FIX[0]
    XC, t = GM.fix_extremal(fx)
    X, tt = np.asfortranarray(XC), np.array(t)
    integ, pr = lto.integrator(), lto.make_params(*GM.fix_prm(fx))
    K, piv, st = np.zeros((7, 7, 8), order="F"), np.zeros(8), np.full(1, -7, dtype=np.int32)
    assert gpu_ctx.lib.lto_guidance_gains_mass(gpu_ctx.handle, 9, _p(X), _p(tt), C.byref(pr), C.byref(integ), 1e-10, _p(K), _p(piv),
                                               _p(st)) == 0
    K1, p1, _ = _gain_single(gpu_ctx, fx)
    assert st[0] == 0 and np.array_equal(K, K1) and np.array_equal(piv, p1)
    x0, xf, dv = _start(fx), np.zeros(7), np.zeros(1)
    assert gpu_ctx.lib.lto_guided_flight_mass(gpu_ctx.handle, 9, _p(X), _p(tt), _p(K), _p(x0), 3, None, C.byref(pr), C.byref(integ),
                                              _p(xf), None, _p(dv), None, None, None, _p(st)) == 0
    r = lto.guided_flight_mass(XC, t, K, x0, GM.fix_prm(fx), 3, ctx=gpu_ctx)
    assert st[0] == 0 and np.array_equal(xf, r.x_final) and dv[0] == r.dv


def t_B(t, B):
    return np.asfortranarray(np.repeat(np.asarray(t)[:, None], B, axis=1))


@pytest.mark.gpu
def test_poisoned_lanes_fail_alone(gpu_ctx):
    """A NaN or infinite start, a start mass of 0, below 0 or NaN, a NaN gain at an update node: status 2 and NaN results from the
    failing span on, the neighbours bit for bit what they are without the poisoned lane."""
    fx = GM.P2_FIX[0]
    XC, t = GM.fix_extremal(fx)
    prm = GM.fix_prm(fx)
    x0 = np.asfortranarray(np.stack([_start(fx, 1e-4 * (b + 1)) for b in range(3)], axis=1))
    K3 = np.asfortranarray(np.repeat(np.asarray(GM.fix_gains(fx))[:, :, :, None], 3, axis=3))
    X3 = np.asfortranarray(np.repeat(np.asarray(XC)[:, :, None], 3, axis=2))
    good = lto.guided_flight_mass(X3, t_B(t, 3), K3, x0, prm, 3, with_nodes=True, ctx=gpu_ctx)
    assert np.all(good.status == 0)

    def neighbours_unchanged(r):
        for b in (0, 2):
            assert np.array_equal(r.x_final[:, b], good.x_final[:, b]) and r.dv[b] == good.dv[b]
            assert np.array_equal(r.nodes[:, :, b], good.nodes[:, :, b]) and np.array_equal(r.lam_final[:, b], good.lam_final[:, b])
            assert r.accepted[b] == good.accepted[b] and r.rejected[b] == good.rejected[b]
    for row, value in ((1, np.nan), (4, np.inf), (6, 0.0), (6, -1000.0), (6, np.nan), (6, np.inf)):
        bad = x0.copy(order="F")
        bad[row, 1] = value
        r = lto.guided_flight_mass(X3, t_B(t, 3), K3, bad, prm, 3, with_nodes=True, ctx=gpu_ctx)
        assert list(r.status) == [0, 2, 0], (row, value)
        assert np.all(np.isnan(r.x_final[:, 1])) and np.isnan(r.dv[1]) and np.all(np.isnan(r.nodes[:, 1:, 1]))
        assert np.all(np.isnan(r.lam_final[:, 1])) and np.array_equal(r.nodes[:, 0, 1], bad[:, 1], equal_nan=True)
        neighbours_unchanged(r)
    Kbad = K3.copy(order="F")
    Kbad[2, 6, 3, 1] = np.nan                                             # node 3 is an update node of update_every = 3
    r = lto.guided_flight_mass(X3, t_B(t, 3), Kbad, x0, prm, 3, with_nodes=True, ctx=gpu_ctx)
    assert list(r.status) == [0, 2, 0]
    assert np.array_equal(r.nodes[:, :4, 1], good.nodes[:, :4, 1]) and np.all(np.isnan(r.nodes[:, 4:, 1]))
    assert np.all(np.isnan(r.x_final[:, 1])) and np.isnan(r.dv[1])
    neighbours_unchanged(r)
    Kskip = K3.copy(order="F")
    Kskip[2, 6, 4, 1] = np.nan                                            # node 4 is not: the gain is never read
    r = lto.guided_flight_mass(X3, t_B(t, 3), Kskip, x0, prm, 3, with_nodes=True, ctx=gpu_ctx)
    assert list(r.status) == [0, 0, 0] and np.array_equal(r.x_final, good.x_final)


@pytest.mark.gpu
def test_a_span_out_of_steps_fails_alone(gpu_ctx):
    """max_steps = 3 per span: the lane whose one span is 4 TU long runs out; its neighbours, whose span is 1e-4 TU, take fewer and
    are bit for bit what they are with the default limit."""
    fx = GM.LONG_FIX
    XC, _ = GM.fix_extremal(fx)
    X2 = np.asfortranarray(np.repeat(np.asarray(XC)[:, [0, 32]][:, :, None], 3, axis=2))
    t = np.asfortranarray(np.array([[0.0, 0.0, 0.0], [1e-4, 4.0, 1e-4]]))
    K = np.zeros((7, 7, 1, 3), order="F")
    x0 = np.asfortranarray(np.stack([_start(fx, 1e-4 * (b + 1)) for b in range(3)], axis=1))
    good = lto.guided_flight_mass(X2, t, K, x0, GM.fix_prm(fx), 1, ctx=gpu_ctx)
    assert np.all(good.status == 0) and good.accepted[1] + good.rejected[1] > 3 >= good.accepted[0] + good.rejected[0]
    r = lto.guided_flight_mass(X2, t, K, x0, GM.fix_prm(fx), 1, integ=lto.integrator(max_steps=3), ctx=gpu_ctx)
    assert list(r.status) == [0, 2, 0] and np.all(np.isnan(r.x_final[:, 1])) and np.isnan(r.dv[1])
    for b in (0, 2):
        assert np.array_equal(r.x_final[:, b], good.x_final[:, b]) and r.dv[b] == good.dv[b]


# ----------------------------------------------------------------------------------------- E, a converged transfer
ISP_DEMO = 2000.0


@functools.lru_cache(maxsize=None)
def _demo_solution():
    spec = importlib.util.spec_from_file_location("halo_demo", os.path.join(ROOT, "examples", "halo_transfer_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    XC, t, _, flag = demo.solve_p2(verbose=False)
    assert flag == 0
    X14, _, flag = drivers.multiShoot_CRTBP_indirect_mass(drivers.lift_to_mass(XC, 1e3), t, MU, DU, TU, XC.shape[1], ISP_DEMO, 10.0,
                                                          False, False, 50, 2.0, 1.0, verbose=False)
    assert flag == 0
    return X14, t, (MU, DU, TU, 10.0, ISP_DEMO, 1.0, 2.0, 1.0)


@pytest.mark.gpu
def test_demo_dispersion_guided_mass(gpu_ctx):
    """The 30-node demo transfer solved with variable mass, 256 starts dispersed by 1 km and 1 cm/s per axis, the same draws open
    loop and guided with an update at every node.  Sample 0 (the nominal start) arrives on the nominal's last node to the solve's
    own defect -- bar 10 max(max |defect|, 1e-12), the mass row relative to m0; every other sample's guided miss is below its
    open-loop miss.  The propellant excess is reported."""
    XC, t, prm = _demo_solution()
    open_loop = drivers.dispersion(gpu_ctx, XC, t, prm, 256, 1.0, 0.01, seed=11)
    guided = drivers.dispersion_guided_mass(gpu_ctx, XC, t, prm, 256, 1.0, 0.01, seed=11)
    assert np.array_equal(open_loop["x0"], guided["x0"])
    assert np.all(guided["status"] == 0) and np.all(open_loop["status"] == 0) and guided["gain_status"] == 0
    defect, _ = lto.indirect_defectCalc(XC, t, lto.make_params(*prm), ctx=gpu_ctx)
    level = max(float(np.max(np.abs(defect[GM.IDX12]))), float(np.max(np.abs(defect[6]))) / GM.M0, 1e-12)
    miss0 = float(np.max(np.abs(guided["x_final"][:6, 0] - XC[:6, -1])))
    po, pg = open_loop["percentiles"], guided["percentiles"]
    print("MEASURED 14-row demo guided: sample 0 misses by %.3e (defect level %.3e), lambda_m(tf) %.3e, smallest pivot ratio %.2e, "
          "nominal dv %.4f m/s, nominal propellant %.6f kg (solution %.6f kg)" % (
              miss0, level, guided["lam_final"][6, 0], float(np.min(guided["pivot"])), guided["dv_nominal_ms"],
              guided["propellant_nominal_kg"], XC[6, 0] - XC[6, -1]))
    for q in (50, 95, 99):
        print("MEASURED 14-row demo %d %%: open loop %.6g km %.6g m/s; guided %.6g km %.6g m/s, dv excess %.6g m/s, propellant excess "
              "%.6g kg" % (q, po["miss_r_km"][q], po["miss_v_ms"][q], pg["miss_r_km"][q], pg["miss_v_ms"][q], pg["dv_excess_ms"][q],
                           pg["propellant_excess_kg"][q]))
    assert miss0 <= 10.0 * level
    assert guided["dv_excess_ms"][0] == 0.0 and guided["propellant_excess_kg"][0] == 0.0
    assert np.all(guided["miss_r_km"][1:] < open_loop["miss_r_km"][1:])


# ------------------------------------------------------------------------------------------------- Isp = infinity
@pytest.mark.gpu
@pytest.mark.parametrize("fx", (GM.P2_FIX[0], GM.P1_FIX, GM.P15_FIX), ids=_id)
def test_isp_infinity_reduces_to_the_12_row_gains(gpu_ctx, fx):
    """Isp = 1e30: the device's K[0:6, 0:6] against the device's 12-row gains of the same fixture, relative to max |K_k|.  Bar:
    max(1e-12, 10 x the difference of the two CPU longdouble recurrences on the device's two Phi arrays) -- what the two sweeps'
    own Phi differ by, carried through the recurrence."""
    X14, t = GM.fix_extremal(fx, 1e30)
    X12, t12 = G.fix_extremal(fx)
    assert np.array_equal(t, t12)
    p14, p12 = GM.fix_prm(fx, 1e30), G.fix_prm(fx)
    g14 = lto.guidance_gains_mass(X14, t, p14, ctx=gpu_ctx)
    g12 = lto.guidance_gains(X12, t, p12, ctx=gpu_ctx)
    assert g14.status == 0 and g12.status == 0
    Phi14, _ = lto.indirect_stm(X14, t, lto.make_params(*p14), ctx=gpu_ctx)
    Phi12, _ = lto.indirect_stm(X12, t, lto.make_params(*p12), ctx=gpu_ctx)
    K14 = GM.recurrence(Phi14, np.longdouble)[0][0:6, 0:6].astype(np.float64)
    K12 = G.recurrence(Phi12, np.longdouble)[0].astype(np.float64)
    scale = np.max(np.abs(K12), axis=(0, 1))
    e_cpu = float(np.max(np.max(np.abs(K14 - K12), axis=(0, 1)) / scale))
    bar = max(1e-12, 10.0 * e_cpu)
    rel = float(np.max(np.max(np.abs(g14.K[0:6, 0:6] - g12.K), axis=(0, 1)) / scale))
    print("MEASURED 14-row Isp = inf %s: device K[0:6, 0:6] against the device's 12-row gains %.3e (bar %.1e; the CPU recurrences on "
          "the two device Phi differ by %.3e)" % (_id(fx), rel, bar, e_cpu))
    assert rel <= bar
    fl = lto.guided_flight_mass(X14, t, g14.K, X14[:7, 0] + GM.start_error(fx, 1e-4) * (np.arange(7) < 6), p14, 3, with_nodes=True, ctx=gpu_ctx)
    assert fl.status == 0 and np.all(fl.nodes[6] == GM.M0)                      # nothing burns: the mass stays, bit for bit
