"""CPU: the model behind lto_guidance_covariance_batch, checked with the oracle and numpy only, and the parts of the
binding that need no device.

* the plain loops of covariance_reference (the header's binary64 order, what the device is held to bit for bit) against the same
  recursion in longdouble: per node, relative to that node's largest |P|, at most 1e-11 on every regular fixture (the cancellation
  A + B K at the last update is what is left of float64 gains: up to 1.3e-12 measured);
* the closed form of update_every = 1, A R A^T, to 1e-13;
* the covariance assembled from central differences of the ORACLE's guided flights, to 2.5e-7 in the sigma-scaled measure -- every
  node of the 12-row p = 2 fixtures, the arrival node of two 14-row ones;
* 2 048 oracle flights with drawn starts and navigation errors: the sample variances within 5 sqrt(2 / N) of the recursion;
* the drivers' unit arithmetic and the shape checks of hotpath.guidance_covariance."""
import numpy as np
import pytest

import lowthrustopt_amd as lto
from lowthrustopt_amd import _lib, drivers, hotpath

import covariance_reference as CR
import guidance_mass_reference as GM
import guidance_reference as G

EVERY = (0, 1, 3)
CD_FIX12 = G.P2_FIX + G.SMALL_FIX + (G.BACK_FIX,)
# The two 14-row fixtures.  The differences perturb the mass by eps m0 = 1e-3 kg, far below the 0.1 .. 1 kg of the covariances, so
# the rounding of the oracle's flights (about 1e-14 in r and v) enters the mass column of G as 1e-14 / 2e-3 per kg and the (r, m)
# and (v, m) elements at 1e-8 .. 1e-6 of sigma_i sigma_j, fixture by fixture; a smaller eps makes it worse (measured), a smaller
# mass sigma hands the same elements to the truncation of the free final mass instead (the costate moves by K eps, about 0.1).
# Arrival node, loops against the oracle's differences, update_every = 0 / 1 / 3, the (r, v) blocks all at or below 6.2e-10:
#   P2_FIX[0] 7.3e-8 1.3e-7 7.1e-8   [1] 5.3e-8 5.6e-7 2.2e-7   [2] 4.6e-8 3.6e-8 3.3e-7   [3] 2.1e-8 6.4e-7 1.1e-6
#   P2_FIX[4] 1.2e-8 4.2e-8 2.3e-7   [5] 2.3e-8 5.1e-8 5.9e-7   [6] 5.0e-8 3.1e-7 1.7e-7   [7] 5.3e-8 3.4e-7 3.1e-7
# The reference resolves the bar at all three cadences on fixtures 0 and 4 only; these two are used here and on the device.
CD_FIX14 = (GM.P2_FIX[0], GM.P2_FIX[4])
CD_BAR = 2.5e-7


def inputs(fx, nx):
    """(XC, t, prm, Phi, K, P0, R) of a fixture: the oracle's STMs, the reference gains, a full start covariance with sigmas about
    1 km, 1 cm/s (and 1 kg) and a full navigation covariance of a tenth of that (covariance_reference.start_sigmas)."""
    mod = G if nx == 6 else GM
    XC, t = mod.fix_extremal(fx)
    sig = CR.start_sigmas(nx, lto.DU, lto.TU)
    return (XC, t, mod.fix_prm(fx), mod.fix_phi(fx), mod.fix_gains(fx), CR.spd(sig, 7 + fx.seed), CR.spd(0.1 * sig, 107 + fx.seed))


@pytest.mark.parametrize("nx", (6, 7))
@pytest.mark.parametrize("fx", G.REGULAR_FIX, ids=GM.fix_id)
def test_loops_against_longdouble(fx, nx):
    _, _, _, Phi, K, P0, R = inputs(fx, nx)
    worst = 0.0
    for every in EVERY:
        P, status = CR.loops(Phi, K, P0, R, every)
        assert status == 0
        err = CR.node_error(P, CR.recursion_ld(Phi, K, P0, R, every))
        worst = max(worst, float(err.max()))
        assert np.array_equal(P, np.swapaxes(P, 0, 1))            # symmetric bit for bit
    print("loops vs longdouble, NX = %d, %s: %.2e" % (nx, GM.fix_id(fx), worst))
    assert worst <= 1e-11


def test_loops_statuses():
    _, _, _, Phi, K, P0, R = inputs(G.P2_FIX[1], 6)
    n = Phi.shape[2] + 1
    Pn, st = CR.loops(Phi, K, P0, R, 0)
    Kbad = np.array(K)
    Kbad[2, 3, 4] = np.nan                                         # node 4 updates for every = 1 and 2, not for 3
    for every, dead_from in ((0, None), (1, 5), (2, 5), (3, None)):
        P, st = CR.loops(Phi, Kbad, P0, R, every)
        assert st == (0 if dead_from is None else 2)
        fin = np.all(np.isfinite(P), axis=(0, 1))
        assert np.array_equal(fin, np.arange(n) < (n if dead_from is None else dead_from))
    Phibad = np.array(Phi)
    Phibad[0, 0, 2] = np.inf
    P, st = CR.loops(Phibad, K, P0, R, 0)
    assert st == 2 and np.array_equal(np.all(np.isfinite(P), axis=(0, 1)), np.arange(n) < 3)
    Rbad = np.array(R)
    Rbad[1, 2] = np.nan
    P, st = CR.loops(Phi, K, P0, Rbad, 0)
    assert st == 2 and np.array_equal(P[:, :, 0], 0.5 * (P0 + P0.T)) and np.all(np.isnan(P[:, :, 1:]))


@pytest.mark.parametrize("nx", (6, 7))
@pytest.mark.parametrize("fx", G.REGULAR_FIX, ids=GM.fix_id)
def test_closed_form(fx, nx):
    """update_every = 1: the arrival covariance of (r, v) is A R A^T whatever P0 is -- with the gains in longdouble, so that what is
    compared is the model and not float64's A + B K."""
    mod = G if nx == 6 else GM
    _, _, _, Phi, _, P0, R = inputs(fx, nx)
    K = mod.recurrence(Phi, np.longdouble)[0]
    ref = CR.closed_form(Phi, R)
    scale = np.max(np.abs(ref))
    for P_start in (P0, 4.0 * P0, np.zeros_like(P0)):       # the cancellation grows with |P0| / |R|
        P = CR.recursion_ld(Phi, K, P_start, R, 1)[0:6, 0:6, -1]
        err = float(np.max(np.abs(P - ref)) / scale)
        assert err <= 1e-13, err


def oracle_cd(fx, nx, every, P0, R):
    """P_nodes from central differences of the oracle's guided flights of a fixture."""
    mod = G if nx == 6 else GM
    XC, t = mod.fix_extremal(fx)
    K, prm = mod.fix_gains(fx), mod.fix_prm(fx)
    n = XC.shape[1]
    scale = None if nx == 6 else GM.X_SCALE
    dx0, nav = CR.cd_perturbations(nx, n, every, scale)
    M = dx0.shape[1]
    nodes = np.empty((nx, n, M))
    for m in range(M):
        g = mod.fly(XC, t, K, XC[:nx, 0] + dx0[:, m], prm, every, nav[:, :, m] if every > 0 else None)
        assert g.ok
        nodes[:, :, m] = g.nodes
    return CR.cd_assemble(nodes, n, every, P0, R, scale)


@pytest.mark.parametrize("fx", CD_FIX12, ids=GM.fix_id)
def test_central_differences_12(fx):
    _, _, _, Phi, K, P0, R = inputs(fx, 6)
    for every in EVERY:
        P, status = CR.loops(Phi, K, P0, R, every)
        assert status == 0
        cd = oracle_cd(fx, 6, every, P0, R)
        err = CR.sigma_scaled_error(P, cd)
        print("central differences, 12 rows, %s, every %d: %.2e" % (GM.fix_id(fx), every, err.max()))
        assert err.max() <= CD_BAR
        assert np.allclose(cd[:, :, 0], 0.5 * (P0 + P0.T), rtol=1e-9, atol=0.0)


@pytest.mark.parametrize("fx", CD_FIX14, ids=GM.fix_id)
def test_central_differences_14_arrival(fx):
    _, _, _, Phi, K, P0, R = inputs(fx, 7)
    for every in EVERY:
        P, status = CR.loops(Phi, K, P0, R, every)
        assert status == 0
        cd = oracle_cd(fx, 7, every, P0, R)
        err = float(CR.sigma_scaled_error(P[:, :, -1], cd[:, :, -1]))
        print("central differences, 14 rows, %s, every %d, arrival: %.2e" % (GM.fix_id(fx), every, err))
        assert err <= CD_BAR


@pytest.mark.parametrize("every", EVERY)
def test_monte_carlo(every):
    """2 048 oracle flights of P2_FIX[0] with starts drawn from P0 and navigation errors from R: every diagonal element of the
    sample covariance about the nominal arrival within 5 sqrt(2 / N) of the recursion's."""
    fx, N = G.P2_FIX[0], 2048
    XC, t, prm, Phi, K, P0, R = inputs(fx, 6)
    n = XC.shape[1]
    nu = CR.n_updates(n, every)
    rng = np.random.default_rng(2024 + every)
    L0, LR = np.linalg.cholesky(0.5 * (P0 + P0.T)), np.linalg.cholesky(0.5 * (R + R.T))
    d = np.empty((6, N))
    for s in range(N):
        x0 = XC[:6, 0] + L0 @ rng.standard_normal(6)
        nav = LR @ rng.standard_normal((6, nu)) if nu else None
        g = G.fly(XC, t, K, x0, prm, every, nav, 1e-12)
        assert g.ok
        d[:, s] = g.x_final - XC[:6, -1]
    P, status = CR.loops(Phi, K, P0, R, every)
    assert status == 0
    ratio = np.mean(d * d, axis=1) / np.diag(P[:, :, -1])
    print("Monte Carlo, every %d: variance ratios %s" % (every, np.array2string(ratio, precision=3)))
    assert np.all(np.abs(ratio - 1.0) <= 5.0 * np.sqrt(2.0 / N))


def test_driver_unit_arithmetic():
    DU, TU = lto.DU, lto.TU
    P = np.zeros((7, 7, 2))
    P[0, 0, 0], P[1, 1, 0], P[2, 2, 0] = (3.0 / DU) ** 2, (4.0 / DU) ** 2, (12.0 / DU) ** 2          # km
    P[3, 3, 0] = P[4, 4, 0] = P[5, 5, 0] = (2.0 / 1e3 * TU / DU) ** 2                                  # m/s
    P[6, 6, 0] = 0.25
    P[:, :, 1] = P[:, :, 0]
    P[0, 0, 1] = -1e-30                                             # a rounded-off negative variance is a zero
    P[6, 6, 1] = np.nan
    s = drivers.covariance_sigmas(P, DU, TU)
    assert s["sigma_r_km"][0] == pytest.approx(13.0, rel=1e-14)
    assert s["sigma_r_max_km"][0] == pytest.approx(12.0, rel=1e-12)
    assert s["sigma_v_ms"][0] == pytest.approx(2.0 * np.sqrt(3.0), rel=1e-14)
    assert s["sigma_m_kg"][0] == 0.5 and np.isnan(s["sigma_m_kg"][1])
    assert s["sigma_r_km"][1] == pytest.approx(np.sqrt(160.0), rel=1e-14)
    s6 = drivers.covariance_sigmas(P[:6, :6, 0], DU, TU)
    assert "sigma_m_kg" not in s6 and float(s6["sigma_r_km"]) == pytest.approx(13.0, rel=1e-14)
    # a rotated position block: the largest principal sigma is not on the diagonal
    Q = np.zeros((6, 6))
    Q[0:3, 0:3] = np.array([[2.0, 1.0, 0.0], [1.0, 2.0, 0.0], [0.0, 0.0, 0.5]]) / DU ** 2
    assert float(drivers.covariance_sigmas(Q, DU, TU)["sigma_r_max_km"]) == pytest.approx(np.sqrt(3.0), rel=1e-12)
    nanP = np.full((6, 6), np.nan)
    assert all(np.isnan(v) for v in drivers.covariance_sigmas(nanP, DU, TU).values())
    # the diagonal inputs are those of dispersion_starts and guided_nav
    D = drivers.covariance_diag(7, 1.0, 0.01, 0.5, DU, TU)
    x0 = drivers.dispersion_starts(np.zeros(6), 3, 1.0, 0.01, 5, DU, TU)
    z = np.random.default_rng(5).standard_normal((6, 3))
    assert np.allclose(np.sqrt(np.diag(D))[:6, None] * z[:, 1:], x0[:, 1:], rtol=1e-15, atol=0.0)
    assert D[6, 6] == 0.25 and np.count_nonzero(D - np.diag(np.diag(D))) == 0
    assert np.array_equal(drivers.covariance_diag(6, None, None, None, DU, TU), np.zeros((6, 6)))


def test_binding_and_shape_checks():
    name = "lto_guidance_covariance_batch"
    assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 22
    assert hasattr(lto.load_library(), name) and lto.load_library().lto_version() == 102
    XC, t, prm, _, _, P0, R = inputs(G.P2_FIX[0], 6)
    p = lto.make_params(*prm)
    bad = [
        dict(P0=P0[:5, :], R=R),                                   # not square
        dict(P0=P0[:, :5], R=R),
        dict(P0=P0, R=R[:5, :5]),
        dict(P0=np.zeros((7, 7)), R=np.zeros((7, 7))),             # 14-row cases for a 12-row solution
        dict(P0=np.zeros((6, 6, 2)), R=np.zeros((6, 6, 3))),
        dict(P0=np.zeros((6, 6, 2)), R=np.zeros((6, 6, 2)), update_every=[1, 2, 3]),
        dict(P0=np.zeros((6, 6, 2)), R=np.zeros((6, 6, 2)), update_every=1),
        dict(P0=P0, R=R, update_every=-1),
        dict(P0=np.zeros((6, 6, 2)), R=np.zeros((6, 6, 2)), update_every=[1, -2]),
        dict(P0=P0, R=R, update_every=1.5),
        dict(P0=np.zeros((6, 6, 0)), R=np.zeros((6, 6, 0)), update_every=[]),
    ]
    for kw in bad:
        kw.setdefault("update_every", 1)
        with pytest.raises(ValueError):
            hotpath.guidance_covariance(XC, t, p, **kw)
    with pytest.raises(ValueError):
        hotpath.guidance_covariance(XC[:11], t, p, P0, R, 1)
    with pytest.raises(ValueError):
        hotpath.guidance_covariance(XC, t[:-1], p, P0, R, 1, ctx=object())
    assert lto.guidance_covariance is hotpath.guidance_covariance
