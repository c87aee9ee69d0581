"""Linear covariance of guided flights on the device (k_guidance_covariance, lto_guidance_covariance_batch) against
tests/covariance_reference.py, which tests/test_guidance_covariance_host.py admits on the CPU:
A  P_nodes, P_final and cov_status bit for bit the plain loops run on the call's own Phi and K; K, pivot and gain_status bit for
   bit those of guidance_gains / guidance_gains_mass;
B  batches with own grids and parameters, three classes: every (trajectory, case) pair bit for bit its single call;
C  the covariance assembled from central differences of the DEVICE's guided flights, bar 1e-6 in the sigma-scaled measure;
D  a singular trajectory between regular ones, a poisoned case, sentinels, NULL outputs, refusals;
E  the demo transfer: 4 096 draws of dispersion_guided against covariance_guided."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

import lowthrustopt_amd as lto
import covariance_reference as CR
import guidance_mass_reference as GM
import guidance_reference as G
from lowthrustopt_amd import drivers
from lowthrustopt_amd.constants import MU, DU, TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_id = GM.fix_id
DOP, RK4 = "dop853", "rk4x64"


def _integ(method):
    return lto.integrator(lto.RK4, steps=64) if method == RK4 else lto.integrator()


def _mod(nx):
    return G if nx == 6 else GM


def _cases(nx, every, seed, skew=0.05):
    """P0, R [nx x nx x n_cases] -- full, each with an antisymmetric part for the call to remove, a different pair per case."""
    sig = CR.start_sigmas(nx, DU, TU)
    P0 = np.asfortranarray(np.stack([CR.spd(sig, seed + 10 * i, skew) for i in range(len(every))], axis=2))
    R = np.asfortranarray(np.stack([CR.spd(0.1 * sig, seed + 10 * i + 5, skew) for i in range(len(every))], axis=2))
    return P0, R, np.array(every, dtype=np.int32)


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _check_against_loops(c, P0, R, every, label):
    """One trajectory's GuidanceCovariance (case axis kept) against the loops on its own Phi and K, bit for bit."""
    for i, ev in enumerate(every):
        P, st = CR.loops(c.Phi, c.K, P0[:, :, i], R[:, :, i], int(ev))
        assert c.cov_status[i] == st, (label, i)
        assert _same(c.P_nodes[:, :, :, i], P), (label, i, float(np.nanmax(np.abs(c.P_nodes[:, :, :, i] - P))))
        assert _same(c.P_final[:, :, i], P[:, :, -1]), (label, i)
        assert _same(c.P_nodes[:, :, -1, i], c.P_final[:, :, i])


# ----------------------------------------------------------------------------------------------- A, bitwise against the loops
A_CASES = [
    (G.SMALL_FIX[0], 6, DOP, (1,)),
    (G.SMALL_FIX[0], 7, RK4, (0, 1)),
    (G.SMALL_FIX[1], 7, DOP, (0, 1, 3)),
    (G.SMALL_FIX[2], 6, RK4, (0, 1, 3, 8)),
    (G.P2_FIX[0], 7, RK4, (0, 1, 3, 8, 100)),
    (G.P2_FIX[1], 6, DOP, (0, 1, 3, 8, 100, 2, 4, 7, 1)),
    (G.LONG_FIX, 6, DOP, (1, 8, 100)),
    (G.LONG_FIX, 7, DOP, (3,)),
    (G.P1_FIX, 6, DOP, (0, 1, 3)),
    (G.P1_FIX, 7, DOP, (1, 8)),
    (G.P15_FIX, 7, DOP, (1, 3, 8, 0)),
    (G.P15_FIX, 6, RK4, (1,)),
    (G.BACK_FIX, 7, DOP, (1, 100)),
    (G.BACK_FIX, 6, RK4, (3,)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("fx,nx,method,every", A_CASES, ids=lambda v: _id(v) if isinstance(v, tuple) and hasattr(v, "seed") else str(v))
def test_bitwise_against_the_loops(gpu_ctx, fx, nx, method, every):
    XC, t = _mod(nx).fix_extremal(fx)
    prm = _mod(nx).fix_prm(fx)
    P0, R, ev = _cases(nx, every, 300 + fx.seed)
    integ = _integ(method)
    c = lto.guidance_covariance(XC, t, prm, P0, R, ev, integ, with_nodes=True, with_phi=True, ctx=gpu_ctx)
    nc, n = len(every), fx.n
    assert c.P_final.shape == (nx, nx, nc) and c.P_nodes.shape == (nx, nx, n, nc) and c.cov_status.shape == (nc,)
    assert c.Phi.shape == (2 * nx, 2 * nx, n - 1) and c.K.shape == (nx, nx, n - 1)
    assert c.gain_status == 0 and np.all(c.cov_status == 0)
    label = "%s NX %d %s" % (_id(fx), nx, method)
    _check_against_loops(c, P0, R, ev, label)
    for i in range(nc):                                            # node 0: the symmetrised P0 as the header forms it
        assert np.array_equal(c.P_nodes[:, :, 0, i], 0.5 * (P0[:, :, i] + P0[:, :, i].T))
    g = (lto.guidance_gains if nx == 6 else lto.guidance_gains_mass)(XC, t, prm, integ, ctx=gpu_ctx)
    assert np.array_equal(c.K, g.K) and np.array_equal(c.pivot, g.pivot) and c.gain_status == g.status
    # Phi is what the gains were built from: the longdouble recurrence on it gives them within its bar
    K_ref, bar, _ = _mod(nx).gain_bars(c.Phi)
    assert np.all(np.max(np.abs(c.K - K_ref), axis=(0, 1)) / np.max(np.abs(K_ref), axis=(0, 1)) <= bar)
    # without the optional outputs, and a single case without its axis
    lean = lto.guidance_covariance(XC, t, prm, P0, R, ev, integ, ctx=gpu_ctx)
    assert lean.P_nodes is None and lean.Phi is None and np.array_equal(lean.P_final, c.P_final)
    one = lto.guidance_covariance(XC, t, prm, P0[:, :, 0], R[:, :, 0], int(ev[0]), integ, with_nodes=True, ctx=gpu_ctx)
    assert one.P_final.shape == (nx, nx) and one.cov_status == 0 and np.array_equal(one.P_nodes, c.P_nodes[:, :, :, 0])


# ---------------------------------------------------------------------------------------------------------------- B, batches
NINE = G.P2_FIX + (G.BACK_FIX, G.P1_FIX, G.P15_FIX)              # the regular fixtures of nine nodes: three classes, three grids
B_EVERY = (0, 1, 3)
_SINGLES = {}


def _single(ctx, nx, fx, i, P0, R, ev):
    """Trajectory fx with case i alone."""
    key = (nx, fx, i)
    if key not in _SINGLES:
        XC, t = _mod(nx).fix_extremal(fx)
        c = lto.guidance_covariance(XC, t, _mod(nx).fix_prm(fx), P0[:, :, i], R[:, :, i], int(ev[i]), with_nodes=True, ctx=ctx)
        _SINGLES[key] = (c.P_nodes.copy(), c.P_final.copy(), c.cov_status, c.K.copy(), c.pivot.copy(), c.gain_status)
    return _SINGLES[key]


def _stack(nx, fixtures):
    mod = _mod(nx)
    XC = np.asfortranarray(np.stack([mod.fix_extremal(f)[0] for f in fixtures], axis=2))
    t = np.asfortranarray(np.stack([mod.fix_extremal(f)[1] for f in fixtures], axis=1))
    return XC, t, [mod.fix_prm(f) for f in fixtures]


@pytest.mark.gpu
@pytest.mark.parametrize("nx", (6, 7))
@pytest.mark.parametrize("B", [1, 3, 64, 65])
def test_batches_are_their_single_calls(gpu_ctx, B, nx):
    """Per-trajectory grids and parameters, three control-law classes in one batch (for 14 rows the call splits it in two): every
    (trajectory, case) pair is the call with that trajectory and that case alone, bit for bit."""
    fixtures = [NINE[(3 * b + b // 11) % len(NINE)] for b in range(B)]
    XC, t, prms = _stack(nx, fixtures)
    P0, R, ev = _cases(nx, B_EVERY, 500)
    c = lto.guidance_covariance(XC, t, prms, P0, R, ev, with_nodes=True, ctx=gpu_ctx)
    assert c.P_nodes.shape == (nx, nx, 9, 3, B) and c.P_final.shape == (nx, nx, 3, B) and c.cov_status.shape == (3, B)
    assert np.all(c.cov_status == 0) and np.all(c.gain_status == 0)
    for b, fx in enumerate(fixtures):
        for i in range(3):
            Pn, Pf, st, K, piv, gs = _single(gpu_ctx, nx, fx, i, P0, R, ev)
            assert np.array_equal(c.P_nodes[:, :, :, i, b], Pn) and np.array_equal(c.P_final[:, :, i, b], Pf), (b, i, fx)
            assert c.cov_status[i, b] == st and c.gain_status[b] == gs
            assert np.array_equal(c.K[:, :, :, b], K) and np.array_equal(c.pivot[:, b], piv)


# ------------------------------------------------------------------------------------- C, central differences on the device
C_FIX = {6: (G.P2_FIX[0], G.P2_FIX[4]), 7: (GM.P2_FIX[0], GM.P2_FIX[4])}       # 14 rows: the two the CPU reference resolves


@pytest.mark.gpu
@pytest.mark.parametrize("method", (DOP, RK4))
@pytest.mark.parametrize("nx", (6, 7))
def test_central_differences_of_device_flights(gpu_ctx, nx, method):
    """P_k = G_0 P0 G_0^T + sum_j G_j R G_j^T from the device's own guided flights (eps = 1e-6, 14 rows: times X_SCALE), one
    flight call per fixture and cadence, under the gains the covariance call returns.  Bar 1e-6 of sigma_i sigma_j: every node for
    12 rows, the arrival node for 14."""
    integ = _integ(method)
    flight = lto.guided_flight if nx == 6 else lto.guided_flight_mass
    scale = None if nx == 6 else GM.X_SCALE
    worst = 0.0
    for fx in C_FIX[nx]:
        XC, t = _mod(nx).fix_extremal(fx)
        prm = _mod(nx).fix_prm(fx)
        P0, R, ev = _cases(nx, (0, 1, 3), 700 + fx.seed, skew=0.0)
        c = lto.guidance_covariance(XC, t, prm, P0, R, ev, integ, with_nodes=True, ctx=gpu_ctx)
        assert np.all(c.cov_status == 0)
        for i, every in enumerate(ev):
            dx0, nav = CR.cd_perturbations(nx, fx.n, int(every), scale)
            x0 = np.asfortranarray(XC[:nx, :1] + dx0)
            r = flight(XC, t, c.K, x0, prm, int(every), nav if every > 0 else None, integ, with_nodes=True, ctx=gpu_ctx)
            assert np.all(r.status == 0)
            cd = CR.cd_assemble(r.nodes, fx.n, int(every), P0[:, :, i], R[:, :, i], scale)
            nodes = slice(None) if nx == 6 else slice(fx.n - 1, fx.n)
            err = float(np.max(CR.sigma_scaled_error(c.P_nodes[:, :, nodes, i], cd[:, :, nodes])))
            print("MEASURED covariance against device differences, NX %d %s %s every %d: %.3e (bar 1e-6)" % (nx, method, _id(fx), every, err))
            worst = max(worst, err)
    assert worst <= 1e-6


# ---------------------------------------------------------------------------------------- D, singular and poisoned inputs
@pytest.mark.gpu
@pytest.mark.parametrize("nx", (6, 7))
def test_a_singular_trajectory_between_regular_neighbours(gpu_ctx, nx):
    """p = 0 has no gains (gain_status 3, K all NaN): its update_every = 0 case never reads one and is valid, its updating cases are
    status 2 with NaN from node 1 on; the neighbours are bit for bit their single calls."""
    sing, left, right = _mod(nx).P0_FIX[0], NINE[1], NINE[10]
    XC, t, prms = _stack(nx, [left, sing, right])
    P0, R, ev = _cases(nx, B_EVERY, 500)
    c = lto.guidance_covariance(XC, t, prms, P0, R, ev, with_nodes=True, with_phi=True, ctx=gpu_ctx)
    assert list(c.gain_status) == [0, 3, 0] and np.all(np.isnan(c.K[:, :, :, 1]))
    assert [list(c.cov_status[:, b]) for b in range(3)] == [[0, 0, 0], [0, 2, 2], [0, 0, 0]]
    P, st = CR.loops(c.Phi[:, :, :, 1], c.K[:, :, :, 1], P0[:, :, 0], R[:, :, 0], 0)
    assert st == 0 and np.array_equal(c.P_nodes[:, :, :, 0, 1], P) and np.array_equal(c.P_final[:, :, 0, 1], P[:, :, -1])
    for i in (1, 2):
        assert np.array_equal(c.P_nodes[:, :, 0, i, 1], 0.5 * (P0[:, :, i] + P0[:, :, i].T))
        assert np.all(np.isnan(c.P_nodes[:, :, 1:, i, 1])) and np.all(np.isnan(c.P_final[:, :, i, 1]))
        assert _same(c.P_nodes[:, :, :, i, 1], CR.loops(c.Phi[:, :, :, 1], c.K[:, :, :, 1], P0[:, :, i], R[:, :, i], int(ev[i]))[0])
    for b, fx in ((0, left), (2, right)):
        for i in range(3):
            Pn, Pf, s1, K, piv, gs = _single(gpu_ctx, nx, fx, i, P0, R, ev)
            assert np.array_equal(c.P_nodes[:, :, :, i, b], Pn) and np.array_equal(c.P_final[:, :, i, b], Pf)
            assert np.array_equal(c.K[:, :, :, b], K) and np.array_equal(c.pivot[:, b], piv)


@pytest.mark.gpu
def test_a_poisoned_case_fails_alone(gpu_ctx):
    fx = G.P2_FIX[2]
    XC, t = G.fix_extremal(fx)
    prm = G.fix_prm(fx)
    every = (0, 1, 3, 1, 8)
    P0, R, ev = _cases(6, every, 900)
    good = lto.guidance_covariance(XC, t, prm, P0, R, ev, with_nodes=True, ctx=gpu_ctx)
    assert np.all(good.cov_status == 0)
    for which, case, value in (("R", 1, np.nan), ("R", 0, np.inf), ("P0", 4, np.nan), ("P0", 2, -np.inf)):
        Pb, Rb = P0.copy(order="F"), R.copy(order="F")
        (Rb if which == "R" else Pb)[2, 3, case] = value
        c = lto.guidance_covariance(XC, t, prm, Pb, Rb, ev, with_nodes=True, ctx=gpu_ctx)
        assert list(c.cov_status) == [2 if i == case else 0 for i in range(5)], (which, case)
        assert np.all(np.isnan(c.P_nodes[:, :, 1:, case])) and np.all(np.isnan(c.P_final[:, :, case]))
        node0 = 0.5 * (Pb[:, :, case] + Pb[:, :, case].T)
        assert _same(c.P_nodes[:, :, 0, case], node0)
        keep = [i for i in range(5) if i != case]
        assert np.array_equal(c.P_nodes[:, :, :, keep], good.P_nodes[:, :, :, keep])
        assert np.array_equal(c.P_final[:, :, keep], good.P_final[:, :, keep]) and np.array_equal(c.K, good.K)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _raw(ctx, ndim=12, n=9, B=2, n_tgrids=1, n_prm=1, integ=None, sing_tol=1e-10, n_cases=3, every=(0, 1, 3), null=(), pad=0, t=None):
    fx = G.P2_FIX[0]
    nx = 7 if ndim == 14 else 6
    XC, _ = _mod(nx).fix_extremal(fx)
    nd = XC.shape[0]
    nn, Bn, nc = max(n, 2), max(B, 1), max(n_cases, 1)
    X = np.asfortranarray(np.repeat(np.resize(XC, (nd, nn))[:, :, None], Bn, axis=2))
    X[:, :min(nn, 9), :] = XC[:, :min(nn, 9), None]
    tg = np.asfortranarray(np.repeat((np.linspace(0.0, 0.5, nn) if t is None else np.asarray(t, dtype=float))[:, None], max(n_tgrids, 1), axis=1))
    prms = (lto.LtoParams * max(n_prm, 1))(*[lto.make_params(*_mod(nx).fix_prm(fx))] * max(n_prm, 1))
    integ = integ or lto.integrator()
    P0, R, _ = _cases(nx, (0,) * nc, 40)
    ev = np.resize(np.array(every, dtype=np.int32), nc)
    ne = nx * nx
    out = dict(K=np.full(ne * (nn - 1) * Bn + pad, -7.0), pivot=np.full((nn - 1) * Bn + pad, -7.0),
               gain_status=np.full(Bn + pad, -7, dtype=np.int32), Phi=np.full(4 * ne * (nn - 1) * Bn + pad, -7.0),
               P_nodes=np.full(ne * nn * nc * Bn + pad, -7.0), P_final=np.full(ne * nc * Bn + pad, -7.0),
               cov_status=np.full(nc * Bn + pad, -7, dtype=np.int32))
    a = {k: (None if k in null else v) for k, v in out.items()}
    rc = ctx.lib.lto_guidance_covariance_batch(
        ctx.handle, ndim, n, B, None if "XC" in null else _p(X), None if "t" in null else _p(tg), n_tgrids,
        None if "prm" in null else prms, n_prm, None if "integ" in null else C.byref(integ), sing_tol, n_cases,
        None if "P0" in null else _p(P0), None if "R" in null else _p(R), None if "update_every" in null else _p(ev), _p(a["K"]),
        _p(a["pivot"]), _p(a["gain_status"]), _p(a["Phi"]), _p(a["P_nodes"]), _p(a["P_final"]), _p(a["cov_status"]))
    return rc, out


@pytest.mark.gpu
def test_refusals(gpu_ctx):
    down = np.linspace(0.0, 0.5, 9)
    down[4] = down[3]
    rkf = (lto.integrator(lto.RKF78_FIXED, steps=4), lto.integrator(lto.RKF78_ADAPTIVE))
    assert _raw(gpu_ctx)[0] == 0 and _raw(gpu_ctx, ndim=14)[0] == 0
    for name in ("XC", "t", "prm", "integ", "gain_status", "P0", "R", "update_every", "P_final", "cov_status"):
        assert _raw(gpu_ctx, null=(name,))[0] == -2, name
    assert gpu_ctx.lib.lto_guidance_covariance_batch(None, 12, 9, 1, None, None, 1, None, 1, None, 1e-10, 1, None, None, None, None, None,
                                                     None, None, None, None, None) == -2
    for kw in (dict(n=1), dict(B=0), dict(t=down), dict(t=down[::-1].copy()), dict(n_tgrids=0), dict(n_tgrids=3, B=2), dict(n_prm=0),
               dict(n_prm=3, B=2), dict(sing_tol=0.0), dict(sing_tol=1.0), dict(sing_tol=float("nan")), dict(n_cases=0),
               dict(n_cases=-1), dict(every=(0, 1, -1)), dict(every=(-3,), n_cases=1)):
        assert _raw(gpu_ctx, **kw)[0] == -1, kw
    for kw in (dict(ndim=6), dict(ndim=13), dict(integ=rkf[0]), dict(integ=rkf[1]), dict(ndim=14, integ=rkf[1])):
        assert _raw(gpu_ctx, **kw)[0] == -3, kw
    assert _raw(gpu_ctx, n=2, n_cases=1, every=(1,))[0] == 0
    with pytest.raises(lto.LtoError) as ei:
        lto.guidance_covariance(G.fix_extremal(G.P2_FIX[0])[0], np.linspace(0.0, 0.5, 9), G.fix_prm(G.P2_FIX[0]), np.eye(6), np.eye(6), 1,
                                lto.integrator(lto.RKF78_ADAPTIVE), ctx=gpu_ctx)
    assert ei.value.code == -3


@pytest.mark.gpu
@pytest.mark.parametrize("ndim", (12, 14))
def test_outputs_stay_inside_their_extents_and_optional_ones_may_be_null(gpu_ctx, ndim):
    ne = (ndim // 2) ** 2
    for n_cases in (3, 5):
        rc, full = _raw(gpu_ctx, ndim=ndim, B=3, n_cases=n_cases, pad=5)
        assert rc == 0 and np.all(full["cov_status"][:n_cases * 3] == 0) and np.all(full["gain_status"][:3] == 0)
        extents = dict(K=ne * 8 * 3, pivot=8 * 3, gain_status=3, Phi=4 * ne * 8 * 3, P_nodes=ne * 9 * n_cases * 3, P_final=ne * n_cases * 3,
                       cov_status=n_cases * 3)
        for k, n in extents.items():
            assert np.all(full[k][n:] == -7) and not np.any(full[k][:n] == -7), k
        optional = ("K", "pivot", "Phi", "P_nodes")
        rc, part = _raw(gpu_ctx, ndim=ndim, B=3, n_cases=n_cases, pad=5, null=optional)
        assert rc == 0
        for k in extents:
            assert np.all(part[k] == -7) if k in optional else np.array_equal(part[k], full[k]), k
        for name in optional:                                      # and one at a time
            rc, part = _raw(gpu_ctx, ndim=ndim, B=3, n_cases=n_cases, pad=5, null=(name,))
            assert rc == 0 and np.all(part[name] == -7)
            assert all(np.array_equal(part[k], full[k]) for k in extents if k != name), name


# ------------------------------------------------------------------------------------------------- E, the demo transfer
@functools.lru_cache(maxsize=None)
def _demo_solution():
    spec = importlib.util.spec_from_file_location("halo_demo", os.path.join(ROOT, "examples", "halo_transfer_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    XC, t, _, flag = demo.solve_p2(verbose=False)
    assert flag == 0
    return XC, t, (MU, DU, TU, 10.0, 1e3, 1.0, 2.0, 1.0)


@pytest.mark.gpu
def test_demo_transfer_against_its_monte_carlo(gpu_ctx):
    """The 30-node demo transfer, starts dispersed by 1 km and 1 cm/s per axis, navigation errors of 0.1 km and 1 mm/s at every
    update: 4 096 draws of dispersion_guided (sample 0 is the undisturbed one, 4 095 count) against covariance_guided, an update at
    every node and at every third.  Every diagonal element of the sample covariance about the nominal arrival within
    5 sqrt(2 / 4095) of P_final, every sample mean within 5 sigma / sqrt(N) of zero."""
    XC, t, prm = _demo_solution()
    N = 4096
    cov = drivers.covariance_guided(gpu_ctx, XC, t, prm, 1.0, 0.01, update_every=np.array([1, 3]), nav_sigma_r_km=0.1,
                                    nav_sigma_v_ms=1e-3)
    assert np.all(cov["cov_status"] == 0) and cov["gain_status"] == 0 and cov["P_final"].shape == (6, 6, 2)
    for i, every in enumerate((1, 3)):
        mc = drivers.dispersion_guided(gpu_ctx, XC, t, prm, N, 1.0, 0.01, seed=11, update_every=every, nav_sigma_r_km=0.1,
                                       nav_sigma_v_ms=1e-3, nav_seed=12)
        assert np.all(mc["status"] == 0)
        d = mc["x_final"][:, 1:] - XC[:6, -1:]
        var = np.diag(cov["P_final"][:, :, i])
        ratio = np.mean(d * d, axis=1) / var
        mean = np.mean(d, axis=1) / np.sqrt(var / (N - 1))
        s_r = np.sqrt(np.mean(np.sum(d[0:3] ** 2, axis=0))) * DU
        s_v = np.sqrt(np.mean(np.sum(d[3:6] ** 2, axis=0))) * DU / TU * 1e3
        print("MEASURED demo covariance, update_every %d: sigma_r %.6g km (sample %.6g), sigma_v %.6g m/s (sample %.6g), largest "
              "principal sigma_r %.6g km; variance ratios %s, means in sigma / sqrt(N) %s" % (
                  every, cov["miss_r_km_rss"][i], s_r, cov["miss_v_ms_rss"][i], s_v, cov["miss_r_km_max"][i],
                  np.array2string(ratio, precision=3), np.array2string(mean, precision=2)))
        assert np.all(np.abs(ratio - 1.0) <= 5.0 * np.sqrt(2.0 / (N - 1)))
        assert np.all(np.abs(mean) <= 5.0)
