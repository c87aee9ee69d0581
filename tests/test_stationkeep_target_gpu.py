"""GPU checks of the target-point station-keeping calls (lto_halo_stm_batch, lto_stationkeep_target_gains_batch and the driver above
them) against the independent host reference (tests/stationkeep_target_reference.py: scipy DOP853 at rtol 1e-13 / atol
1e-14 with one solve per span for the STMs, plain loops in the header's order for the gains).  Every bound is a named constant of
tests/test_stationkeep_target_host.py, which holds the reference's own spread to a tenth of it; the gains are compared bit for bit.
The shapes are the smallest that can still go wrong: 1 and 3 phases (the uneven 0.1, 0.35, 0.8), 1 and 2 horizons, 1, 2 and 3 orbits
(packaged orbits 1, 2, 1: 9 records cross the 8-records-per-block edge and leave a ragged tail), 65 records for the one-lane gains
kernel (65 crosses the 64-lane block).

Figures measured on an MI355X are in DESIGN 4.30."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import manifold_reference as MR  # noqa: E402
import stationkeep_reference as SR  # noqa: E402
import stationkeep_target_reference as TR  # noqa: E402
import test_stationkeep_target_host as H  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import _lib, drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402

pytestmark = pytest.mark.gpu

ORBITS3 = (0, 1, 0)                                  # packaged orbits 1, 2, 1
STM_FIELDS = ("X", "Phi", "X_tgt", "accepted", "rejected", "status")


@pytest.fixture(scope="module")
def orbits():
    return MR.packaged_orbits(synth.halo_orbits(), MU)


def _integ(**kw):
    return lto.integrator(rtol=TR.RTOL, atol=TR.ATOL, **kw)


def _inputs(orbits, ks):
    return (np.stack([orbits[k][0] for k in ks], axis=1), np.array([orbits[k][1] for k in ks]))


def _stm(ctx, orbits, ks, taus, horizons, integ=None):
    s0, per = _inputs(orbits, ks)
    return lto.halo_stm(s0, per, taus, horizons, MU=MU, integ=integ or _integ(), ctx=ctx)


@pytest.fixture(scope="module")
def nine(gpu_ctx, orbits):
    """The 9-record call (3 phases x 3 orbits, 2 horizons) several tests read; flown once and left unchanged."""
    return _stm(gpu_ctx, orbits, ORBITS3, TR.TAUS3, TR.HORIZONS)


# ---------------------------------------------------------------------------------------------------------------- 1. the STM call
@pytest.mark.parametrize("P,K,B", [(1, 1, 1), (3, 2, 1), (1, 2, 2), (3, 1, 2), (3, 2, 3)])
def test_stm_against_the_reference(gpu_ctx, orbits, P, K, B):
    taus, hz, ks = TR.TAUS3[:P], TR.HORIZONS[:K], ORBITS3[:B]
    ref = TR.stms(orbits, ks, taus, hz, MU)
    r = _stm(gpu_ctx, orbits, ks, taus, hz)
    dx, dxt, dphi = np.abs(r.X - ref.X).max(), np.abs(r.X_tgt - ref.X_tgt).max(), H.rel_block(r.Phi, ref.Phi)
    print("%d phases x %d horizons x %d orbits: X %.2e, X_tgt %.2e, Phi %.2e (relative); steps %d..%d, rejected <= %d"
          % (P, K, B, dx, dxt, dphi, r.accepted.min(), r.accepted.max(), r.rejected.max()))
    assert r.X.shape == (6, P, B) and r.Phi.shape == (6, 6, K, P, B) and r.X_tgt.shape == (6, K, P, B) and r.status.shape == (P, B)
    assert np.all(r.status == 0) and np.array_equal(r.tau, taus) and np.array_equal(r.horizons, hz)
    assert dx <= H.GPU_X and dxt <= H.GPU_X_TGT and dphi <= H.GPU_PHI
    if B == 1:                                               # a single orbit without the batch axis
        s = lto.halo_stm(orbits[0][0], orbits[0][1], taus, hz, MU=MU, integ=_integ(), ctx=gpu_ctx)
        assert s.Phi.shape == (6, 6, K, P) and np.array_equal(s.Phi, r.Phi[..., 0]) and np.array_equal(s.X, r.X[..., 0])


def test_device_stms_are_symplectic_and_compose(gpu_ctx, orbits, nine):
    worst = 0.0
    for b in range(3):
        for j in range(3):
            for h in range(2):
                Phi = nine.Phi[:, :, h, j, b]
                worst = max(worst, np.abs(Phi.T @ SR.S @ Phi - SR.S).max() / np.abs(Phi).max() ** 2)
    a = _stm(gpu_ctx, orbits, (0,), (0.0,), (0.25, 0.5))
    c = _stm(gpu_ctx, orbits, (0,), (0.25,), (0.25,))
    whole, parts = a.Phi[:, :, 1, 0, 0], c.Phi[:, :, 0, 0, 0] @ a.Phi[:, :, 0, 0, 0]
    d = np.abs(whole - parts).max() / np.abs(whole).max()
    print("device: |Phi^T S Phi - S| / max |Phi|^2 <= %.2e, composition %.2e relative" % (worst, d))
    assert worst <= H.GPU_PHI and d <= H.GPU_PHI
    assert np.abs(a.X_tgt[:, 0, 0, 0] - c.X[:, 0, 0]).max() <= H.GPU_X


def test_one_period_from_phase_zero_is_the_table_call(gpu_ctx, orbits):
    s0, per = _inputs(orbits, (0, 1))
    r = lto.halo_stm(s0, per, [0.0], [1.0], MU=MU, integ=_integ(), ctx=gpu_ctx)
    t = lto.halo_table(s0, per, 2, MU=MU, integ=_integ(), ctx=gpu_ctx)
    d = H.rel_block(r.Phi[:, :, 0, 0, :], t.M)
    print("Phi(P, 0) against halo_table(n_samples=2).M: %.2e relative, bit-equal: %s; X_tgt against its last sample: %.2e"
          % (d, np.array_equal(r.Phi[:, :, 0, 0, :], t.M), np.abs(r.X_tgt[:, 0, 0, :] - t.X[:, 1, :]).max()))
    assert np.all(r.status == 0) and np.all(t.status == 0) and d <= H.GPU_PHI
    assert np.array_equal(r.X[:, 0, :], s0) and np.all(r.accepted[0] > 0)                  # tau = 0 flies nothing
    for k in (0, 1):
        assert np.abs(r.Phi[:, :, 0, 0, k] - orbits[k][2]).max() / np.abs(orbits[k][2]).max() <= H.GPU_PHI


def test_rk4_against_the_reference_rk4(gpu_ctx, orbits):
    ks = ORBITS3[:2]
    ref = TR.stms(orbits, ks, TR.TAUS3, TR.HORIZONS, MU, rk4_steps=H.RK4_STEPS)
    r = _stm(gpu_ctx, orbits, ks, TR.TAUS3, TR.HORIZONS, integ=lto.integrator(lto.RK4, steps=H.RK4_STEPS))
    dx, dxt, dphi = np.abs(r.X - ref.X).max(), np.abs(r.X_tgt - ref.X_tgt).max(), H.rel_block(r.Phi, ref.Phi)
    print("RK4 x %d per span: X %.2e, X_tgt %.2e, Phi %.2e (relative)" % (H.RK4_STEPS, dx, dxt, dphi))
    assert np.all(r.status == 0) and np.all(r.accepted == 3 * H.RK4_STEPS) and np.all(r.rejected == 0)
    assert dx <= H.GPU_RK4_X and dxt <= H.GPU_RK4_X_TGT and dphi <= H.GPU_RK4_PHI
    r0 = _stm(gpu_ctx, orbits, (0,), (0.0,), (1.0,), integ=lto.integrator(lto.RK4, steps=7))
    assert r0.accepted[0, 0] == 7 and np.array_equal(r0.X[:, 0, 0], orbits[0][0])          # a coast of 0 takes no steps


def test_a_record_does_not_depend_on_its_batch(gpu_ctx, orbits, nine):
    for g in (0, 7, 8):
        b, j = divmod(g, 3)
        s = _stm(gpu_ctx, orbits, (ORBITS3[b],), (TR.TAUS3[j],), TR.HORIZONS)
        for f in STM_FIELDS:
            assert np.array_equal(np.asarray(getattr(nine, f))[..., j, b], np.asarray(getattr(s, f))[..., 0, 0]), (g, f)
    # the optional outputs left out: the others do not move
    s0, per = _inputs(orbits, ORBITS3)
    s0 = np.asfortranarray(s0)
    tau, hz = np.array(TR.TAUS3), np.array(TR.HORIZONS)
    X, Phi, status = np.zeros((6, 3, 3), order="F"), np.zeros((6, 6, 2, 3, 3), order="F"), np.zeros((3, 3), dtype=np.int32, order="F")
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                    # noqa: E731
    integ = _integ()
    rc = gpu_ctx.fn("halo_stm_batch")(gpu_ctx.handle, 3, 2, 3, MU, p(s0), p(per), p(tau), p(hz), C.byref(integ), p(X), p(Phi), None, None,
                                      None, p(status))
    assert rc == 0 and np.array_equal(X, nine.X) and np.array_equal(Phi, nine.Phi) and np.array_equal(status, nine.status)


def test_a_bad_orbit_fails_alone(gpu_ctx, orbits, nine):
    s0, per = _inputs(orbits, ORBITS3)
    s0[2, 1] = np.nan
    r = lto.halo_stm(s0, per, TR.TAUS3, TR.HORIZONS, MU=MU, integ=_integ(), ctx=gpu_ctx)
    assert np.array_equal(r.status, [[0, 2, 0]] * 3)
    assert np.all(np.isnan(r.X[:, :, 1])) and np.all(np.isnan(r.Phi[..., 1])) and np.all(np.isnan(r.X_tgt[..., 1]))
    for b in (0, 2):
        for f in STM_FIELDS:
            assert np.array_equal(np.asarray(getattr(r, f))[..., b], np.asarray(getattr(nine, f))[..., b]), (b, f)
    # a period that is not positive, one that is not finite
    s0, per = _inputs(orbits, ORBITS3)
    per[0], per[2] = -per[0], np.inf
    r2 = lto.halo_stm(s0, per, TR.TAUS3, TR.HORIZONS, MU=MU, integ=_integ(), ctx=gpu_ctx)
    assert np.array_equal(r2.status, [[2, 0, 2]] * 3) and np.all(np.isnan(r2.Phi[..., 0])) and np.all(np.isnan(r2.X[..., 2]))
    assert np.array_equal(r2.Phi[..., 1], nine.Phi[..., 1])
    # spans that run out of steps: NaN everywhere, status 2
    r3 = _stm(gpu_ctx, orbits, ORBITS3, TR.TAUS3, TR.HORIZONS, integ=_integ(max_steps=3))
    assert np.all(r3.status == 2) and np.all(np.isnan(r3.X)) and np.all(np.isnan(r3.Phi)) and np.all(np.isnan(r3.X_tgt))


def test_stm_argument_errors_return_their_codes(gpu_ctx, orbits):
    EINVAL, ENULL, EUNSUPPORTED = _lib.LTO_EINVAL, _lib.LTO_ENULL, _lib.LTO_EUNSUPPORTED
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)            # noqa: E731
    s0, per = _inputs(orbits, ORBITS3[:2])
    a = dict(state0=np.asfortranarray(s0), period=per, tau=np.array([0.1, 0.8]), horizon=np.array([0.5, 1.0]))
    outs = dict(X=np.full((6, 2, 2), 7.0), Phi=np.full((6, 6, 2, 2, 2), 7.0), status=np.full((2, 2), 7, dtype=np.int32))

    def call(n_phase=2, n_tgt=2, n_batch=2, mu=MU, integ=_integ(), **over):
        b = dict(a, **outs)
        b.update(over)
        return gpu_ctx.fn("halo_stm_batch")(gpu_ctx.handle, n_phase, n_tgt, n_batch, mu, p(b["state0"]), p(b["period"]), p(b["tau"]),
                                            p(b["horizon"]), None if integ is None else C.byref(integ), p(b["X"]), p(b["Phi"]), None, None,
                                            None, p(b["status"]))
    hz = lambda *v: np.array(v, dtype=float)                                      # noqa: E731
    for kw in (dict(n_phase=0), dict(n_tgt=0), dict(n_batch=0), dict(mu=0.0), dict(mu=1.0), dict(mu=float("nan")),
               dict(horizon=hz(0.0, 1.0)), dict(horizon=hz(-0.5, 1.0)), dict(horizon=hz(0.5, 0.5)), dict(horizon=hz(1.0, 0.5)),
               dict(horizon=hz(0.5, np.inf)), dict(horizon=hz(np.nan, 1.0)), dict(tau=np.array([0.1, np.nan])),
               dict(tau=np.array([np.inf, 0.2])), dict(integ=lto.integrator(lto.RK4, steps=0)),
               dict(n_phase=1 << 12, n_tgt=1 << 4, n_batch=1 << 10)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(integ=lto.integrator(lto.RKF78_ADAPTIVE)), dict(integ=lto.integrator(lto.RKF78_FIXED, steps=10))):
        assert call(**kw) == EUNSUPPORTED, kw
    for kw in (dict(state0=None), dict(period=None), dict(tau=None), dict(horizon=None), dict(integ=None), dict(X=None), dict(Phi=None),
               dict(status=None)):
        assert call(**kw) == ENULL, kw
    assert all(np.all(v == 7) for v in outs.values())
    assert call() == 0 and np.all(outs["status"] == 0) and np.all(np.isfinite(outs["Phi"]))


# -------------------------------------------------------------------------------------------------------------- 2. the gains call
def _records(nine, n):
    """n records of 2 targets from the device's own Phi: the 9 of the shared call, repeated with a scale that keeps them distinct."""
    flat = nine.Phi.reshape(6, 6, 2, 9, order="F")
    return np.asfortranarray(np.stack([flat[:, :, :, g % 9] * (1.0 + 0.03125 * (g // 9)) for g in range(n)], axis=3))


@pytest.mark.parametrize("n,K,q,r", [(1, 1, TR.Q, (1.0,)), (1, 2, TR.Q, (1.0, 1.0)), (9, 1, 1e-4, (2.0,)), (9, 2, TR.Q, (1.0, 1.0)),
                                     (65, 2, TR.Q, (0.5, 2.0)), (65, 1, 0.0, (1.0,))])
def test_gains_equal_the_reference_loops_bit_for_bit(gpu_ctx, nine, n, K, q, r):
    Phi = np.asfortranarray(_records(nine, n)[:, :, :K, :])
    G, pivot, status = TR.gains(Phi, q, r)
    g = lto.stationkeep_target_gains(Phi, q=q, r=r, ctx=gpu_ctx)
    print("%d records x %d targets, q %.0e: pivot %.1e .. %.1e, |G| <= %.3g" % (n, K, q, pivot.min(), pivot.max(), np.abs(G).max()))
    assert np.all(status == 0) and g.G.shape == (3, 6, n)
    assert np.array_equal(g.G, G) and np.array_equal(g.pivot, pivot) and np.array_equal(g.status, status)


def test_gains_keep_the_shape_of_the_stm_call(gpu_ctx, nine):
    g = lto.stationkeep_target_gains(nine.Phi, ctx=gpu_ctx)
    G, pivot, status = TR.gains(nine.Phi, TR.Q, (1.0, 1.0))
    assert g.G.shape == (3, 6, 3, 3) and g.pivot.shape == (3, 3) and g.status.shape == (3, 3)
    assert np.array_equal(g.G, G) and np.array_equal(g.pivot, pivot) and np.all(g.status == 0)
    one = lto.stationkeep_target_gains(nine.Phi[:, :, :, 1, 2], ctx=gpu_ctx)
    assert one.status == 0 and np.array_equal(one.G, G[:, :, 1, 2]) and one.pivot == pivot[1, 2]


def test_gains_flag_only_the_bad_records(gpu_ctx, nine):
    Phi = _records(nine, 65).copy()
    Phi[4, 2, 1, 3] = np.nan                                 # a NaN outside the rows the law reads: still an input that is not finite
    Phi[0, 4, 0, 64] = np.inf
    Phi[:3, 3:, :, 7] = 0.0                                  # B = 0 in every block of record 7
    ref = TR.gains(Phi, 0.0, (1.0, 1.0))
    g = lto.stationkeep_target_gains(Phi, q=0.0, r=(1.0, 1.0), ctx=gpu_ctx)
    want = np.zeros(65, dtype=np.int32)
    want[3], want[64], want[7] = 2, 2, 3
    assert np.array_equal(g.status, want) and np.array_equal(ref[2], want)
    assert np.array_equal(g.G, ref[0], equal_nan=True) and np.array_equal(g.pivot, ref[1], equal_nan=True)
    bad = want != 0
    assert np.all(np.isnan(g.G[:, :, bad])) and np.all(np.isnan(g.pivot[bad])) and np.all(np.isfinite(g.G[:, :, ~bad]))
    clean = lto.stationkeep_target_gains(_records(nine, 65), q=0.0, r=(1.0, 1.0), ctx=gpu_ctx)
    assert np.array_equal(g.G[:, :, ~bad], clean.G[:, :, ~bad])                  # the neighbours are untouched
    # with q > 0 the record without B is regular, and its law is no burn; sing_tol above every pivot: status 3 everywhere else
    g1 = lto.stationkeep_target_gains(Phi, q=1.0, r=(1.0, 1.0), ctx=gpu_ctx)
    assert g1.status[7] == 0 and np.all(g1.G[:, :, 7] == 0.0) and g1.pivot[7] == 1.0
    g2 = lto.stationkeep_target_gains(Phi, q=0.0, r=(1.0, 1.0), sing_tol=0.9, ctx=gpu_ctx)
    assert np.array_equal(g2.status, np.where(want == 2, 2, 3))


def test_gains_argument_errors_return_their_codes(gpu_ctx, nine):
    EINVAL, ENULL = _lib.LTO_EINVAL, _lib.LTO_ENULL
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)            # noqa: E731
    Phi = _records(nine, 9)
    G, pivot, status = np.full((3, 6, 9), 7.0), np.full(9, 7.0), np.full(9, 7, dtype=np.int32)
    w = lambda *v: np.array(v, dtype=float)                                       # noqa: E731

    def call(n_tgt=2, n_rec=9, Phi=Phi, q=TR.Q, r=w(1.0, 1.0), tol=1e-12, G=G, status=status):
        return gpu_ctx.fn("stationkeep_target_gains_batch")(gpu_ctx.handle, n_tgt, n_rec, p(Phi), q, p(r), tol, p(G), p(pivot), p(status))
    for kw in (dict(n_tgt=0), dict(n_rec=0), dict(q=-1e-9), dict(q=float("inf")), dict(q=float("nan")), dict(r=w(1.0, -1.0)),
               dict(r=w(np.nan, 1.0)), dict(r=w(1.0, np.inf)), dict(r=w(0.0, 0.0)), dict(tol=-1e-9), dict(tol=1.0), dict(tol=float("nan")),
               dict(n_tgt=2, n_rec=1 << 25)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(Phi=None), dict(r=None), dict(G=None), dict(status=None)):
        assert call(**kw) == ENULL, kw
    assert np.all(G == 7.0) and np.all(pivot == 7.0) and np.all(status == 7)
    assert call() == 0 and np.all(status == 0) and np.all(np.isfinite(G))


# ------------------------------------------------------------------------------------------------------------------- 3. the drivers
def test_driver_gains_against_the_reference(gpu_ctx, orbits):
    g = drivers.target_point_gains(orbits[0], taus=TR.TAUS3, MU=MU, integ=_integ(), ctx=gpu_ctx)
    L = TR.law(orbits, 0, TR.TAUS3, MU)
    dg = np.abs(g.G - L.G).max() / np.abs(L.G).max()
    print("target-point law of orbit 1 at %s: X_ref %.2e, G %.2e (relative), |G| <= %.3g" % (g.tau, np.abs(g.X_ref - L.X_ref).max(), dg,
                                                                                         np.abs(L.G).max()))
    assert np.array_equal(g.tau, TR.TAUS3) and np.array_equal(g.dt, L.dt) and g.W is None and g.alpha is None and g.lam is None
    assert np.abs(g.X_ref - L.X_ref).max() <= H.GPU_X and dg <= H.GPU_G
    # the law asks for no hyperbolic pair: an orbit whose M the Floquet-mode driver refuses
    no_pair = (orbits[0][0], orbits[0][1], np.eye(6))
    with pytest.raises(ValueError):
        drivers.stationkeeping_gains(no_pair, taus=TR.TAUS3, MU=MU, integ=_integ(), ctx=gpu_ctx)
    g2 = drivers.target_point_gains(no_pair, taus=TR.TAUS3, MU=MU, integ=_integ(), ctx=gpu_ctx)
    assert np.array_equal(g2.G, g.G)
    with pytest.raises(ValueError):
        drivers.target_point_gains(orbits[0], taus=TR.TAUS3, MU=MU, integ=_integ(max_steps=3), ctx=gpu_ctx)


@pytest.mark.parametrize("per_run", [False, True])
def test_flight_under_the_law_against_the_reference(gpu_ctx, orbits, per_run):
    """3 runs x 3 uneven phases x 2 revolutions, nav and exe given, under the law drivers.target_point_gains returns (per_run: one
    law per run, about orbits 1 and 2 alternating).  The reference flies the same X_ref, dt and G, so the bounds are those of the
    flights' own spread; how far the device's law is from the reference's is test_driver_gains_against_the_reference's business."""
    n_orb = 3 if per_run else 1
    gs = [drivers.target_point_gains(orbits[(b % 2) if per_run else 0], taus=TR.TAUS3, MU=MU, integ=_integ(), ctx=gpu_ctx)
          for b in range(n_orb)]
    for b, g in enumerate(gs):
        L = TR.law(orbits, (b % 2) if per_run else 0, TR.TAUS3, MU)
        assert np.array_equal(g.tau, TR.TAUS3) and np.array_equal(g.dt, L.dt)
        assert np.abs(g.X_ref - L.X_ref).max() <= H.GPU_X and np.abs(g.G - L.G).max() <= H.GPU_G * np.abs(L.G).max()
    e, nav, exe = SR.draws(3, 6, 11)
    x0 = np.stack([gs[b if per_run else 0].X_ref[:, 0] for b in range(3)], axis=1) + e
    c = SR.Case(np.stack([g.X_ref for g in gs], axis=2), np.stack([g.dt for g in gs], axis=1), np.stack([g.G for g in gs], axis=3), x0,
                nav, exe, 2, n_orb)
    ref = SR.fly(("target", "driver law %d" % per_run), c, MU)
    sq = c.n_orb == 1
    r = lto.stationkeep_flight(c.X_ref[:, :, 0] if sq else c.X_ref, c.dt[:, 0] if sq else c.dt, c.G[:, :, :, 0] if sq else c.G, c.x0,
                               c.n_rev, nav=c.nav, exe=c.exe, MU=MU, integ=_integ(), ctx=gpu_ctx)
    d = dict(x=np.abs(r.x_final - ref.x_final).max(), dev_r=np.nanmax(np.abs(r.dev[0] - ref.dev[0])),
             dev_v=np.nanmax(np.abs(r.dev[1] - ref.dev[1])), hist=np.nanmax(np.abs(r.dv_hist - ref.dv_hist)),
             total=np.abs(r.dv_total - ref.dv_total).max(), dev_final=np.abs(r.dev_final - ref.dev_final).max())
    print("target-point flights, per-run %d: " % per_run + " ".join("%s %.2e" % kv for kv in d.items()))
    assert np.array_equal(r.status, ref.status) and np.array_equal(r.n_burn, ref.n_burn) and np.all(r.status == 0) and np.all(r.n_burn == 6)
    for k, v in d.items():
        assert v <= H.GPU_TARGET[k], (k, v, H.GPU_TARGET[k])


def test_driver_monte_carlo_keeps_every_run(gpu_ctx, orbits):
    """The vetted Monte Carlo (tests/golden/stationkeep_target_mc.json): 16 runs, 20 revolutions, four burns each."""
    gold = H.monte_carlo_golden()
    kw = dict(H.MONTE_CARLO, MU=MU, integ=_integ(), ctx=gpu_ctx)
    L = TR.law(orbits, 0, TR.TAUS4, MU)
    g = drivers.target_point_gains(orbits[0], MU=MU, integ=_integ(), ctx=gpu_ctx)
    dg = np.abs(g.G - L.G).max() / np.abs(L.G).max()
    out = drivers.stationkeep(orbits[0], gains=g, **kw)
    print("device law against the reference's %.2e; target-point: lost %.0f %%, dv per year %.2f (median) %.2f (max) m/s, largest "
          "deviation %.2f km" % (dg, 100.0 * out["lost_share"], np.median(out["dv_per_year_ms"]), out["dv_per_year_ms"].max(),
                                 np.nanmax(out["dev_r_km"])))
    assert dg <= H.GPU_G and np.array_equal(g.tau, TR.TAUS4)
    assert np.all(out["status"] == 0) and out["lost_share"] == 0.0 and np.all(out["n_burn"] == 80)
    assert np.nanmax(out["dev_r_km"]) * H.MC_MARGIN <= H.MONTE_CARLO["r_lost_km"]
    # dv per run under the device's own law against the reference's flights under the reference's law: the laws differ within
    # GPU_X and GPU_G, which H.GPU_TARGET_MC_LAW accounts for
    d_law = np.abs(out["dv_ms"] / H.MS - np.array(gold["law"]["dv_total"])).max()
    print("dv per run, the device's law against the reference's law and flights: %.2e" % d_law)
    assert d_law <= H.GPU_TARGET_MC_LAW
    # the same draws under the reference's law: dv per run against the reference's flight
    ref = drivers.stationkeep(orbits[0], gains=g._replace(X_ref=L.X_ref, G=L.G), **kw)
    d = dict(total=np.abs(ref["dv_ms"] / H.MS - np.array(gold["law"]["dv_total"])).max(),
             x=np.abs(ref["x_final"].T - np.array(gold["law"]["x_final"])).max(),
             dev_final=np.abs(np.stack([ref["dev_final_r_km"] / H.KM, ref["dev_final_v_ms"] / H.MS], axis=1)
                              - np.array(gold["law"]["dev_final"])).max())
    print("reference law on the device against the reference's flights over 20 revolutions: " + " ".join("%s %.2e" % kv for kv in d.items()))
    assert np.all(ref["status"] == 0)
    for k, v in d.items():
        assert v <= H.GPU_TARGET_MC[k], (k, v)
    # without a law every run is lost
    free = drivers.stationkeep(orbits[0], gains=g._replace(G=np.zeros_like(g.G)), **kw)
    print("uncontrolled: lost at %s" % free["lost_at"])
    assert np.array_equal(free["x0"], out["x0"]) and np.all(free["status"] == 1) and free["lost_share"] == 1.0
