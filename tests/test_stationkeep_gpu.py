"""GPU checks of the station-keeping calls (lto_stationkeep_gains_batch, lto_stationkeep_flight_batch and the drivers above them,
DESIGN 4.29) against the independent host reference (tests/stationkeep_reference.py: plain loops in the header's order for the
gains, scipy DOP853 at rtol 1e-13 / atol 1e-14 with one solve per span for the flights).  Every bound is a named constant of
tests/test_stationkeep_host.py, which holds the reference's own spread to a tenth of it; the gains are compared bit for bit.  The
shapes are the smallest that can still go wrong: 1, 3 and 65 runs (65 crosses the 64-lane block), one burn per revolution and three
at the uneven phases 0.1, 0.35, 0.8 (the first burn off phase 0, the wrap-round span flown), one and two revolutions.

Figures measured on an MI355X are in DESIGN 4.29."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import manifold_reference as MR  # noqa: E402
import stationkeep_reference as SR  # noqa: E402
import test_stationkeep_host as H  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import _lib, drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("x_final", "dv_total", "n_burn", "dev", "dv_hist", "dev_final", "accepted", "rejected", "status", "lost_at")


@pytest.fixture(scope="module")
def orbits():
    return MR.packaged_orbits(synth.halo_orbits(), MU)


def _integ():
    return lto.integrator(rtol=SR.RTOL, atol=SR.ATOL)


def _fly(ctx, c, integ=None, **kw):
    sq = c.n_orb == 1
    return lto.stationkeep_flight(c.X_ref[:, :, 0] if sq else c.X_ref, c.dt[:, 0] if sq else c.dt, c.G[:, :, :, 0] if sq else c.G, c.x0,
                                  c.n_rev, nav=c.nav, exe=c.exe, MU=MU, integ=integ or _integ(), ctx=ctx, **kw)


def _one(c, b):
    """Run b of the case c as a case of its own."""
    o = slice(b, b + 1) if c.n_orb > 1 else slice(0, 1)
    return SR.Case(c.X_ref[:, :, o], c.dt[:, o], c.G[:, :, :, o], c.x0[:, b:b + 1], None if c.nav is None else c.nav[:, :, b:b + 1],
                   None if c.exe is None else c.exe[:, :, b:b + 1], c.n_rev, 1)


def _same_run(r, b, s):
    """Run b of the flight r equals the single-run flight s bit for bit, NaN in the same places."""
    return all(np.array_equal(np.asarray(getattr(r, f))[..., b], np.asarray(getattr(s, f))[..., 0], equal_nan=True) for f in FIELDS)


def _compare(tag, r, ref, bounds):
    d = dict(x=np.abs(r.x_final - ref.x_final).max(), dev_r=np.nanmax(np.abs(r.dev[0] - ref.dev[0])),
             dev_v=np.nanmax(np.abs(r.dev[1] - ref.dev[1])), hist=np.nanmax(np.abs(r.dv_hist - ref.dv_hist)),
             total=np.abs(r.dv_total - ref.dv_total).max(), dev_final=np.abs(r.dev_final - ref.dev_final).max())
    print("%-34s " % tag + " ".join("%s %.2e" % kv for kv in d.items()) + "  steps %d..%d, rejected <= %d"
          % (r.accepted.min(), r.accepted.max(), r.rejected.max()))
    assert np.array_equal(r.status, ref.status) and np.array_equal(r.n_burn, ref.n_burn) and np.array_equal(r.lost_at, ref.lost_at)
    assert np.array_equal(np.isnan(r.dev), np.isnan(ref.dev)) and np.array_equal(np.isnan(r.dv_hist), np.isnan(ref.dv_hist))
    assert np.array_equal(r.dv_hist == 0.0, ref.dv_hist == 0.0)
    for k, v in d.items():
        assert v <= bounds[k], (tag, k, v, bounds[k])


# ------------------------------------------------------------------------------------------------------------------------ 1. gains
@pytest.mark.parametrize("P,B", [(1, 1), (5, 1), (1, 2), (5, 2)])
def test_gains_equal_the_reference_loops_bit_for_bit(gpu_ctx, orbits, P, B):
    V = np.stack([MR.shared_seeds(orbits, k, 8, MU)[2][:, :, :P] for k in range(B)], axis=3)
    W, G, alpha, status = SR.gains(V, 1e-8)
    r = lto.stationkeep_gains(V if B > 1 else V[..., 0], ctx=gpu_ctx)
    got = [np.asarray(a).reshape(ref.shape) for a, ref in zip((r.W, r.G, r.alpha, r.status), (W, G, alpha, status))]
    print("%d phases x %d orbits: alpha %.3f .. %.3f, |G| <= %.3g" % (P, B, alpha.min(), alpha.max(), np.abs(G).max()))
    assert np.all(status == 0)
    assert np.array_equal(got[0], W) and np.array_equal(got[1], G) and np.array_equal(got[2], alpha) and np.array_equal(got[3], status)
    for b in range(B):                                       # W . v_u = 1, and the law removes the unstable component
        for j in range(P):
            assert abs(got[0][:, j, b] @ V[:, 0, j, b] - 1.0) < 1e-14


def test_gains_flag_only_the_bad_records(gpu_ctx, orbits):
    V = np.stack([MR.shared_seeds(orbits, k, 8, MU)[2][:, :, :5] for k in range(2)], axis=3).copy()
    V[2, 1, 3, 0] = np.nan                                   # a NaN in the stable vector of (phase 3, orbit 0)
    V[:3, 1, 1, 1] = 0.0                                     # v_s without a position part at (phase 1, orbit 1): w_v = 0, alpha = 0
    V[3, 0, 4, 1] = np.inf
    ref = SR.gains(V, 1e-8)
    r = lto.stationkeep_gains(V, ctx=gpu_ctx)
    want = np.zeros((5, 2), dtype=np.int32)
    want[3, 0], want[1, 1], want[4, 1] = 2, 3, 2
    assert np.array_equal(r.status, want) and np.array_equal(ref[3], want)
    for got, exp in zip((r.W, r.G, r.alpha), ref[:3]):
        assert np.array_equal(got, exp, equal_nan=True)
    bad = want != 0
    assert np.all(np.isnan(r.W[:, bad])) and np.all(np.isnan(r.G[:, :, bad])) and np.all(np.isnan(r.alpha[bad]))
    assert np.all(np.isfinite(r.W[:, ~bad])) and np.all(np.isfinite(r.G[:, :, ~bad]))
    # sing_tol above alpha: status 3 for every record, whatever else it holds
    r1 = lto.stationkeep_gains(V[..., 0], sing_tol=0.9, ctx=gpu_ctx)
    assert np.array_equal(r1.status, [3, 3, 3, 2, 3])


# --------------------------------------------------------------------------------------------------- 2. flights against the reference
@pytest.mark.parametrize("B,n_man,n_rev,errors,per_run", [
    (1, 1, 1, False, False), (3, 3, 2, True, False), (65, 3, 2, True, False), (3, 1, 2, True, True), (3, 3, 1, False, True),
    (65, 3, 2, True, True)])
def test_flight_under_the_law_against_the_reference(gpu_ctx, orbits, B, n_man, n_rev, errors, per_run):
    c = SR.case(orbits, MU, B, n_man, n_rev, errors, per_run)
    ref = SR.fly(("gpu law", B, n_man, n_rev, errors, per_run), c, MU)
    r = _fly(gpu_ctx, c)
    _compare("law B %d n_man %d n_rev %d err %d per-run %d" % (B, n_man, n_rev, errors, per_run), r, ref, H.GPU_LAW)
    assert np.all(r.status == 0) and np.all(r.n_burn == n_man * n_rev) and np.all(r.lost_at == -1)


@pytest.mark.parametrize("per_run", [False, True])
def test_rk4_flight_against_the_reference_rk4(gpu_ctx, orbits, per_run):
    c = SR.case(orbits, MU, 3, 3, 2, True, per_run)
    ref = SR.fly(("rk4 %d" % per_run, "other"), c, MU, rk4_steps=H.RK4_STEPS)
    r = _fly(gpu_ctx, c, integ=lto.integrator(lto.RK4, steps=H.RK4_STEPS))
    _compare("rk4 x %d per-run %d" % (H.RK4_STEPS, per_run), r, ref, H.GPU_RK4)
    assert np.all(r.accepted == 6 * H.RK4_STEPS) and np.all(r.rejected == 0)


def test_a_law_that_is_not_ours(gpu_ctx, orbits):
    """A random finite G: the flight knows nothing of Floquet modes."""
    c = SR.case(orbits, MU, 8, 3, 2, True, True, random_gain=H.RANDOM_GAIN)
    ref = SR.fly(("random law", "tight"), c, MU)
    r = _fly(gpu_ctx, c)
    _compare("random law", r, ref, H.GPU_FREE)
    assert np.all(r.status == 0)


# -------------------------------------------------------------------------------------------------------------------- 3. thresholds
def test_dead_band_and_clip_on_the_vetted_inputs(gpu_ctx, orbits):
    c = H.threshold_case(orbits)
    ref = SR.fly(("thresholds", "tight"), c, MU, dv_min=H.DV_MIN, dv_max=H.DV_MAX)
    r = _fly(gpu_ctx, c, dv_min=H.DV_MIN, dv_max=H.DV_MAX)
    _compare("dead band and clip", r, ref, H.GPU_FREE)
    print("burns %s of 3, applied |dv|:\n%s" % (r.n_burn, r.dv_hist.T))
    assert r.n_burn[0] == 0 and np.all(r.dv_hist[:, 0] == 0.0) and r.dv_total[0] == 0.0          # every burn of the small run skipped
    assert np.all(r.n_burn[1:] == 3)
    # the large run is clipped: the commanded part has the size dv_max, the execution error comes on top of it
    assert np.all(np.abs(r.dv_hist[:, 2] - H.DV_MAX) < 0.2 * H.DV_MAX) and np.all(ref.cmd[:, 2] > 2.0 * H.DV_MAX)
    free = _fly(gpu_ctx, c)
    assert np.all(free.n_burn == 3) and np.all(free.dv_hist[:, 2] > 2.0 * H.DV_MAX)


def test_uncontrolled_runs_are_lost_where_the_reference_loses_them(gpu_ctx, orbits):
    c = H.lost_case(orbits)
    ref = SR.fly(("lost", "tight"), c, MU, r_lost=H.R_LOST)
    r = _fly(gpu_ctx, c, r_lost=H.R_LOST)
    _compare("G = 0, r_lost %.1e" % H.R_LOST, r, ref, H.GPU_FREE)
    print("lost at %s" % r.lost_at)
    assert np.all(r.status == 1) and np.array_equal(r.lost_at, ref.lost_at)
    for b, u in enumerate(r.lost_at):
        assert np.all(np.isfinite(r.dev[:, :u + 1, b])) and np.all(np.isnan(r.dev[:, u + 1:, b]))
        assert np.all(r.dv_hist[:u, b] == 0.0) and np.all(np.isnan(r.dv_hist[u:, b]))
        assert r.dev[0, u, b] > H.R_LOST and np.array_equal(r.dev_final[:, b], r.dev[:, u, b])
        assert r.n_burn[b] == u and r.dv_total[b] == 0.0 and np.all(np.isfinite(r.x_final[:, b]))


# ------------------------------------------------------------------------------------------------------ 4. isolation and invariance
def test_a_bad_start_fails_alone(gpu_ctx, orbits):
    c = SR.case(orbits, MU, 3, 3, 2, True, False)
    x0 = c.x0.copy()
    x0[4, 1] = np.nan
    c = c._replace(x0=x0)
    r = _fly(gpu_ctx, c)
    assert list(r.status) == [0, 2, 0]
    assert np.all(np.isnan(r.x_final[:, 1])) and np.isnan(r.dv_total[1]) and np.all(np.isnan(r.dev_final[:, 1]))
    assert np.all(np.isnan(r.dev[:, :, 1])) and np.all(np.isnan(r.dv_hist[:, 1])) and r.n_burn[1] == 0 and r.lost_at[1] == -1
    for b in (0, 2):
        assert _same_run(r, b, _fly(gpu_ctx, _one(c, b)))
    # a NaN in one run's navigation error at its fourth update: that run fails there and keeps its history up to it
    nav = c.nav.copy()
    nav[2, 3, 2] = np.nan
    r2 = _fly(gpu_ctx, c._replace(x0=SR.case(orbits, MU, 3, 3, 2, True, False).x0, nav=nav))
    assert list(r2.status) == [0, 0, 2] and r2.n_burn[2] == 3
    assert np.all(np.isfinite(r2.dev[:, :3, 2])) and np.all(np.isnan(r2.dev[:, 3:, 2])) and np.all(np.isnan(r2.dv_hist[3:, 2]))
    # a span that runs out of steps
    r3 = _fly(gpu_ctx, c, integ=lto.integrator(rtol=SR.RTOL, atol=SR.ATOL, max_steps=5))
    assert np.all(r3.status == 2) and np.all(np.isnan(r3.x_final))


@pytest.mark.parametrize("per_run", [False, True])
def test_a_run_does_not_depend_on_its_batch(gpu_ctx, orbits, per_run):
    c = SR.case(orbits, MU, 65, 3, 2, True, per_run)
    r = _fly(gpu_ctx, c)
    for b in (0, 1, 63, 64):
        assert _same_run(r, b, _fly(gpu_ctx, _one(c, b))), b
    # optional outputs left out: the others do not move
    sq = c.n_orb == 1
    B, n_upd = 65, 6
    x_final, dv_total, status = np.zeros((6, B), order="F"), np.zeros(B), np.zeros(B, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                    # noqa: E731
    arrs = [np.asfortranarray(a) for a in (c.X_ref, c.dt, c.G, c.x0, c.nav, c.exe)]
    integ = _integ()
    rc = gpu_ctx.fn("stationkeep_flight_batch")(gpu_ctx.handle, 3, 2, B, MU, p(arrs[0]), p(arrs[1]), p(arrs[2]), 1 if sq else B, p(arrs[3]),
                                                p(arrs[4]), p(arrs[5]), 0.0, 0.0, 0.0, C.byref(integ), p(x_final), p(dv_total), None, None,
                                                None, None, None, None, p(status), None)
    assert rc == 0 and n_upd == c.nav.shape[1]
    assert np.array_equal(x_final, r.x_final) and np.array_equal(dv_total, r.dv_total) and np.array_equal(status, r.status)


# --------------------------------------------------------------------------------------------------- 5. consistency with existing code
def test_one_span_without_a_law_is_the_section_flight(gpu_ctx, orbits):
    c = SR.case(orbits, MU, 3, 1, 1, False, True)
    c = c._replace(G=np.zeros_like(c.G))
    r = _fly(gpu_ctx, c)
    f = lto.section_flight(c.x0, c.dt[0], n_cross=0, MU=MU, integ=_integ(), ctx=gpu_ctx)
    d = np.abs(r.x_final - f.x_end).max()
    print("one span, G = 0, against lto_section_flight_batch: %.2e" % d)
    assert np.all(f.status == 0) and np.all(r.status == 0) and d <= H.GPU_LAW["x"]
    d0 = c.x0 - c.X_ref[:, 0]
    assert np.all(r.dv_total == 0.0) and np.all(r.n_burn == 1)                   # no dead band: a zero command is a burn of size zero
    assert np.allclose(r.dev[:, 0], [np.linalg.norm(d0[:3], axis=0), np.linalg.norm(d0[3:], axis=0)], rtol=1e-14, atol=0.0)


# ------------------------------------------------------------------------------------------------------------------------ 6. drivers
def test_driver_gains_against_the_reference(gpu_ctx, orbits):
    g = drivers.stationkeeping_gains(orbits[0], taus=SR.TAUS3, MU=MU, integ=_integ(), ctx=gpu_ctx)
    L = SR.law(orbits, 0, SR.TAUS3, MU)
    print("gains of orbit 1 at %s: X_ref %.2e, W %.2e, G %.2e (relative), alpha %s" % (
        g.tau, np.abs(g.X_ref - L.X_ref).max(), np.abs(g.W - L.W).max() / np.abs(L.W).max(), np.abs(g.G - L.G).max() / np.abs(L.G).max(), g.alpha))
    assert np.array_equal(g.tau, SR.TAUS3) and np.array_equal(g.dt, L.dt)
    import test_manifold_host as HM
    assert np.abs(g.X_ref - L.X_ref).max() <= HM.GPU_SEED_X
    # W and G are built from the device's unit vectors, each within GPU_SEED_V of the reference's: first order in that
    assert np.abs(g.W - L.W).max() <= 20.0 * HM.GPU_SEED_V * np.abs(L.W).max() ** 2
    assert np.abs(g.G - L.G).max() <= 20.0 * HM.GPU_SEED_V * np.abs(L.G).max() * np.abs(L.W).max()
    with pytest.raises(ValueError):
        drivers.stationkeeping_gains((orbits[0][0], orbits[0][1], np.eye(6)), MU=MU, ctx=gpu_ctx)          # no hyperbolic pair


def test_driver_monte_carlo(gpu_ctx, orbits):
    kw = dict(H.MONTE_CARLO, MU=MU, integ=_integ(), ctx=gpu_ctx)
    out = drivers.stationkeep(orbits[0], **kw)
    p = out["percentiles"]
    print("controlled: dv per year %.2f / %.2f / %.2f m/s (50 / 95 / 99 %%), largest deviation %.0f km, lost %.0f %%"
          % (p["dv_per_year_ms"][50], p["dv_per_year_ms"][95], p["dv_per_year_ms"][99], np.nanmax(out["dev_r_km"]), 100.0 * out["lost_share"]))
    assert np.all(out["status"] == 0) and out["lost_share"] == 0.0 and np.all(out["n_burn"] == 12)
    assert np.allclose(out["t_days"], 3.0 * orbits[0][1] * TU / 86400.0, rtol=1e-14)
    for k in ("dv_ms", "dv_per_year_ms"):
        for q in (50, 95, 99):
            assert p[k][q] == float(np.percentile(out[k], q))
    assert np.allclose(out["dv_per_year_ms"], out["dv_ms"] / out["t_days"] * 365.25, rtol=1e-14)
    g = out["gains"]
    # the same draws without a law (test_stationkeep_host.py vets that the reference loses the runs nearest to the stable directions)
    free = drivers.stationkeep(orbits[0], gains=g._replace(G=np.zeros_like(g.G)), **kw)
    print("uncontrolled: lost %.0f %%, at updates %d..%d" % (100.0 * free["lost_share"], free["lost_at"].min(), free["lost_at"].max()))
    assert np.array_equal(free["x0"], out["x0"])
    assert np.all(free["status"] == 1) and free["lost_share"] == 1.0
    assert np.all(free["t_days"] < out["t_days"])


# ---------------------------------------------------------------------------------------------------------------- 7. argument errors
def test_argument_errors_return_their_codes_and_launch_nothing(gpu_ctx, orbits):
    EINVAL, ENULL, EUNSUPPORTED = _lib.LTO_EINVAL, _lib.LTO_ENULL, _lib.LTO_EUNSUPPORTED
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)            # noqa: E731
    V = np.asfortranarray(np.stack([MR.shared_seeds(orbits, k, 8, MU)[2][:, :, :2] for k in range(2)], axis=3))
    W, G, alpha, status = np.full((6, 2, 2), 7.0), np.full((3, 6, 2, 2), 7.0), np.full((2, 2), 7.0), np.full((2, 2), 7, dtype=np.int32)

    def gains(n_phase=2, n_batch=2, V=V, tol=1e-8, G=G, status=status):
        return gpu_ctx.fn("stationkeep_gains_batch")(gpu_ctx.handle, n_phase, n_batch, p(V), tol, p(W), p(G), p(alpha), p(status))
    for kw in (dict(n_phase=0), dict(n_batch=0), dict(tol=-1e-9), dict(tol=1.0), dict(tol=float("nan")), dict(n_phase=1 << 20, n_batch=1 << 8)):
        assert gains(**kw) == EINVAL, kw
    for kw in (dict(V=None), dict(G=None), dict(status=None)):
        assert gains(**kw) == ENULL, kw
    assert np.all(W == 7.0) and np.all(G == 7.0) and np.all(alpha == 7.0) and np.all(status == 7)

    c = SR.case(orbits, MU, 3, 3, 2, True, True)
    a = dict(X_ref=np.asfortranarray(c.X_ref), dt=np.asfortranarray(c.dt), G=np.asfortranarray(c.G), x0=np.asfortranarray(c.x0),
             nav=np.asfortranarray(c.nav), exe=np.asfortranarray(c.exe))
    outs = dict(x_final=np.full((6, 3), 7.0), dv_total=np.full(3, 7.0), status=np.full(3, 7, dtype=np.int32))

    def flight(n_man=3, n_rev=2, n_batch=3, mu=MU, n_orb=3, dv_min=0.0, dv_max=0.0, r_lost=0.0, integ=_integ(), **over):
        b = dict(a, **outs)
        b.update(over)
        return gpu_ctx.fn("stationkeep_flight_batch")(
            gpu_ctx.handle, n_man, n_rev, n_batch, mu, p(b["X_ref"]), p(b["dt"]), p(b["G"]), n_orb, p(b["x0"]), p(b["nav"]), p(b["exe"]),
            dv_min, dv_max, r_lost, None if integ is None else C.byref(integ), p(b["x_final"]), p(b["dv_total"]), None, None, None, None,
            None, None, p(b["status"]), None)
    bad_dt = [a["dt"].copy() for _ in range(3)]
    bad_dt[0][1, 2], bad_dt[1][0, 0], bad_dt[2][2, 1] = 0.0, np.inf, -0.5
    for kw in (dict(n_man=0), dict(n_rev=0), dict(n_batch=0), dict(n_orb=2), dict(n_orb=0), dict(dt=bad_dt[0]), dict(dt=bad_dt[1]),
               dict(dt=bad_dt[2]), dict(dv_min=-1e-9), dict(dv_max=float("inf")), dict(r_lost=float("nan")), dict(mu=0.0), dict(mu=1.0),
               dict(integ=lto.integrator(lto.RK4, steps=0)), dict(n_rev=1 << 27)):
        assert flight(**kw) == EINVAL, kw
    for kw in (dict(integ=lto.integrator(lto.RKF78_ADAPTIVE)), dict(integ=lto.integrator(lto.RKF78_FIXED, steps=10))):
        assert flight(**kw) == EUNSUPPORTED, kw
    for kw in (dict(X_ref=None), dict(dt=None), dict(G=None), dict(x0=None), dict(integ=None), dict(x_final=None), dict(dv_total=None),
               dict(status=None)):
        assert flight(**kw) == ENULL, kw
    assert all(np.all(v == 7) for v in outs.values())
    assert flight() == 0 and np.all(outs["status"] == 0) and np.all(np.isfinite(outs["x_final"]))
