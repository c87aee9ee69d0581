"""Control replay on the device (k_replay_moments, k_control_replay) against tests/replay_reference.py: A lanes and
batches, B control-law classes, knot counts, the mass row, RK4 and sampling, C refusals and poisoned starts, D the demo transfer
flown from its own start and from dispersed ones."""
import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest

import lowthrustopt_amd as lto
import replay_reference as R
from lowthrustopt_amd import drivers
from lowthrustopt_amd.constants import MU, DU, TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check(label, x, dv, ref, bars):
    """One lane against its reference Flight: the final state element by element, dv relative."""
    bx, bdv = bars
    e_x = float(np.max(np.abs(x - ref.x_final)))
    e_dv = abs(dv - ref.dv) / abs(ref.dv) if ref.dv != 0.0 else abs(dv)
    print("MEASURED %s: |x - ref| %.3e (bar %.1e), dv rel %.3e (bar %.1e)" % (label, e_x, bx, e_dv, bdv))
    assert np.all(np.abs(x - ref.x_final) <= bx), label
    assert e_dv <= bdv, label
    return e_x, e_dv


# ------------------------------------------------------------------------------------------------------------- A, lanes
def _lane_templates(own_history):
    """[(start fixture, history fixture)]: every start with its own history, or every start under the history of fixture 0."""
    return [(fx, fx if own_history else R.LANE_FIX[0]) for fx in R.admitted(R.LANE_FIX, None if own_history else R.LANE_FIX[0])]


_SINGLES = {}


def _lane_singles(ctx, own_history):
    """The single call of every template, once per process: [(x_final, dv, accepted, rejected)]."""
    if own_history not in _SINGLES:
        out = []
        for fs, fh in _lane_templates(own_history):
            x0, lamv, prm = R.fix_problem(fs, fh)
            r = lto.control_replay(x0, lamv, 0.0, fh.tof, prm, ctx=ctx)
            assert r.status == 0
            out.append((r.x_final.copy(), r.dv, r.accepted, r.rejected))
        _SINGLES[own_history] = out
    return _SINGLES[own_history]


@pytest.mark.gpu
@pytest.mark.parametrize("own_history", [False, True], ids=["hist1", "histB"])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 129])
def test_lanes(gpu_ctx, B, own_history):
    tm = _lane_templates(own_history)
    assert len(tm) >= 7
    singles = _lane_singles(gpu_ctx, own_history)
    probs = [R.fix_problem(fs, fh) for fs, fh in tm]
    x0, lamv, own = R.place([(p[0], p[1]) for p in probs], B)
    r = lto.control_replay(x0, lamv if own_history else probs[0][1], 0.0, 0.5, probs[0][2], ctx=gpu_ctx)
    assert r.x_final.shape == (6, B) and np.all(r.status == 0)
    worst = 0.0
    for b in range(B):
        fs, fh = tm[own[b]]
        ref = R.fix_flight(fs, hist=None if own_history else fh)
        bx, bdv = R.fix_bars(fs, None if own_history else fh)
        assert np.all(np.abs(r.x_final[:, b] - ref.x_final) <= bx) and abs(r.dv[b] - ref.dv) <= bdv * abs(ref.dv), b
        worst = max(worst, float(np.max(np.abs(r.x_final[:, b] - ref.x_final))))
        sx, sdv, sa, sr = singles[own[b]]
        assert np.array_equal(r.x_final[:, b], sx) and r.dv[b] == sdv and r.accepted[b] == sa and r.rejected[b] == sr, b
    print("MEASURED lanes B=%d %s: largest |x - ref| %.3e" % (B, "own histories" if own_history else "one history", worst))


# ------------------------------------------------------------------------------------------------ B, classes and knots
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(R.CLASS_FIX))
def test_classes_and_knots(gpu_ctx, name):
    fx = R.CLASS_FIX[name]
    if not R.fix_e_ref(fx)[0]:
        pytest.fail("fixture %s is not admitted: the class list of replay_reference.py must change" % name)
    x0, lamv, prm = R.fix_problem(fx)
    X0, _, _ = R.place([(x0, lamv)], 2)
    r = lto.control_replay(X0, lamv, 0.0, fx.tof, prm, ctx=gpu_ctx)
    assert np.all(r.status == 0) and np.all(r.accepted >= fx.n_knots - 1)
    assert np.array_equal(r.x_final[:, 0], r.x_final[:, 1]) and r.dv[0] == r.dv[1]
    _check(name, r.x_final[:, 0], r.dv[0], R.fix_flight(fx), R.fix_bars(fx))


@pytest.mark.gpu
def test_mixed_classes_in_one_batch(gpu_ctx):
    """One call whose lanes carry different control laws (one launch per class): every lane as its own single-class call."""
    names = ("p2_k9_1x", "p15_k9_1", "p0_k9_1")
    fxs = [R.Fix(54, 9, 1.0, 10.0, 2.0, 1.0), R.CLASS_FIX["p15_k9_1"], R.CLASS_FIX["p0_k9_1"]]
    probs = [R.fix_problem(fx) for fx in fxs]
    B = 7
    own = np.arange(B) % 3
    x0 = np.asfortranarray(np.stack([probs[k][0] for k in own], axis=1))
    lamv = np.asfortranarray(np.stack([probs[k][1] for k in own], axis=2))
    r = lto.control_replay(x0, lamv, 0.0, 1.0, [probs[k][2] for k in own], ctx=gpu_ctx)
    assert np.all(r.status == 0)
    for k in range(3):
        s = lto.control_replay(probs[k][0], probs[k][1], 0.0, 1.0, probs[k][2], ctx=gpu_ctx)
        for b in np.nonzero(own == k)[0]:
            assert np.array_equal(r.x_final[:, b], s.x_final) and r.dv[b] == s.dv, (names[k], b)
        _check(names[k], s.x_final, s.dv, R.fix_flight(fxs[k]), R.fix_bars(fxs[k]))


@pytest.mark.gpu
def test_infinite_isp_is_the_constant_mass_system(gpu_ctx):
    """nstate = 7 at Isp = 1e30: the mass stays what it was, bit for bit, and rows 0..5 are the 6-state run at that mass."""
    fx = R.CLASS_FIX["p1_rho01_k9_05"]
    x0, lamv, prm = R.fix_problem(fx)
    prm7 = R.prm_tuple(fx.thrust, fx.p, fx.rho, fx.td, 1e30)
    r7 = lto.control_replay(np.append(x0, R.MASS), lamv, 0.0, fx.tof, prm7, sample_every=1, ctx=gpu_ctx)
    r6 = lto.control_replay(x0, lamv, 0.0, fx.tof, prm, ctx=gpu_ctx)
    assert r7.status == 0 and r6.status == 0
    assert np.all(r7.samples[6] == R.MASS) and r7.x_final[6] == R.MASS
    bx, bdv = R.fix_bars(fx)
    print("MEASURED Isp = 1e30 against the 6-state run: %.3e, dv rel %.3e" % (np.max(np.abs(r7.x_final[:6] - r6.x_final)),
                                                                              abs(r7.dv - r6.dv) / r6.dv))
    assert np.all(np.abs(r7.x_final[:6] - r6.x_final) <= bx) and abs(r7.dv - r6.dv) <= bdv * abs(r6.dv)
    _check("Isp=1e30", r7.x_final[:6], r7.dv, R.fix_flight(fx), (bx, bdv))


@pytest.mark.gpu
def test_zero_history_is_a_ballistic_coast(gpu_ctx, oracle):
    """An all-zero history: no thrust, dv = 0; the end state is the oracle's flow of zero costates, at 1e-11 (the bar of the tail
    test of DESIGN 4.12)."""
    x0 = R.fix_problem(R.CLASS_FIX["p2_k4_1"])[0]
    prm = R.prm_tuple(10.0, 2.0, 1.0)
    y, rc, _, _ = oracle.flow_state_costate(np.append(x0, np.zeros(6)), np.array(prm), 1.0, oracle.DOP853_ADAPTIVE, 0, 1e-13, 1e-13)
    assert rc == 0
    for m in (4, 9):
        r = lto.control_replay(x0, np.zeros((3, m)), 0.0, 1.0, prm, ctx=gpu_ctx)
        e = float(np.max(np.abs(r.x_final - y[:6])))
        print("MEASURED coast, %d knots: %.3e" % (m, e))
        assert r.status == 0 and r.dv == 0.0 and e <= 1e-11


@pytest.mark.gpu
@pytest.mark.parametrize("steps", [1, 2, 16])
def test_rk4(gpu_ctx, steps):
    for name in ("p2_k4_1", "p1_rho01_k9_05", "m_p2_k9_05"):
        fx = R.CLASS_FIX[name]
        ref, e_rk4 = R.fix_rk4(fx, steps)
        x0, lamv, prm = R.fix_problem(fx)
        r = lto.control_replay(x0, lamv, 0.0, fx.tof, prm, integ=lto.integrator(lto.RK4, steps=steps), ctx=gpu_ctx)
        bar = max(1e-14, 10.0 * e_rk4)
        e = np.abs(r.x_final - ref.x_final) / np.maximum(1.0, np.abs(ref.x_final))
        print("MEASURED RK4 x %d %s: %.3e (bar %.1e), dv %.3e" % (steps, name, float(np.max(e)), bar, abs(r.dv - ref.dv)))
        assert r.status == 0 and r.accepted == steps * (fx.n_knots - 1) and r.rejected == 0
        assert np.all(e <= bar) and abs(r.dv - ref.dv) <= bar


@pytest.mark.gpu
def test_samples(gpu_ctx):
    fx = R.CLASS_FIX["m_p2_k9_05"]
    x0, lamv, prm = R.fix_problem(fx)
    X0, _, _ = R.place([(x0, lamv), (R.fix_problem(R.CLASS_FIX["m_back_k9_05"])[0], lamv)], 3)
    ref = R.fix_flight(fx)
    bx, _ = R.fix_bars(fx)
    base = lto.control_replay(X0, lamv, 0.0, fx.tof, prm, ctx=gpu_ctx)
    assert base.samples is None and len(base.sample_knots) == 0
    for every in (1, 3, fx.n_knots - 1, fx.n_knots + 5):
        r = lto.control_replay(X0, lamv, 0.0, fx.tof, prm, sample_every=every, ctx=gpu_ctx)
        knots = lto.replay_sample_knots(fx.n_knots, every)
        assert r.samples.shape == (7, len(knots), 3) and np.array_equal(r.sample_knots, knots)
        assert np.array_equal(r.x_final, base.x_final) and np.array_equal(r.dv, base.dv)
        assert np.array_equal(r.samples[:, 0, :], X0)                       # knot 0: the start, bit for bit
        assert np.array_equal(r.samples[:, -1, :], r.x_final)               # the last knot: x_final, bit for bit
        e = float(np.max(np.abs(r.samples[:, :, 0] - ref.knots[:, knots])))
        print("MEASURED samples every %d: %.3e (bar %.1e)" % (every, e, bx))
        assert e <= bx


# ------------------------------------------------------------------------------------------------------------- C, edges
def _raw(ctx, nstate=6, n_knots=9, B=2, t0=0.0, t1=0.5, n_hist=1, n_prm=1, integ=None, every=0, null=(), pad=0):
    """lto_control_replay_batch through ctypes with every argument in reach; returns (rc, outputs by name)."""
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)          # noqa: E731
    fx = R.LANE_FIX[0]
    x0, lamv, prm = R.fix_problem(fx)
    nk = max(n_knots, 1)
    L = np.asfortranarray(np.repeat(np.resize(lamv, (3, nk))[:, :, None], max(n_hist, 1), axis=2))
    X = np.asfortranarray(np.repeat(np.resize(np.append(x0, R.MASS), nstate if nstate > 0 else 6)[:, None], max(B, 1), axis=1))
    prms = (lto.LtoParams * max(n_prm, 1))(*[lto.make_params(*prm)] * max(n_prm, 1))
    integ = integ or lto.integrator()
    ns = len(lto.replay_sample_knots(nk, every)) if every > 0 else 0
    Bn = max(B, 1)
    out = dict(x_final=np.full(max(nstate, 6) * Bn + pad, -7.0), samples=np.full(max(nstate, 6) * max(ns, 1) * Bn + pad, -7.0),
               dv=np.full(Bn + pad, -7.0), accepted=np.full(Bn + pad, -7, dtype=np.int32),
               rejected=np.full(Bn + pad, -7, dtype=np.int32), status=np.full(Bn + pad, -7, dtype=np.int32))
    a = {k: (None if k in null else v) for k, v in out.items()}
    rc = ctx.lib.lto_control_replay_batch(ctx.handle, nstate, n_knots, B, t0, t1, None if "lamv" in null else p(L), n_hist,
                                          None if "x0" in null else p(X), None if "prm" in null else prms, n_prm,
                                          None if "integ" in null else C.byref(integ), every, p(a["x_final"]), p(a["samples"]),
                                          p(a["dv"]), p(a["accepted"]), p(a["rejected"]), p(a["status"]))
    return rc, out


@pytest.mark.gpu
def test_refusals(gpu_ctx):
    assert _raw(gpu_ctx)[0] == 0
    for name in ("lamv", "x0", "prm", "integ", "x_final", "dv", "status"):
        assert _raw(gpu_ctx, null=(name,))[0] == -2, name
    assert _raw(gpu_ctx, every=2, null=("samples",))[0] == -2
    assert _raw(gpu_ctx, every=0, null=("samples",))[0] == 0
    assert gpu_ctx.lib.lto_control_replay_batch(None, 6, 9, 1, 0.0, 0.5, None, 1, None, None, 1, None, 0, None, None, None, None, None,
                                                None) == -2
    for kw in (dict(n_knots=3), dict(t1=0.0), dict(t0=0.5, t1=0.25), dict(t1=float("inf")), dict(t1=float("nan")),
               dict(t0=float("-inf")), dict(n_hist=0), dict(n_hist=3, B=2), dict(n_prm=0), dict(n_prm=3, B=2), dict(every=-1),
               dict(B=0), dict(integ=lto.integrator(lto.RK4, steps=0))):
        assert _raw(gpu_ctx, **kw)[0] == -1, kw
    for kw in (dict(nstate=5), dict(nstate=8), dict(nstate=12), dict(integ=lto.integrator(lto.RKF78_FIXED, steps=4)),
               dict(integ=lto.integrator(lto.RKF78_ADAPTIVE))):
        assert _raw(gpu_ctx, **kw)[0] == -3, kw
    assert _raw(gpu_ctx, n_knots=4)[0] == 0 and _raw(gpu_ctx, nstate=7)[0] == 0


@pytest.mark.gpu
def test_outputs_stay_inside_their_extents_and_counters_may_be_null(gpu_ctx):
    rc, full = _raw(gpu_ctx, nstate=7, B=3, every=3, pad=5)
    assert rc == 0 and np.all(full["status"][:3] == 0)
    ns = len(lto.replay_sample_knots(9, 3))
    for k, n in (("x_final", 21), ("samples", 7 * ns * 3), ("dv", 3), ("accepted", 3), ("rejected", 3), ("status", 3)):
        assert np.all(full[k][n:] == -7) and not np.any(full[k][:n] == -7), k
    rc, part = _raw(gpu_ctx, nstate=7, B=3, every=3, pad=5, null=("accepted", "rejected"))
    assert rc == 0
    for k in ("x_final", "samples", "dv", "status"):
        assert np.array_equal(part[k], full[k]), k
    assert np.all(part["accepted"] == -7) and np.all(part["rejected"] == -7)       # not handed to the call
    # the one-start entry is the batch entry at B = 1
    fx = R.LANE_FIX[0]
    x0, lamv, prm = R.fix_problem(fx)
    p = lambda a: a.ctypes.data_as(C.c_void_p)                                     # noqa: E731
    xf, dv, st = np.zeros(6), np.zeros(1), np.full(1, -7, dtype=np.int32)
    integ, pr = lto.integrator(), lto.make_params(*prm)
    L, X = np.asfortranarray(lamv), np.array(x0)
    assert gpu_ctx.lib.lto_control_replay(gpu_ctx.handle, 6, 9, 0.0, 0.5, p(L), p(X), C.byref(pr), C.byref(integ), 0, p(xf), None, p(dv),
                                          None, None, p(st)) == 0
    r = lto.control_replay(x0, lamv, 0.0, 0.5, prm, ctx=gpu_ctx)
    assert st[0] == 0 and np.array_equal(xf, r.x_final) and dv[0] == r.dv


@pytest.mark.gpu
def test_poisoned_starts_fail_alone(gpu_ctx):
    """A NaN start, a start mass that is not positive or not finite: status 2, NaN results, the sample of knot 0 the start as it
    was handed in; the neighbours bit for bit what they are without the poisoned lane."""
    fx = R.CLASS_FIX["m_p2_k9_05"]
    x0, lamv, prm = R.fix_problem(fx)
    X0, _, _ = R.place([(x0, lamv)], 3)
    X0[0, 2] += 1e-3
    good = lto.control_replay(X0, lamv, 0.0, fx.tof, prm, sample_every=4, ctx=gpu_ctx)
    assert np.all(good.status == 0)
    for row, value in ((1, np.nan), (4, np.inf), (6, 0.0), (6, -5.0), (6, np.nan), (6, np.inf)):
        bad = X0.copy(order="F")
        bad[row, 1] = value
        r = lto.control_replay(bad, lamv, 0.0, fx.tof, prm, sample_every=4, ctx=gpu_ctx)
        assert list(r.status) == [0, 2, 0], (row, value)
        assert np.all(np.isnan(r.x_final[:, 1])) and np.isnan(r.dv[1]) and np.all(np.isnan(r.samples[:, 1:, 1]))
        assert np.array_equal(r.samples[:, 0, 1], bad[:, 1], equal_nan=True)
        for b in (0, 2):
            assert np.array_equal(r.x_final[:, b], good.x_final[:, b]) and r.dv[b] == good.dv[b]
            assert np.array_equal(r.samples[:, :, b], good.samples[:, :, b])
            assert r.accepted[b] == good.accepted[b] and r.rejected[b] == good.rejected[b]
    # a NaN in one lane's history
    L = np.asfortranarray(np.repeat(np.asarray(lamv)[:, :, None], 3, axis=2))
    L[2, 5, 1] = np.nan
    r = lto.control_replay(X0, L, 0.0, fx.tof, prm, ctx=gpu_ctx)
    assert list(r.status) == [0, 2, 0] and np.all(np.isnan(r.x_final[:, 1]))
    for b in (0, 2):
        assert np.array_equal(r.x_final[:, b], good.x_final[:, b])


@pytest.mark.gpu
def test_an_interval_out_of_steps_fails_alone(gpu_ctx):
    """max_steps = 3 per interval: the lane whose first interval holds the switch of a p = 1 law at rho = 1e-4 (the reference
    takes 12 steps there) runs out and is NaN from that interval on; its smooth neighbours take a step per interval and are
    bit for bit what they are with the default limit."""
    smooth, steep = R.CLASS_FIX["p2_k65_05"], R.Fix(70, 65, 0.5, 1.0, 1.0, 1e-4)
    ps, pt = R.fix_problem(smooth), R.fix_problem(steep)
    x0 = np.asfortranarray(np.stack([ps[0], pt[0], ps[0]], axis=1))
    x0[1, 2] += 1e-4
    lamv = np.asfortranarray(np.stack([ps[1], pt[1], ps[1]], axis=2))
    prms = [ps[2], pt[2], ps[2]]
    good = lto.control_replay(x0, lamv, 0.0, 0.5, prms, sample_every=16, ctx=gpu_ctx)
    assert np.all(good.status == 0) and good.accepted[1] + good.rejected[1] > good.accepted[0] + 3
    r = lto.control_replay(x0, lamv, 0.0, 0.5, prms, integ=lto.integrator(max_steps=3), sample_every=16, ctx=gpu_ctx)
    assert list(r.status) == [0, 2, 0]
    assert np.all(np.isnan(r.x_final[:, 1])) and np.isnan(r.dv[1]) and np.all(np.isnan(r.samples[:, 1:, 1]))
    assert np.array_equal(r.samples[:, 0, 1], x0[:, 1])
    for b in (0, 2):
        assert np.array_equal(r.x_final[:, b], good.x_final[:, b]) and r.dv[b] == good.dv[b]
        assert np.array_equal(r.samples[:, :, b], good.samples[:, :, b])


# -------------------------------------------------------------------------------------------------------- D, end to end
@functools.lru_cache(maxsize=None)
def _demo_solution():
    spec = importlib.util.spec_from_file_location("halo_demo", os.path.join(ROOT, "examples", "halo_transfer_demo.py"))
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    XC, t, _, flag = demo.solve_p2(verbose=False)
    assert flag == 0
    return XC, t, (MU, DU, TU, 10.0, 1e3, 1.0, 2.0, 1.0)


@pytest.mark.gpu
def test_demo_transfer_flown_from_its_own_start(gpu_ctx):
    XC, t, prm = _demo_solution()
    miss = {}
    for m in (129, 257):
        out = drivers.fly_control(gpu_ctx, XC, t, prm, n_knots=m)
        assert out["status"][0] == 0
        miss[m] = (float(out["miss_r_km"][0]), float(out["miss_v_ms"][0]))
        print("MEASURED demo transfer replayed, %d knots: miss %.6g km, %.6g m/s, dv %.6f m/s, %d steps" % (
            m, miss[m][0], miss[m][1], out["dv_ms"][0], out["accepted"][0]))
    assert miss[257][0] < miss[129][0]


@pytest.mark.gpu
def test_demo_dispersion(gpu_ctx):
    XC, t, prm = _demo_solution()
    nominal = drivers.fly_control(gpu_ctx, XC, t, prm, n_knots=257)
    out = drivers.dispersion(gpu_ctx, XC, t, prm, 256, 1.0, 0.01, seed=11, n_knots=257)
    assert np.all(out["status"] == 0) and out["x_final"].shape == (6, 256)
    assert np.array_equal(out["x_final"][:, 0], nominal["x_final"][:, 0]) and out["dv"][0] == nominal["dv"][0]
    pc = out["percentiles"]
    print("MEASURED dispersion, 256 samples, 1 km / 1 cm/s: nominal %.6g km, median %.6g km, 95 %% %.6g km, 99 %% %.6g km; median %.6g m/s" % (
        nominal["miss_r_km"][0], pc["miss_r_km"][50], pc["miss_r_km"][95], pc["miss_r_km"][99], pc["miss_v_ms"][50]))
    assert pc["miss_r_km"][50] > nominal["miss_r_km"][0]
    assert pc["miss_r_km"][50] <= pc["miss_r_km"][95] <= pc["miss_r_km"][99]
