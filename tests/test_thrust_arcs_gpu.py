"""Thrust arcs on the device (k_indirect_events, k_events_compact) against tests/thrust_reference.py.

Bars, from the reference's own error (thrust_reference.bars): |t_event - ref| <= max(1e-12 TU, 10 e_t) and
|dv - ref| <= max(1e-12, 10 e_dv) |ref|, with e_t = 4.1e-15 TU (the two CPU determinations of the fixture roots) and
e_dv = 5.5e-9 (the reference dv at rtol = atol = 1e-13 against 1e-12) measured on the CPU -- so 1e-12 TU and 5.5e-8.  burn_time is a
sum of differences of event times: n_events bars, plus rounding.  The five-crossing segment (thrust_reference.EXTRA) is 6 TU long
and is held to its own measured error, e_t = 3.1e-11 TU there.
Device errors measured on an MI355X (every test prints its own as MEASURED before it asserts), |t - ref| in TU and dv relative:
  one crossing 1.2e-16, 3.1e-12;  join only 0 (the event is t[1]), 1.9e-10;  two crossings 7.8e-16, 2.2e-12;
  66 nodes x 3: p = 1 8.9e-16, 1.7e-11;  p = 2 4.2e-15, 1.0e-8;  p = 0 no event, dv and burn_time equal to aL (tf - t0) and tf - t0;
  RK4 x 16 against the same algorithm in numpy 1.4e-17, 4.5e-16;  five crossings 5.0e-11 (own bar 3.1e-10), 1.0e-11."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thrust_reference as R  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu


def _prms(prms):
    return [lto.make_params(*q) for q in prms]


def _events(ctx, name, b=None, integ=None, **kw):
    XC, T, prms = R.case_problem(name)
    if b is None:
        return lto.indirect_events(XC, T, _prms(prms), integ=integ, ctx=ctx, **kw)
    return lto.indirect_events(XC[:, :, b], T[:, b], lto.make_params(*prms[b]), integ=integ, ctx=ctx, **kw)


def _check(ev, b, ref, t, bars, label):
    """Trajectory b of a batched result against its reference Arcs (the rules live in thrust_reference.check_arcs)."""
    R.check_arcs(ev, b, ref, t, bars, label)


def _same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True)
               for f in ("n_events", "t_event", "kind", "on0", "dv", "burn_time", "dv_seg", "status"))


def test_one_crossing_in_one_segment(gpu_ctx, oracle):
    ev = _events(gpu_ctx, "one_crossing")
    _, T, _ = R.case_problem("one_crossing")
    ref = R.case_reference("one_crossing")[0][1]
    _check(ev, 0, ref, T[:, 0], R.bars(), "one_crossing")
    assert ev.n_events[0] == 1 and ev.kind[0, 0] == (-1 if ref.on0 else 1)


def test_join_event_at_the_node(gpu_ctx, oracle):
    ev = _events(gpu_ctx, "join_only")
    _, T, _ = R.case_problem("join_only")
    _check(ev, 0, R.case_reference("join_only")[0][1], T[:, 0], R.bars(), "join_only")
    assert ev.n_events[0] == 1 and ev.t_event[0, 0] == T[1, 0]


def test_two_crossings_many_crossings_and_truncation(gpu_ctx, oracle):
    ev = _events(gpu_ctx, "two_crossings")
    _, T, _ = R.case_problem("two_crossings")
    _check(ev, 0, R.case_reference("two_crossings")[0][1], T[:, 0], R.bars(), "two_crossings")
    assert ev.n_events[0] == 2
    # five crossings in one segment: status 1, the first four listed, dv complete
    ev = _events(gpu_ctx, "many_crossings")
    _, T, _ = R.case_problem("many_crossings")
    ref = R.case_reference("many_crossings")[0][1]
    bt = R.bars(("many_crossings",))[0]
    e_time = float(np.max(np.abs(ev.t_event[:R.KEEP, 0] - ref.t_event[:R.KEEP])))
    e_dv = abs(ev.dv[0] - ref.dv) / abs(ref.dv)
    print("MEASURED many_crossings: n_events %d, |t - ref| %.3e (bar %.1e), dv rel %.3e (bar %.1e)" % (ev.n_events[0], e_time, bt, e_dv, R.bars()[1]))
    assert ev.status[0] == 1 and ev.n_events[0] == 5 and ev.on0[0] == ref.on0
    assert np.array_equal(ev.kind[:, 0], ref.kind) and np.all(np.isnan(ev.t_event[R.KEEP:, 0]))
    assert e_time <= bt and e_dv <= R.bars()[1]
    # more events than max_events: the first one only, everything else as in the full call
    full = _events(gpu_ctx, "mixed66", b=0)
    cut = _events(gpu_ctx, "mixed66", b=0, max_events=1)
    assert cut.status == 1 and full.status == 0 and cut.n_events == full.n_events > 1
    assert cut.t_event.shape == (1,) and cut.t_event[0] == full.t_event[0] and cut.kind[0] == full.kind[0]
    assert cut.dv == full.dv and cut.burn_time == full.burn_time and np.array_equal(cut.dv_seg, full.dv_seg)


def test_mixed_classes_past_one_wavefront(gpu_ctx, oracle):
    XC, T, prms = R.case_problem("mixed66")
    assert XC.shape == (12, 66, 3) and [q[6] for q in prms] == [1.0, 2.0, 0.0]
    ev = _events(gpu_ctx, "mixed66")
    refs = R.case_reference("mixed66")
    for b in range(3):
        _check(ev, b, refs[b][1], T[:, b], R.bars(), "mixed66")
    span = T[-1, 2] - T[0, 2]
    aL = R.accel_limit(prms[2])
    assert ev.n_events[2] == 0 and ev.on0[2] == 1
    assert abs(ev.burn_time[2] - span) <= 1e-13 * span and abs(ev.dv[2] - aL * span) <= 1e-13 * aL * span


def test_batch_singles_repeat_and_plan_are_bit_identical(gpu_ctx, oracle):
    import torch
    XC, T, prms = R.case_problem("mixed66")
    ev = _events(gpu_ctx, "mixed66")
    assert _same(ev, _events(gpu_ctx, "mixed66"))
    for b in range(3):
        one = _events(gpu_ctx, "mixed66", b=b)
        for f in ("t_event", "kind", "dv_seg"):
            assert np.array_equal(getattr(one, f), getattr(ev, f)[:, b], equal_nan=True), (f, b)
        for f in ("n_events", "on0", "dv", "burn_time", "status"):
            assert getattr(one, f) == getattr(ev, f)[b], (f, b)
    n, B, M = 66, 3, 64
    plan = lto.IndirectPlan(gpu_ctx, n, B, _prms(prms), lto.integrator())
    Xd = torch.from_numpy(synth.to_soa_nodes(XC)).cuda()
    tg = torch.from_numpy(np.ascontiguousarray(T.T.reshape(-1))).cuda()
    i32 = lambda *s: torch.full(s, -77, dtype=torch.int32, device="cuda")          # noqa: E731
    f64 = lambda *s: torch.full(s, -7.25e300, dtype=torch.float64, device="cuda")  # noqa: E731
    ne, kd, o0, st = i32(B), i32(B, M), i32(B), i32(B)
    te, dv, bt, ds = f64(B, M), f64(B), f64(B), f64(B * (n - 1))
    plan.events(Xd, n * B, tg, B, M, ne, te, kd, o0, dv, bt, st, dv_seg=ds)
    torch.cuda.synchronize()
    plan.close()
    assert np.array_equal(ne.cpu().numpy(), ev.n_events) and np.array_equal(st.cpu().numpy(), ev.status)
    assert np.array_equal(o0.cpu().numpy(), ev.on0)
    assert np.array_equal(te.cpu().numpy().T, ev.t_event, equal_nan=True) and np.array_equal(kd.cpu().numpy().T, ev.kind)
    assert np.array_equal(dv.cpu().numpy(), ev.dv) and np.array_equal(bt.cpu().numpy(), ev.burn_time)
    assert np.array_equal(ds.cpu().numpy().reshape(B, n - 1).T, ev.dv_seg)


def test_rk4_against_the_same_algorithm(gpu_ctx, oracle):
    integ = lto.integrator(lto.RK4, steps=16)
    ev = _events(gpu_ctx, "one_crossing", integ=integ)
    _, T, _ = R.case_problem("one_crossing")
    _check(ev, 0, R.case_reference("one_crossing", rk4_steps=16)[0][1], T[:, 0], R.bars(), "one_crossing rk4x16")
    no_seg = _events(gpu_ctx, "one_crossing", integ=integ, with_dv_seg=False)      # dv_seg = NULL
    assert no_seg.dv_seg is None and no_seg.dv[0] == ev.dv[0] and no_seg.t_event[0, 0] == ev.t_event[0, 0]


def test_nan_node_poisons_its_trajectory_only(gpu_ctx, oracle):
    XC, T, prms = R.case_problem("mixed66")
    good = lto.indirect_events(XC, T, _prms(prms), ctx=gpu_ctx)
    for k in (7, 65):                                       # an interior node; the last node, which starts no segment
        bad = np.array(XC, order="F")
        bad[4, k, 1] = np.nan
        ev = lto.indirect_events(bad, T, _prms(prms), ctx=gpu_ctx)
        assert list(ev.status) == [0, 2, 0]
        assert ev.n_events[1] == 0 and ev.on0[1] == 0 and np.isnan(ev.dv[1]) and np.isnan(ev.burn_time[1])
        assert np.all(np.isnan(ev.t_event[:, 1])) and np.all(ev.kind[:, 1] == 0) and np.all(np.isnan(ev.dv_seg[:, 1]))
        for b in (0, 2):
            for f in ("t_event", "kind", "dv_seg"):
                assert np.array_equal(getattr(ev, f)[:, b], getattr(good, f)[:, b], equal_nan=True)
            for f in ("n_events", "on0", "dv", "burn_time", "status"):
                assert getattr(ev, f)[b] == getattr(good, f)[b]


def test_refusals(gpu_ctx):
    lib = gpu_ctx.lib
    prm = lto.make_params(lto.MU, lto.DU, lto.TU, 0.05, 1000.0, 1.0, 1.0, 1e-2)

    def call(ndim=12, integ=None, max_events=8, null_status=False, t=(0.0, 0.1)):
        integ = integ or lto.integrator()
        XC = np.asfortranarray(np.full((ndim, 2), 0.5))
        t = np.array(t)
        ne, kd, o0, st = (np.zeros(8, dtype=np.int32) for _ in range(4))
        te, dv, bt = np.zeros(8), np.zeros(1), np.zeros(1)
        p = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731
        return lib.lto_indirect_events_batch(gpu_ctx.handle, ndim, 2, 1, p(XC), p(t), 1, C.byref(prm), 1, C.byref(integ), max_events,
                                             p(ne), p(te), p(kd), p(o0), p(dv), p(bt), None, None if null_status else p(st))
    assert call() == 0
    assert call(ndim=14) == -3
    assert call(integ=lto.integrator(lto.RKF78_FIXED, steps=4)) == -3
    assert call(integ=lto.integrator(lto.RKF78_ADAPTIVE)) == -3
    assert call(max_events=0) == -1
    assert call(t=(0.1, 0.1)) == -1
    assert call(null_status=True) == -2
