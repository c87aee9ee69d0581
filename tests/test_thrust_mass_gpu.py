"""Variable-mass thrust arcs on the device (k_indirect_events<14>, k_events_compact) against
tests/thrust_mass_reference.py.

Bars, from the reference's own error (thrust_mass_reference.bars): |t_event - ref| <= max(1e-12 TU, 10 e_t) + 4 eps max|t|,
|dv - ref| <= 10 e_dv |ref|, |propellant - ref| <= 10 e_dm |ref|, with e_t = 8.9e-14 TU, e_dv = 2.5e-9 and e_dm = 2.5e-9 measured
on the CPU -- so 1e-12 TU, 2.5e-8 and 2.5e-8.  Every test prints its own errors as MEASURED before it asserts.
Measured on an MI355X, |t - ref| in TU, dv and propellant relative:
  one crossing 4.2e-17 .. 2.2e-16, 5.2e-11;  join only 0 (the event is t[1]), 2.3e-10;  two crossings 8.3e-15, 6.4e-11;
  66 nodes x 3 at Isp 2000 s: p = 1 8.9e-16, 1.3e-12, 1.2e-12;  p = 2 4.2e-15, 1.0e-12, 1.4e-12;  p = 0 no event, propellant 1.7e-13;
  at Isp 20 s: p = 1 6.7e-16, 1.2e-11;  p = 2 3.6e-15, 5.1e-13;  p = 0 propellant 0;
  p = 0 dm_seg against thrustLimit / (Isp 9.81) TU dt: 1.6e-15 (Isp 2000 s), 1.8e-15 (Isp 20 s), bar 1e-13.  (With the mass itself as
  the lane's state this was 2.6e-12 at Isp 2000 s, eps m / dm of a double near 1000 kg; the lane now carries the mass change.)
  |kappa dv_seg - ln(m_i / (m_i - dm_seg))| 1.8e-16 at most (bars 8.9e-16 .. 4e-10, every segment inside its own);
  RK4 x 16: 2.2e-16, 1.3e-15, 5.5e-12;  Isp = 1e30 against the 12-row entry: 4.4e-16 TU, dv 4.9e-11, propellant 0.0."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thrust_mass_reference as M  # noqa: E402
import thrust_reference as R  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

FIELDS = ("n_events", "t_event", "kind", "on0", "dv", "burn_time", "dv_seg", "propellant", "dm_seg", "status")
PER_SEG = ("t_event", "kind", "dv_seg", "dm_seg")
PER_TRAJ = ("n_events", "on0", "dv", "burn_time", "propellant", "status")


def _prms(prms):
    return [lto.make_params(*q) for q in prms]


def _events(ctx, fix, b=None, integ=None, **kw):
    XC, T, prms = M.case_problem(*fix)
    if b is None:
        return lto.indirect_events_mass(XC, T, _prms(prms), integ=integ, ctx=ctx, **kw)
    return lto.indirect_events_mass(XC[:, :, b], T[:, b], lto.make_params(*prms[b]), integ=integ, ctx=ctx, **kw)


def _same(a, b):
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) for f in FIELDS)


def _check_rocket(ev, fix, label):
    """kappa dv_seg against ln(m_i / (m_i - dm_seg)) for every segment: both sides carry the quadrature error the dv bar allows."""
    XC, T, prms = M.case_problem(*fix)
    bdv = M.bars()[1]
    for b, prm in enumerate(prms):
        k = M.kappa(prm)
        m_i = XC[6, :-1, b]
        d = np.abs(k * ev.dv_seg[:, b] - np.log(m_i / (m_i - ev.dm_seg[:, b])))
        bar = k * bdv * np.abs(ev.dv_seg[:, b]) + 4.0 * M.EPS
        print("MEASURED %s[%d]: |kappa dv_seg - ln(m_i / (m_i - dm_seg))| %.3e (smallest bar %.3e)" % (label, b, d.max(), bar.min()))
        assert np.all(d <= bar)


def _check(ev, fix, refs, label):
    _, T, _ = M.case_problem(*fix)
    bt, bdv, bdm = M.bars()
    for b, (_, ref) in enumerate(refs):
        R.check_arcs(ev, b, ref.arcs, T[:, b], (bt, bdv), label, abs_time=True)
        M.check_mass(ev, b, ref, bdm, label)


@pytest.mark.parametrize("isp,m0", M.COMBOS)
def test_one_crossing_join_only_two_crossings(gpu_ctx, oracle, isp, m0):
    for name, n_ev in (("one_crossing", 1), ("join_only", 1), ("two_crossings", 2)):
        fix = (name, isp, m0)
        ev = _events(gpu_ctx, fix)
        label = "%s Isp %g m0 %g" % fix
        _check(ev, fix, M.case_reference(*fix), label)
        _check_rocket(ev, fix, label)
        assert ev.n_events[0] == n_ev
        if name == "join_only":
            assert ev.t_event[0, 0] == M.case_problem(*fix)[1][1, 0]


@pytest.mark.parametrize("isp", (2000.0, 20.0))
def test_mixed_classes_past_one_wavefront(gpu_ctx, oracle, isp):
    fix = ("mixed66", isp, 1000.0)
    XC, T, prms = M.case_problem(*fix)
    assert XC.shape == (14, 66, 3) and [q[6] for q in prms] == [1.0, 2.0, 0.0]
    ev = _events(gpu_ctx, fix)
    label = "mixed66 Isp %g" % isp
    _check(ev, fix, M.case_reference(*fix), label)
    _check_rocket(ev, fix, label)
    # p = 0: always on, and the mass falls linearly: any RK formula integrates that exactly
    span = T[-1, 2] - T[0, 2]
    rate = prms[2][3] / (isp * 9.81) * lto.TU                       # kg per TU
    want = rate * np.diff(T[:, 2])
    e_bt = abs(ev.burn_time[2] - span) / span
    e_dm = float(np.max(np.abs(ev.dm_seg[:, 2] - want) / want))
    print("MEASURED %s p = 0: burn_time rel %.3e, dm_seg against thrustLimit / (Isp 9.81) TU dt rel %.3e (bar 1e-13)" % (label, e_bt, e_dm))
    assert ev.n_events[2] == 0 and ev.on0[2] == 1
    assert e_bt <= 1e-13
    assert e_dm <= 1e-13


def test_sums_follow_the_documented_order(gpu_ctx, oracle):
    """propellant == wave_sum(dm_seg) and dv == wave_sum(dv_seg) bit for bit, with 130 nodes for three chunks of the compaction."""
    XC66, T66, prms = M.case_problem("mixed66", 2000.0, 1000.0)
    XC = np.asfortranarray(np.concatenate([XC66[:, :, 0], XC66[:, :65, 0][:, ::-1]], axis=1)[:, :130])
    t = np.concatenate([[0.0], np.cumsum(np.resize(np.diff(T66[:, 0]), 129))])
    assert XC.shape == (14, 130)
    ev = lto.indirect_events_mass(XC, t, lto.make_params(*prms[0]), max_events=128, ctx=gpu_ctx)
    print("MEASURED 130 nodes: n_events %d, status %d, propellant %.6e kg, dv %.6e" % (ev.n_events, ev.status, ev.propellant, ev.dv))
    assert ev.status == 0 and ev.n_events > 3
    assert ev.propellant == R.wave_sum(ev.dm_seg) and ev.dv == R.wave_sum(ev.dv_seg)
    ev66 = _events(gpu_ctx, ("mixed66", 2000.0, 1000.0))
    for b in range(3):
        assert ev66.propellant[b] == R.wave_sum(ev66.dm_seg[:, b]) and ev66.dv[b] == R.wave_sum(ev66.dv_seg[:, b])


def test_infinite_isp_reduces_to_the_constant_mass_system(gpu_ctx, oracle):
    XC0, T, prms = M.case_problem("mixed66", 2000.0, 1000.0)
    XC = np.array(XC0, order="F")
    XC[6] = 1000.0
    p14 = [lto.make_params(q[0], q[1], q[2], q[3], 1e30, q[5], q[6], q[7]) for q in prms]
    p12 = [lto.make_params(q[0], q[1], q[2], q[3], 1000.0, q[5], q[6], q[7]) for q in prms]
    ev = lto.indirect_events_mass(XC, T, p14, ctx=gpu_ctx)
    old = lto.indirect_events(np.asfortranarray(XC[M.IDX12]), T, p12, ctx=gpu_ctx)
    bt, bdv = R.bars()
    k = int(old.n_events.max())
    d_t = float(np.nanmax(np.abs(ev.t_event[:k] - old.t_event[:k])))
    e_dv = float(np.max(np.abs(ev.dv - old.dv) / np.abs(old.dv)))
    print("MEASURED Isp 1e30 against the 12-row entry: |t - t12| %.3e TU (bar %.1e), dv rel %.3e (bar %.1e), propellant %r"
          % (d_t, bt, e_dv, bdv, list(ev.propellant)))
    assert np.array_equal(ev.n_events, old.n_events) and np.array_equal(ev.kind, old.kind) and np.array_equal(ev.on0, old.on0)
    assert np.array_equal(np.isnan(ev.t_event), np.isnan(old.t_event))
    assert d_t <= bt + 4.0 * M.EPS * float(np.max(np.abs(T))) and e_dv <= bdv
    assert np.all(ev.propellant == 0.0) and np.all(ev.dm_seg == 0.0)


def test_rk4_against_the_same_algorithm(gpu_ctx, oracle):
    integ = lto.integrator(lto.RK4, steps=16)
    for fix in (("one_crossing", 2000.0, 700.0), ("two_crossings", 20.0, 1000.0)):
        ev = _events(gpu_ctx, fix, integ=integ)
        _check(ev, fix, M.case_reference(*fix, rk4_steps=16), "%s rk4x16" % fix[0])


def test_batch_singles_repeat_plan_and_null_outputs_are_bit_identical(gpu_ctx, oracle):
    import torch
    fix = ("mixed66", 2000.0, 1000.0)
    XC, T, prms = M.case_problem(*fix)
    ev = _events(gpu_ctx, fix)
    assert _same(ev, _events(gpu_ctx, fix))
    for b in range(3):
        one = _events(gpu_ctx, fix, b=b)
        for f in PER_SEG:
            assert np.array_equal(getattr(one, f), getattr(ev, f)[:, b], equal_nan=True), (f, b)
        for f in PER_TRAJ:
            assert getattr(one, f) == getattr(ev, f)[b], (f, b)
    # dm_seg = NULL and dv_seg = NULL
    bare = _events(gpu_ctx, fix, with_dv_seg=False, with_dm_seg=False)
    assert bare.dv_seg is None and bare.dm_seg is None
    assert all(np.array_equal(getattr(bare, f), getattr(ev, f), equal_nan=True) for f in FIELDS if f not in ("dv_seg", "dm_seg"))
    # max_events = 1: status 1, the first event only, dv and propellant complete
    full = _events(gpu_ctx, fix, b=0)
    cut = _events(gpu_ctx, fix, b=0, max_events=1)
    assert cut.status == 1 and full.status == 0 and cut.n_events == full.n_events > 1
    assert cut.t_event.shape == (1,) and cut.t_event[0] == full.t_event[0] and cut.kind[0] == full.kind[0]
    assert cut.dv == full.dv and cut.burn_time == full.burn_time and cut.propellant == full.propellant
    assert np.array_equal(cut.dv_seg, full.dv_seg) and np.array_equal(cut.dm_seg, full.dm_seg)
    # the _dev entry: a leading dimension with room behind the nodes, sentinel-filled outputs
    n, B, Mx = 66, 3, 64
    ldx = n * B + 37
    plan = lto.IndirectPlan(gpu_ctx, n, B, _prms(prms), lto.integrator(), ndim=14)
    soa = np.full((14, ldx), 1e300)
    soa[:, :n * B] = synth.to_soa_nodes(XC)
    Xd = torch.from_numpy(soa).cuda()
    tg = torch.from_numpy(np.array(T.T.reshape(-1))).cuda()
    i32 = lambda *s: torch.full(s, -77, dtype=torch.int32, device="cuda")          # noqa: E731
    f64 = lambda *s: torch.full(s, -7.25e300, dtype=torch.float64, device="cuda")  # noqa: E731
    ne, kd, o0, st = i32(B), i32(B, Mx), i32(B), i32(B)
    te, dv, bt, pr, ds, dm = f64(B, Mx), f64(B), f64(B), f64(B), f64(B * (n - 1)), f64(B * (n - 1))
    plan.events_mass(Xd, ldx, tg, B, Mx, ne, te, kd, o0, dv, bt, pr, st, dv_seg=ds, dm_seg=dm)
    torch.cuda.synchronize()
    plan.close()
    assert np.array_equal(ne.cpu().numpy(), ev.n_events) and np.array_equal(st.cpu().numpy(), ev.status)
    assert np.array_equal(o0.cpu().numpy(), ev.on0)
    assert np.array_equal(te.cpu().numpy().T, ev.t_event, equal_nan=True) and np.array_equal(kd.cpu().numpy().T, ev.kind)
    assert np.array_equal(dv.cpu().numpy(), ev.dv) and np.array_equal(bt.cpu().numpy(), ev.burn_time)
    assert np.array_equal(pr.cpu().numpy(), ev.propellant)
    assert np.array_equal(ds.cpu().numpy().reshape(B, n - 1).T, ev.dv_seg)
    assert np.array_equal(dm.cpu().numpy().reshape(B, n - 1).T, ev.dm_seg)


def test_nan_node_and_zero_mass_poison_their_trajectory_only(gpu_ctx, oracle):
    fix = ("mixed66", 2000.0, 1000.0)
    XC, T, prms = M.case_problem(*fix)
    good = _events(gpu_ctx, fix)
    for row, k, value in ((4, 7, np.nan), (4, 65, np.nan), (6, 7, 0.0), (6, 65, 0.0), (6, 0, -3.0)):
        bad = np.array(XC, order="F")
        bad[row, k, 1] = value
        ev = lto.indirect_events_mass(bad, T, _prms(prms), ctx=gpu_ctx)
        assert list(ev.status) == [0, 2, 0], (row, k, value)
        assert ev.n_events[1] == 0 and ev.on0[1] == 0 and np.isnan(ev.dv[1]) and np.isnan(ev.burn_time[1]) and np.isnan(ev.propellant[1])
        assert np.all(np.isnan(ev.t_event[:, 1])) and np.all(ev.kind[:, 1] == 0)
        assert np.all(np.isnan(ev.dv_seg[:, 1])) and np.all(np.isnan(ev.dm_seg[:, 1]))
        for b in (0, 2):
            for f in PER_SEG:
                assert np.array_equal(getattr(ev, f)[:, b], getattr(good, f)[:, b], equal_nan=True)
            for f in PER_TRAJ:
                assert getattr(ev, f)[b] == getattr(good, f)[b]


def test_refusals(gpu_ctx):
    import torch
    lib = gpu_ctx.lib
    prm = lto.make_params(lto.MU, lto.DU, lto.TU, 0.05, 2000.0, 1.0, 1.0, 1e-2)
    p = lambda a: a.ctypes.data_as(C.c_void_p)          # noqa: E731

    def call(integ=None, max_events=8, null=None, t=(0.0, 0.1)):
        integ = integ or lto.integrator()
        XC = np.asfortranarray(np.full((14, 2), 0.5))
        XC[6] = 1000.0
        t = np.array(t)
        ne, kd, o0, st = (np.zeros(8, dtype=np.int32) for _ in range(4))
        te, dv, bt, pr = np.zeros(8), np.zeros(1), np.zeros(1), np.zeros(1)
        return lib.lto_indirect_events_mass_batch(gpu_ctx.handle, 2, 1, p(XC), p(t), 1, C.byref(prm), 1, C.byref(integ), max_events,
                                                  p(ne), p(te), p(kd), p(o0), p(dv), p(bt), None,
                                                  None if null == "propellant" else p(pr), None, None if null == "status" else p(st))
    assert call() == 0
    assert call(integ=lto.integrator(lto.RKF78_FIXED, steps=4)) == -3
    assert call(integ=lto.integrator(lto.RKF78_ADAPTIVE)) == -3
    assert call(max_events=0) == -1
    assert call(t=(0.1, 0.1)) == -1
    assert call(null="propellant") == -2
    assert call(null="status") == -2
    # a 12-row plan into the _dev entry
    prm12 = lto.make_params(lto.MU, lto.DU, lto.TU, 0.05, 1000.0, 1.0, 1.0, 1e-2)
    plan = lto.IndirectPlan(gpu_ctx, 2, 1, [prm12], lto.integrator())
    Xd = torch.full((14, 2), 0.5, dtype=torch.float64, device="cuda")
    td = torch.tensor([0.0, 0.1], dtype=torch.float64, device="cuda")
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device="cuda")          # noqa: E731
    f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device="cuda")        # noqa: E731
    with pytest.raises(lto.LtoError) as err:
        plan.events_mass(Xd, 2, td, 1, 8, i32(1), f64(8), i32(8), i32(1), f64(1), f64(1), f64(1), i32(1))
    torch.cuda.synchronize()
    plan.close()
    assert err.value.code == -3
    # the old entry still refuses 14 rows
    XC = np.asfortranarray(np.full((14, 2), 0.5))
    t = np.array([0.0, 0.1])
    ne, kd, o0, st = (np.zeros(8, dtype=np.int32) for _ in range(4))
    te, dv, bt = np.zeros(8), np.zeros(1), np.zeros(1)
    integ = lto.integrator()
    assert lib.lto_indirect_events_batch(gpu_ctx.handle, 14, 2, 1, p(XC), p(t), 1, C.byref(prm), 1, C.byref(integ), 8, p(ne), p(te),
                                         p(kd), p(o0), p(dv), p(bt), None, p(st)) == -3
