"""Thrust events on the device (k_indirect_events, k_events_compact): a shape sweep of the crossing search and of the
compaction, against trajectories strung from the segment templates of tests/thrust_reference.py (a template's reference is
computed once on the CPU; the CRTBP with this control law is autonomous, so the segment has the same crossings, shifted, wherever
it is placed; tests/test_thrust_arcs_host.py holds the reference to that and every pattern to the feature it is built for).

Bars, from the reference's own error (thrust_reference.pool_tolerances; measured on the CPU): |t_event - ref| <=
max(1e-12 TU, 10 e_t) + 4 eps max|t| with e_t = 4.1e-15 TU over all admitted templates (the same as the older fixtures'), the
five-crossing template against its own e_t = 3.1e-11 TU; dv relative <= max(1e-12, 10 e_dv) with e_dv = 6.6e-9 over the patterns
(p = 2; older fixtures 5.5e-9) -- but 9.2e-7 on the all-off patterns, whose dv is 1e-7 .. 4e-5 DU/TU, so that the integrators'
absolute 1e-13 weighs more: they have a bar of their own so as not to widen every other pattern's.  Autonomy of the reference: 1.8e-15 TU at most between a template integrated at t_i = 0, 1.7, 12.3.
Exact: status, n_events, on0, kind, the NaN / 0 tail beyond the listed events, dv == wave_sum(dv_seg).
Device errors measured on an MI355X (every test prints its own as MEASURED before it asserts), |t - ref| in TU and dv relative:
  A compaction shapes: 3.6e-15, 7.2e-9 (five-crossing template 5.0e-11 against 3.1e-10; all-off patterns 7.8e-7 against 9.2e-6);
  B classes and integrators: 4.4e-15, 1.0e-8 (p = 2; backward p = 1 1.3e-9, p = 1.5 1.4e-10, p = 3 5.9e-11, end-proximity
    3.1e-10), RK4 against the same algorithm 3.3e-16, 1.5e-15;
  C plumbing: 1.3e-15 (five-crossing template 5.0e-11), 2.4e-10; every bit-equality held."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thrust_reference as R  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
FIELDS = ("n_events", "t_event", "kind", "on0", "dv", "burn_time", "dv_seg", "status")
WORST = {}


def _note(group, e):
    w = WORST.setdefault(group, [0.0, 0.0])
    w[0], w[1] = max(w[0], e[0]), max(w[1], e[1])
    print("MEASURED group %s so far: |t - ref| %.3e TU, dv rel %.3e" % (group, w[0], w[1]))


def _problem(pats, t0=0.0, rk4=None):
    """(XC [12 x n x B], T [n x B], params, placed) of patterns of one length."""
    placed = [R.place(p, t0, rk4_steps=rk4) for p in pats]
    XC = np.asfortranarray(np.stack([p[0] for p in placed], axis=2))
    T = np.asfortranarray(np.stack([p[1] for p in placed], axis=1))
    return XC, T, [lto.make_params(*R.pattern_prm(p)) for p in pats], placed


def _events(ctx, pats, M=64, t0=0.0, integ=None, rk4=None, **kw):
    XC, T, prms, placed = _problem(pats, t0, rk4)
    return lto.indirect_events(XC, T, prms, max_events=M, integ=integ, ctx=ctx, **kw), placed


def _check(ev, b, pat, placed, M, family, label, group, t_ulp=0):
    _, t, segs = placed
    ref = R.compact(segs, t, M)
    bt, bdv = R.sweep_bars(family)
    e = R.check_arcs(ev, b, ref, t, (R.event_bars(pat, segs, bt), bdv), label, abs_time=True, t_ulp=t_ulp)
    _note(group, e)
    return ref


def _same(a, b, fields=FIELDS):
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) for f in fields)


def _column(ev, b):
    return [np.array(getattr(ev, f))[..., b] for f in FIELDS]


def _same_column(ev, b, one):
    return all(np.array_equal(x, y[..., 0], equal_nan=True) for x, y in zip(_column(ev, b), [np.array(getattr(one, f)) for f in FIELDS]))


# ---- A. compaction shapes (p = 1, DOP853 at 1e-13) ------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg", R.NSEGS)
def test_quiet_and_edges(gpu_ctx, oracle, nseg):
    pats = [R.pat_quiet(nseg, 1), R.pat_quiet(nseg, 0), R.pat_edges(nseg)]
    ev, placed = _events(gpu_ctx, pats)
    for b, fam in enumerate(("quiet_on", "quiet_off", "edges")):
        _check(ev, b, pats[b], placed[b], 64, fam, "%s%d" % (fam, nseg), "A")
    T = placed[0][1]
    span, aL = T[-1] - T[0], R.accel_limit(R.pattern_prm(pats[0]))
    assert ev.n_events[0] == 0 and ev.n_events[1] == 0 and np.all(np.isnan(ev.t_event[:, :2])) and np.all(ev.kind[:, :2] == 0)
    assert abs(ev.burn_time[0] - span) <= 1e-13 * span and ev.burn_time[1] == 0.0
    assert 0.5 * aL * span < ev.dv[0] <= aL * span          # p = 1: on is more than half thrust, the law saturates only far from g = 0
    assert ev.n_events[2] == len({0, 63, 64, nseg - 1} & set(range(nseg)))


@pytest.mark.parametrize("nseg", (65, 128, 129))
def test_joins_where_the_chunks_meet(gpu_ctx, oracle, nseg):
    pat = R.pat_boundary_joins(nseg)
    ev, placed = _events(gpu_ctx, [pat])
    _check(ev, 0, pat, placed[0], 64, "joins", "joins%d" % nseg, "A")
    t = placed[0][1]
    want = [t[64], t[128]] if nseg == 129 else [t[64]]
    assert list(ev.t_event[:len(want), 0]) == want and list(ev.kind[:len(want), 0]) == [-1, 1][:len(want)]


@pytest.mark.parametrize("nseg", (65, 129))
def test_dense_lists_and_every_max_events(gpu_ctx, oracle, nseg):
    pat = R.pat_dense(nseg)
    full, placed = _events(gpu_ctx, [pat], 300)
    K = int(full.n_events[0])
    assert K > nseg - 1
    _check(full, 0, pat, placed[0], 300, "dense", "dense%d M=300" % nseg, "A")
    for M in (1, 63, 64, 65, K - 1, K, K + 1):
        ev, _ = _events(gpu_ctx, [pat], M)
        _check(ev, 0, pat, placed[0], M, "dense", "dense%d M=%d" % (nseg, M), "A")
        assert ev.status[0] == (0 if M >= K else 1) and ev.n_events[0] == K
        m = min(M, K)
        assert np.array_equal(ev.t_event[:m, 0], full.t_event[:m, 0]) and np.array_equal(ev.kind[:m, 0], full.kind[:m, 0])
        assert np.all(np.isnan(ev.t_event[m:, 0])) and np.all(ev.kind[m:, 0] == 0)
        assert _same(ev, full, ("dv", "burn_time", "dv_seg"))


def test_holes(gpu_ctx, oracle):
    pats = [R.pat_holes(at) for at in R.HOLES]
    ev, placed = _events(gpu_ctx, pats, 300)
    for b, at in enumerate(R.HOLES):
        ref = _check(ev, b, pats[b], placed[b], 300, "holes", "holes%s" % (at,), "A")
        first = R.event_owner(placed[b][2]).index(at[0])
        listed = int(np.sum(np.isfinite(ev.t_event[:, b])))
        assert listed == first + R.KEEP and ev.status[b] == 1 and ev.n_events[b] == ref.n_events > listed
    # max_events ahead of the hole: the cut rules, everything else as before
    for b, at in enumerate(R.HOLES):
        hole = R.event_owner(placed[b][2]).index(at[0]) + R.KEEP
        M = hole - 2
        cut, _ = _events(gpu_ctx, [pats[b]], M)
        _check(cut, 0, pats[b], placed[b], M, "holes", "holes%s M=%d" % (at, M), "A")
        assert cut.status[0] == 1 and np.array_equal(cut.t_event[:, 0], ev.t_event[:M, b]) and cut.n_events[0] == ev.n_events[b]
        assert cut.dv[0] == ev.dv[b] and cut.burn_time[0] == ev.burn_time[b]


# ---- B. classes and integrators -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", R.CLASSES)
def test_classes_alone(gpu_ctx, oracle, cls):
    pat = R.pat_cycle(cls)
    prm = R.pattern_prm(pat)
    ev, placed = _events(gpu_ctx, [pat], 128, t0=1.7)
    _check(ev, 0, pat, placed[0], 128, "cycle_" + cls, "cycle_" + cls, "B")
    if cls == "p0":
        span = placed[0][1][-1] - placed[0][1][0]
        assert ev.n_events[0] == 0 and abs(ev.dv[0] - R.accel_limit(prm) * span) <= 1e-13 * R.accel_limit(prm) * span
    else:
        assert ev.n_events[0] > 4 and ev.status[0] == 0


def test_classes_in_one_batch(gpu_ctx, oracle):
    order = ("p1", "p2", "p1.5", "p0", "p1back")
    pats = [R.pat_cycle(c) for c in order]
    assert [R.pattern_prm(p)[5:7] for p in pats] == [(1.0, 1.0), (1.0, 2.0), (1.0, 1.5), (1.0, 0.0), (-1.0, 1.0)]
    ev, placed = _events(gpu_ctx, pats, 128, t0=1.7)
    for b, c in enumerate(order):
        fam = "plumbing" if c == "p1" else "cycle_" + c
        _check(ev, b, pats[b], placed[b], 128, fam, "batch of classes " + c, "B")
        one, _ = _events(gpu_ctx, [pats[b]], 128, t0=1.7)
        assert _same_column(ev, b, one), c


def test_crossings_next_to_a_segment_end(gpu_ctx, oracle):
    assert len(R.prox_admitted()) >= 3
    for tid in R.prox_admitted():
        for nseg in (1, 65):
            pat = R.pat_prox(tid, nseg)
            ev, placed = _events(gpu_ctx, [pat])
            _check(ev, 0, pat, placed[0], 64, "prox", "prox %s %g x%d" % (tid[1], tid[2], nseg), "B")
            assert ev.n_events[0] == 1 and ev.status[0] == 0
            t = placed[0][1]
            assert t[nseg - 1] < ev.t_event[0, 0] < t[nseg]


@pytest.mark.parametrize("steps", (1, 2, 16, 64))
def test_rk4_two_crossings(gpu_ctx, oracle, steps):
    pat = [R.pick("p1", None, 2)]
    integ = lto.integrator(lto.RK4, steps=steps)
    ev, placed = _events(gpu_ctx, [pat], integ=integ, rk4=steps)
    ref = R.compact(placed[0][2], placed[0][1], 64)
    _note("B", R.check_arcs(ev, 0, ref, placed[0][1], R.bars(), "rk4 x%d two crossings" % steps, t_ulp=1))
    assert ev.n_events[0] == (0 if steps == 1 else 2)


def test_rk4_dense(gpu_ctx, oracle):
    pat = R.pat_dense(65)
    ev, placed = _events(gpu_ctx, [pat], 300, integ=lto.integrator(lto.RK4, steps=16), rk4=16)
    ref = R.compact(placed[0][2], placed[0][1], 300)
    _note("B", R.check_arcs(ev, 0, ref, placed[0][1], R.bars(), "rk4 x16 dense65", t_ulp=1))
    assert ev.n_events[0] > 64


# ---- C. batch plumbing ----------------------------------------------------------------------------------------------------------
def _plumbing():
    pats = R.pat_plumbing()
    XC, T, prms, placed = _problem(pats)
    XC[:, 17, 2] = np.nan                                   # trajectory 2: an all-NaN node
    return pats, XC, T, prms, placed


def test_batch_equals_singles_with_sick_neighbours(gpu_ctx, oracle):
    pats, XC, T, prms, placed = _plumbing()
    ev = lto.indirect_events(XC, T, prms, ctx=gpu_ctx)
    assert list(ev.status) == [1, 0, 2, 0, 1, 0]
    for b in range(6):
        one = lto.indirect_events(XC[:, :, b:b + 1], T[:, b:b + 1], prms[b], ctx=gpu_ctx)
        assert _same_column(ev, b, one), b
        if b != 2:
            _check(ev, b, pats[b], placed[b], 64, "plumbing", "plumbing", "C")
    assert ev.n_events[2] == 0 and ev.on0[2] == 0 and np.isnan(ev.dv[2]) and np.isnan(ev.burn_time[2])
    assert np.all(np.isnan(ev.t_event[:, 2])) and np.all(ev.kind[:, 2] == 0) and np.all(np.isnan(ev.dv_seg[:, 2]))
    # one parameter set for all is six copies of it; no dv_seg changes nothing else
    assert _same(lto.indirect_events(XC, T, prms[0], ctx=gpu_ctx), ev)
    bare = lto.indirect_events(XC, T, prms, ctx=gpu_ctx, with_dv_seg=False)
    assert bare.dv_seg is None and _same(bare, ev, [f for f in FIELDS if f != "dv_seg"])


def test_one_grid_for_the_batch(gpu_ctx, oracle):
    pats = R.pat_shared_grid()
    XC, T, prms, placed = _problem(pats)
    assert all(np.array_equal(T[:, b], T[:, 0]) for b in range(6))
    each = lto.indirect_events(XC, T, prms, ctx=gpu_ctx)
    shared = lto.indirect_events(XC, np.array(T[:, 0]), prms[0], ctx=gpu_ctx)
    assert _same(shared, each)
    for b in range(6):
        _check(shared, b, pats[b], placed[b], 64, "shared", "shared grid", "C")
    assert len(set(shared.n_events)) >= 3


@pytest.mark.parametrize("fill", (-7.25e300, np.nan))
def test_plan_entry_with_padding(gpu_ctx, oracle, fill):
    import torch
    pats, XC, T, prms, _ = _plumbing()
    n, B = 66, 6
    ldx, S = n * B + 37, (n - 1) * B
    host = {M: lto.indirect_events(XC, T, prms, max_events=M, ctx=gpu_ctx) for M in (64, 7)}
    X = np.full((12, ldx), fill)
    X[:, :n * B] = synth.to_soa_nodes(XC)
    Xd = torch.from_numpy(X).cuda()
    tg = torch.from_numpy(np.ascontiguousarray(T.T.reshape(-1))).cuda()
    plan = lto.IndirectPlan(gpu_ctx, n, B, prms, lto.integrator())
    defect = torch.zeros(12, S, dtype=torch.float64, device="cuda")
    plan.defect(Xd, ldx, tg, B, defect, S)
    torch.cuda.synchronize()
    counts = plan.step_counts()
    i32 = lambda *s: torch.full(s, -77, dtype=torch.int32, device="cuda")          # noqa: E731
    f64 = lambda *s: torch.full(s, -7.25e300, dtype=torch.float64, device="cuda")  # noqa: E731
    for M in (64, 7):                                       # twice on one plan, another max_events the second time
        ne, kd, o0, st = i32(B), i32(B, M), i32(B), i32(B)
        te, dv, bt, ds = f64(B, M), f64(B), f64(B), f64(S)
        plan.events(Xd, ldx, tg, B, M, ne, te, kd, o0, dv, bt, st, dv_seg=ds)
        torch.cuda.synchronize()
        after = plan.step_counts()
        assert np.array_equal(after[0], counts[0]) and np.array_equal(after[1], counts[1])      # the events call leaves them
        ev = host[M]
        assert np.array_equal(ne.cpu().numpy(), ev.n_events) and np.array_equal(st.cpu().numpy(), ev.status)
        assert np.array_equal(o0.cpu().numpy(), ev.on0)
        assert np.array_equal(te.cpu().numpy().T, ev.t_event, equal_nan=True) and np.array_equal(kd.cpu().numpy().T, ev.kind)
        assert np.array_equal(dv.cpu().numpy(), ev.dv, equal_nan=True) and np.array_equal(bt.cpu().numpy(), ev.burn_time, equal_nan=True)
        assert np.array_equal(ds.cpu().numpy().reshape(B, n - 1).T, ev.dv_seg, equal_nan=True)
        d2 = torch.zeros_like(defect)
        plan.defect(Xd, ldx, tg, B, d2, S)                  # a defect sweep in between: the same as before the events call
        torch.cuda.synchronize()
        assert torch.equal(torch.nan_to_num(d2), torch.nan_to_num(defect))
        again = plan.step_counts()
        assert np.array_equal(again[0], counts[0]) and np.array_equal(again[1], counts[1])
    plan.close()


def test_a_segment_out_of_max_steps(gpu_ctx, oracle):
    import torch
    pats = [R.pat_edges(65), R.pat_holes((30,), 65)]
    XC, T, prms, placed = _problem(pats)
    n, B = 66, 2
    S = (n - 1) * B
    plan = lto.IndirectPlan(gpu_ctx, n, B, prms, lto.integrator())
    Xd = torch.from_numpy(synth.to_soa_nodes(XC)).cuda()
    tg = torch.from_numpy(np.ascontiguousarray(T.T.reshape(-1))).cuda()
    defect = torch.zeros(12, S, dtype=torch.float64, device="cuda")
    plan.defect(Xd, n * B, tg, B, defect, S)
    torch.cuda.synchronize()
    acc, rej = plan.step_counts()
    plan.close()
    total = (acc + rej).reshape(B, n - 1)
    long_steps = int(acc.reshape(B, n - 1)[1, 30])
    short = int(np.max(np.delete(total.reshape(-1), (n - 1) + 30)))
    max_steps = long_steps // 2                             # the events sweep carries q too and resolves the switch: it takes no fewer
    print("defect sweep: short segments up to %d steps, the 6 TU segment %d accepted; max_steps = %d" % (short, long_steps, max_steps))
    assert 4 * short <= max_steps                           # and four times the defect sweep's steps are room for the short ones
    integ = lto.integrator(max_steps=max_steps)
    ev = lto.indirect_events(XC, T, prms, integ=integ, ctx=gpu_ctx)
    assert list(ev.status) == [0, 2]
    one = lto.indirect_events(XC[:, :, :1], T[:, :1], prms[0], integ=integ, ctx=gpu_ctx)
    assert _same_column(ev, 0, one)
    _check(ev, 0, pats[0], placed[0], 64, "edges", "beside a segment out of steps", "C")
    assert ev.n_events[1] == 0 and np.isnan(ev.dv[1]) and np.all(np.isnan(ev.t_event[:, 1])) and np.all(np.isnan(ev.dv_seg[:, 1]))
