"""Variable-mass thrust events on the device (k_indirect_events<14>, k_events_compact with the dm column): a shape
sweep of the 14-row lane and of the mass budget through the compaction, against trajectories strung from the lifted segment
templates of tests/thrust_mass_reference.py (tests/test_thrust_mass_host.py holds that reference to itself and every pattern to
the feature it is built for).  Two lifted pools: LOW = (Isp 20 s, 1000 kg), where a p = 3 segment burns 3 % .. 6 % of its mass and
the moving threshold decides crossings, and HIGH = (2000 s, 700 kg), with the dm of engine-off segments near the rounding of the
mass.

Bars, all from the reference's own error (thrust_mass_reference.pool_tolerances, per pool; measured on the CPU):
|t_event - ref| <= max(1e-12 TU, 10 e_t) + 4 eps max|t| with e_t = 8.9e-14 TU (LOW) and 1.9e-15 TU (HIGH), the five-crossing
template against its own e_t = 3.1e-12 / 1.9e-11 TU; dv and propellant relative <= max(1e-12, 10 e) with e_dv = e_dm = 1.0e-9 (LOW)
and 1.5e-9 (HIGH) over the patterns, 7.9e-7 / 8.5e-7 on the all-off patterns, 2.6e-11 / 1.3e-10 on the backward class, and 1.7e-4
on the one-segment rungs of the rounding ladder (q = 1e-15, below the integrators' absolute tolerance).  dm_seg to the
propellant's absolute bar.  The reference dm is -m_i expm1(-kappa q), exactly 0 where that is below half a unit in the last place
of m_i (no template lies within 1 % of that boundary).
Exact: status, n_events, on0, kind, the NaN / 0 tail, dv == wave_sum(dv_seg), propellant == wave_sum(dm_seg), which dm_seg are 0.
No literal tolerance here but the floors 1e-12 and 4 eps max|t|; the RK4 comparison adds steps eps m_i per segment, since that
reference forms dm from the propagated masses, each step rounding m.
Device errors measured on an MI355X (every test prints its own as MEASURED before it asserts), |t - ref| in TU, dv and
propellant relative (the two agree to three digits everywhere: dm carries q's error):
  A budget through the compaction: 1.1e-14, 9.4e-11 (five-crossing template 7.4e-12 against 3.1e-11; all-off patterns 1.7e-6 at
    Isp 20 s against 7.9e-6 and 1.5e-6 at 2000 s against 8.5e-6, with 3 of 63 and 6 of 129 dm_seg exactly 0 there);
  B classes: 1.4e-14 (p = 3 at Isp 20 s), 8.1e-13 (p = 2; p = 1.5 6e-16, p = 3 1.5e-14, backward p = 1 5.8e-12, p = 0 8e-16),
    end-proximity 4.4e-16 and 9.6e-11, |kappa dv_seg - ln(m_i / (m_i - dm_seg))| 1.8e-16 at most; the seven p = 3 segments whose
    crossings the moving threshold decides have the reference's counts; RK4 against the same algorithm 1.1e-15, 6.9e-15 and
    propellant 2.8e-14; the ladder's rungs at 1.5 and 10 half-units 9.8e-5 against 1.7e-3, the three others exactly 0;
  C plumbing: 6.4e-15 (five-crossing template at 2000 s 5.1e-11 against 1.9e-10), 4.0e-11; every bit-equality held."""
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
BUDGET = ("dv", "burn_time", "propellant", "dv_seg", "dm_seg")
WORST = {}
LOW, HIGH = M.pools(M.LOW), M.pools(M.HIGH)


def _note(group, e):
    w = WORST.setdefault(group, [0.0, 0.0, 0.0])
    w[:] = [max(a, b) for a, b in zip(w, e)]
    print("MEASURED group %s so far: |t - ref| %.3e TU, dv rel %.3e, propellant rel %.3e" % (group, w[0], w[1], w[2]))


def _problem(pats, t0=0.0, rk4=None):
    """(XC [14 x n x B], T [n x B], params, placed) of patterns of one length."""
    placed = [M.place(p, t0, rk4_steps=rk4) for p in pats]
    XC = np.asfortranarray(np.stack([p[0] for p in placed], axis=2))
    T = np.asfortranarray(np.stack([p[1] for p in placed], axis=1))
    return XC, T, [lto.make_params(*M.pattern_prm(p)) for p in pats], placed


def _events(ctx, pats, Mx=64, t0=0.0, integ=None, rk4=None, **kw):
    XC, T, prms, placed = _problem(pats, t0, rk4)
    return lto.indirect_events_mass(XC, T, prms, max_events=Mx, integ=integ, ctx=ctx, **kw), placed


def _check(ev, b, pat, placed, Mx, fam, label, group, key=None):
    """check_arcs and check_mass of trajectory b against the pattern's reference, with the bars of its pool (key: the pool of its
    first template unless given) and family."""
    _, t, segs = placed
    ref = M.compact(segs, t, Mx)
    bt, bdv, bdm = M.sweep_bars(key or pat[0][3:], fam)
    e_t, e_dv = R.check_arcs(ev, b, ref.arcs, t, (M.event_bars(pat, segs, bt), bdv), label, abs_time=True)
    _note(group, (e_t, e_dv, M.check_mass(ev, b, ref, bdm, label, zeros=True)))
    return ref


def _check_rocket(ev, b, pat, placed, fam, label):
    """kappa dv_seg against ln(m_i / (m_i - dm_seg)) for every segment, as tests/test_thrust_mass_gpu.py: both sides carry the
    quadrature error the dv bar allows."""
    XC = placed[0]
    k, bdv = M.kappa(M.pattern_prm(pat)), M.sweep_bars(pat[0][3:], fam)[1]
    m_i = XC[6, :-1]
    d = np.abs(k * ev.dv_seg[:, b] - np.log(m_i / (m_i - ev.dm_seg[:, b])))
    bar = abs(k) * bdv * np.abs(ev.dv_seg[:, b]) + 4.0 * M.EPS
    print("MEASURED %s[%d]: |kappa dv_seg - ln(m_i / (m_i - dm_seg))| %.3e (smallest bar %.3e)" % (label, b, d.max(), bar.min()))
    assert np.all(d <= bar)


def _same(a, b, fields=FIELDS):
    return all(np.array_equal(getattr(a, f), getattr(b, f), equal_nan=True) for f in fields)


def _same_column(ev, b, one):
    return all(np.array_equal(np.array(getattr(ev, f))[..., b], np.array(getattr(one, f))[..., 0], equal_nan=True) for f in FIELDS)


# ---- A. the budget through the compaction (p = 1, DOP853 at 1e-13) ---------------------------------------------------------------
@pytest.mark.parametrize("nseg", R.NSEGS)
def test_quiet_and_edges(gpu_ctx, oracle, nseg):
    pats = [R.pat_quiet(nseg, 1, src=LOW), R.pat_quiet(nseg, 0, src=LOW), R.pat_edges(nseg, src=LOW), R.pat_quiet(nseg, 0, src=HIGH)]
    ev, placed = _events(gpu_ctx, pats)
    for b, (fam, name) in enumerate((("rest", "quiet_on"), ("quiet_off", "quiet_off"), ("rest", "edges"), ("quiet_off", "quiet_off at 2000 s"))):
        _check(ev, b, pats[b], placed[b], 64, fam, "%s%d" % (name, nseg), "A")
    assert list(ev.n_events[[0, 1, 3]]) == [0, 0, 0] and np.all(np.isnan(ev.t_event[:, [0, 1, 3]])) and np.all(ev.kind[:, [0, 1, 3]] == 0)
    assert ev.burn_time[0] > 0.0 and ev.burn_time[1] == 0.0 and ev.burn_time[3] == 0.0
    assert ev.n_events[2] == len({0, 63, 64, nseg - 1} & set(range(nseg)))
    assert np.all(ev.dm_seg[:, 0] > 0.0) and np.all(ev.dm_seg[:, 1] > 0.0)
    # all-off at 2000 s: the reference's |dm| against half a unit in the last place of m_i says which dm_seg are exactly 0
    ratio = np.array([M.ratio(tid) for tid in pats[3]])
    assert np.all((ratio < 0.99) | (ratio > 1.01))
    print("MEASURED quiet_off at 2000 s x%d: %d dm_seg exactly 0, the others %.3e .. kg" % (nseg, int(np.sum(ev.dm_seg[:, 3] == 0.0)),
                                                                                        np.min(ev.dm_seg[:, 3][ev.dm_seg[:, 3] != 0.0], initial=np.inf)))
    assert np.array_equal(ev.dm_seg[:, 3] == 0.0, ratio < 0.99) and np.all(ev.dm_seg[:, 3] >= 0.0)


@pytest.mark.parametrize("nseg", (65, 128, 129))
def test_joins_where_the_chunks_meet(gpu_ctx, oracle, nseg):
    pat = R.pat_boundary_joins(nseg, src=LOW)
    ev, placed = _events(gpu_ctx, [pat])
    _check(ev, 0, pat, placed[0], 64, "rest", "joins%d" % nseg, "A")
    t = placed[0][1]
    want = [t[64], t[128]] if nseg == 129 else [t[64]]
    assert ev.n_events[0] == len(want)
    assert list(ev.t_event[:len(want), 0]) == want and list(ev.kind[:len(want), 0]) == [-1, 1][:len(want)]


@pytest.mark.parametrize("nseg", (65, 129))
def test_dense_lists_and_every_max_events(gpu_ctx, oracle, nseg):
    pat = R.pat_dense(nseg, src=LOW)
    full, placed = _events(gpu_ctx, [pat], 300)
    K = int(full.n_events[0])
    assert K > nseg - 1
    _check(full, 0, pat, placed[0], 300, "rest", "dense%d M=300" % nseg, "A")
    for Mx in (1, 63, 64, 65, K - 1, K, K + 1):
        ev, _ = _events(gpu_ctx, [pat], Mx)
        _check(ev, 0, pat, placed[0], Mx, "rest", "dense%d M=%d" % (nseg, Mx), "A")
        assert ev.status[0] == (0 if Mx >= K else 1) and ev.n_events[0] == K
        m = min(Mx, K)
        assert np.array_equal(ev.t_event[:m, 0], full.t_event[:m, 0]) and np.array_equal(ev.kind[:m, 0], full.kind[:m, 0])
        assert np.all(np.isnan(ev.t_event[m:, 0])) and np.all(ev.kind[m:, 0] == 0)
        assert _same(ev, full, BUDGET)


def test_holes(gpu_ctx, oracle):
    pats = [R.pat_holes(at, src=LOW) for at in R.HOLES]
    ev, placed = _events(gpu_ctx, pats, 300)
    for b, at in enumerate(R.HOLES):
        ref = _check(ev, b, pats[b], placed[b], 300, "rest", "holes%s" % (at,), "A")
        first = R.event_owner(placed[b][2]).index(at[0])
        listed = int(np.sum(np.isfinite(ev.t_event[:, b])))
        assert listed == first + R.KEEP and ev.status[b] == 1 and ev.n_events[b] == ref.arcs.n_events > listed
        assert np.all(np.isfinite(ev.dm_seg[:, b])) and np.all(ev.dm_seg[:, b] > 0.0)          # the budget is complete
    # max_events ahead of the hole: the cut rules, the budget as before
    for b, at in enumerate(R.HOLES):
        hole = R.event_owner(placed[b][2]).index(at[0]) + R.KEEP
        Mx = hole - 2
        cut, _ = _events(gpu_ctx, [pats[b]], Mx)
        _check(cut, 0, pats[b], placed[b], Mx, "rest", "holes%s M=%d" % (at, Mx), "A")
        assert cut.status[0] == 1 and np.array_equal(cut.t_event[:, 0], ev.t_event[:Mx, b]) and cut.n_events[0] == ev.n_events[b]
        assert all(np.array_equal(getattr(cut, f)[..., 0], getattr(ev, f)[..., b]) for f in BUDGET)


def test_either_optional_output_alone(gpu_ctx, oracle):
    pats = [R.pat_dense(65, src=LOW), R.pat_quiet(65, 0, src=HIGH), R.pat_holes((30,), 65, src=LOW)]
    full, placed = _events(gpu_ctx, pats)
    for b, fam in enumerate(("rest", "quiet_off", "rest")):
        _check(full, b, pats[b], placed[b], 64, fam, "optional outputs", "A")
    no_dm, _ = _events(gpu_ctx, pats, with_dm_seg=False)
    no_dv, _ = _events(gpu_ctx, pats, with_dv_seg=False)
    assert no_dm.dm_seg is None and no_dm.dv_seg is not None and _same(no_dm, full, [f for f in FIELDS if f != "dm_seg"])
    assert no_dv.dv_seg is None and no_dv.dm_seg is not None and _same(no_dv, full, [f for f in FIELDS if f != "dv_seg"])


# ---- B. classes and integrators --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", M.POOLS, ids=("low", "high"))
@pytest.mark.parametrize("cls", R.CLASSES)
def test_classes_alone(gpu_ctx, oracle, cls, key):
    """p1back: kappa carries time_direction (include/lto.h), so the mass grows along a backward segment: dm_seg <= 0 everywhere
    and propellant < 0.  p3 at Isp 20 s: the segments whose number of crossings differs under a threshold frozen at m_i (the host
    test finds them) have the reference's number of events on the device."""
    pat = R.pat_cycle(cls, src=M.pools(key))
    fam = M.family("cycle_" + cls)
    label = "cycle_%s Isp %g" % (cls, key[0])
    ev, placed = _events(gpu_ctx, [pat], 128, t0=1.7)
    _check(ev, 0, pat, placed[0], 128, fam, label, "B")
    _check_rocket(ev, 0, pat, placed[0], fam, label)
    _, t, segs = placed[0]
    if cls == "p0":
        assert ev.n_events[0] == 0 and ev.on0[0] == 1
    else:
        assert ev.n_events[0] > 4 and ev.status[0] == 0
    if cls == "p1back":
        assert M.kappa(M.pattern_prm(pat)) < 0.0 and np.all(ev.dm_seg[:, 0] <= 0.0) and ev.propellant[0] < 0.0
    else:
        assert np.all(ev.dm_seg[:, 0] >= 0.0) and ev.propellant[0] > 0.0
    if cls == "p3" and key == M.LOW:
        differ = M.mass_driven(M.LOW)[1]
        own = np.array(R.event_owner(segs))
        listed = ev.t_event[:len(own), 0]
        where = [i for i, tid in enumerate(pat) if tid in differ]
        assert len(where) >= 3 and len(own) == ev.n_events[0]
        for i in where:
            mine = listed[own == i]
            inside = int(np.sum((mine > t[i]) & (mine < t[i + 1])))
            joined = int(i + 1 < len(segs) and segs[i].on_e != segs[i + 1].on_s)
            print("MEASURED %s segment %d: %d crossings on the device (reference %d, frozen threshold %d)"
                  % (label, i, inside, len(segs[i].roots), M.tmpl_frozen(pat[i])))
            assert inside == len(segs[i].roots) != M.tmpl_frozen(pat[i]) and len(mine) == inside + joined
            assert int(np.sum((listed > t[i]) & (listed < t[i + 1]))) == inside


def test_classes_in_one_batch(gpu_ctx, oracle):
    order = ("p2", "p1.5", "p3", "p1back", "p0")
    pats = [R.pat_cycle(c, src=LOW) for c in order]
    assert [M.pattern_prm(p)[5:7] for p in pats] == [(1.0, 2.0), (1.0, 1.5), (1.0, 3.0), (-1.0, 1.0), (1.0, 0.0)]
    ev, placed = _events(gpu_ctx, pats, 128, t0=1.7)
    for b, c in enumerate(order):
        _check(ev, b, pats[b], placed[b], 128, M.family("cycle_" + c), "batch of classes " + c, "B")
        one, _ = _events(gpu_ctx, [pats[b]], 128, t0=1.7)
        assert _same_column(ev, b, one), c


def test_crossings_next_to_a_segment_end(gpu_ctx, oracle):
    assert len(M.prox_admitted(M.LOW)) >= 3
    for tid in M.prox_admitted(M.LOW):
        for nseg in (1, 65):
            pat = R.pat_prox(tid, nseg, src=LOW)
            ev, placed = _events(gpu_ctx, [pat])
            _check(ev, 0, pat, placed[0], 64, "rest", "prox %s %g x%d" % (tid[1], tid[2], nseg), "B")
            assert ev.n_events[0] == 1 and ev.status[0] == 0
            t = placed[0][1]
            assert t[nseg - 1] < ev.t_event[0, 0] < t[nseg]


def _check_rk4(ev, pat, placed, Mx, steps, label):
    """Against the device's algorithm restated in numpy.  That reference propagates m itself and forms dm = m_i - m_end, every
    step rounding m: the comparison gets steps eps m_i per segment beside the bar."""
    XC, t, segs = placed
    ref = M.compact(segs, t, Mx)
    bt, bdv, bdm = M.sweep_bars(M.LOW)
    e = R.check_arcs(ev, 0, ref.arcs, t, (bt, bdv), label, t_ulp=1)
    _note("B rk4", e + (M.check_mass(ev, 0, ref, bdm, label, abs_dm=steps * M.EPS * float(np.max(XC[6]))),))


@pytest.mark.parametrize("steps", (1, 2, 16, 64))
def test_rk4_two_crossings(gpu_ctx, oracle, steps):
    pat = [LOW.pick("p1", None, 2)]
    ev, placed = _events(gpu_ctx, [pat], integ=lto.integrator(lto.RK4, steps=steps), rk4=steps)
    _check_rk4(ev, pat, placed[0], 64, steps, "rk4 x%d two crossings" % steps)
    assert ev.n_events[0] == (0 if steps == 1 else 2)


def test_rk4_dense(gpu_ctx, oracle):
    pat = R.pat_dense(65, src=LOW)
    ev, placed = _events(gpu_ctx, [pat], 300, integ=lto.integrator(lto.RK4, steps=16), rk4=16)
    _check_rk4(ev, pat, placed[0], 300, 16, "rk4 x16 dense65")
    assert ev.n_events[0] > 64


def test_rounding_ladder(gpu_ctx, oracle):
    """One engine-off p = 1 node under five Isp: the reference's |dm| at 0.1, 0.7, 1.5 and 10 half-units in the last place of
    m_i, and Isp = 1e30.  dm_seg is exactly 0 below 1 and at 1e30, and not 0 above 1, within the rungs' own bar."""
    rungs = M.ladder()
    pats = [[tid] for tid in rungs]
    ev, placed = _events(gpu_ctx, pats)
    ratio = [M.ratio(tid) for tid in rungs]
    for b, tid in enumerate(rungs):
        print("MEASURED rung %d: Isp %.6g s, reference |dm| / half-ulp %.4g, reference dm %.6e kg, device dm_seg %.6e kg"
              % (b, tid[3], ratio[b], M.tmpl_seg(tid).dm, ev.dm_seg[0, b]))
        _check(ev, b, pats[b], placed[b], 64, "rung", "ladder rung %d" % b, "B ladder", key=M.HIGH)
    assert list(ev.dm_seg[0] == 0.0) == [r < 1.0 for r in ratio] == [True, True, False, False, True]
    assert np.all(ev.status == 0) and np.all(ev.propellant == ev.dm_seg[0])
    assert np.all(ev.n_events == ev.n_events[0]) and np.all(ev.on0 == ev.on0[0])          # p = 1: g does not see the mass
    for f in ("t_event", "kind"):
        assert all(np.array_equal(getattr(ev, f)[:, b], getattr(ev, f)[:, 0], equal_nan=True) for b in range(5))


# ---- C. batch plumbing -----------------------------------------------------------------------------------------------------------
def _plumbing():
    pats = R.pat_plumbing(src=HIGH)
    XC, T, prms, placed = _problem(pats)
    XC[:, 17, 2] = np.nan                                   # trajectory 2: an all-NaN node
    XC[6, 40, 3] = 0.0                                      # trajectory 3: a node without mass
    return pats, XC, T, prms, placed


def test_batch_equals_singles_with_sick_neighbours(gpu_ctx, oracle):
    pats, XC, T, prms, placed = _plumbing()
    ev = lto.indirect_events_mass(XC, T, prms, ctx=gpu_ctx)
    assert list(ev.status) == [1, 0, 2, 2, 1, 0]
    for b in range(6):
        one = lto.indirect_events_mass(XC[:, :, b:b + 1], T[:, b:b + 1], prms[b], ctx=gpu_ctx)
        assert _same_column(ev, b, one), b
        if b not in (2, 3):
            _check(ev, b, pats[b], placed[b], 64, "rest", "plumbing", "C")
    for b in (2, 3):
        assert ev.n_events[b] == 0 and ev.on0[b] == 0 and np.isnan(ev.dv[b]) and np.isnan(ev.burn_time[b]) and np.isnan(ev.propellant[b])
        assert np.all(np.isnan(ev.t_event[:, b])) and np.all(ev.kind[:, b] == 0)
        assert np.all(np.isnan(ev.dv_seg[:, b])) and np.all(np.isnan(ev.dm_seg[:, b]))
    # one parameter set for all is six copies of it
    assert _same(lto.indirect_events_mass(XC, T, prms[0], ctx=gpu_ctx), ev)


def test_one_grid_for_the_batch(gpu_ctx, oracle):
    pats = R.pat_shared_grid(src=LOW)
    XC, T, prms, placed = _problem(pats)
    assert all(np.array_equal(T[:, b], T[:, 0]) for b in range(6))
    each = lto.indirect_events_mass(XC, T, prms, ctx=gpu_ctx)
    shared = lto.indirect_events_mass(XC, np.array(T[:, 0]), prms[0], ctx=gpu_ctx)
    assert _same(shared, each)
    for b in range(6):
        _check(shared, b, pats[b], placed[b], 64, "rest", "shared grid", "C")
    assert len(set(shared.n_events)) >= 3


@pytest.mark.parametrize("fill", (-7.25e300, np.nan))
def test_plan_entry_with_padding(gpu_ctx, oracle, fill):
    import torch
    pats, XC, T, prms, _ = _plumbing()
    n, B = 66, 6
    ldx, S = n * B + 37, (n - 1) * B
    host = {Mx: lto.indirect_events_mass(XC, T, prms, max_events=Mx, ctx=gpu_ctx) for Mx in (64, 7)}
    X = np.full((14, ldx), fill)
    X[:, :n * B] = synth.to_soa_nodes(XC)
    Xd = torch.from_numpy(X).cuda()
    tg = torch.from_numpy(np.ascontiguousarray(T.T.reshape(-1))).cuda()
    plan = lto.IndirectPlan(gpu_ctx, n, B, prms, lto.integrator(), ndim=14)
    defect = torch.zeros(14, S, dtype=torch.float64, device="cuda")
    plan.defect(Xd, ldx, tg, B, defect, S)
    torch.cuda.synchronize()
    counts = plan.step_counts()
    i32 = lambda *s: torch.full(s, -77, dtype=torch.int32, device="cuda")          # noqa: E731
    f64 = lambda *s: torch.full(s, -7.25e300, dtype=torch.float64, device="cuda")  # noqa: E731
    for Mx in (64, 7):                                      # twice on one plan, another max_events the second time
        ne, kd, o0, st = i32(B), i32(B, Mx), i32(B), i32(B)
        te, dv, bt, pr, ds, dm = f64(B, Mx), f64(B), f64(B), f64(B), f64(S), f64(S)
        plan.events_mass(Xd, ldx, tg, B, Mx, ne, te, kd, o0, dv, bt, pr, st, dv_seg=ds, dm_seg=dm)
        torch.cuda.synchronize()
        after = plan.step_counts()
        assert np.array_equal(after[0], counts[0]) and np.array_equal(after[1], counts[1])      # the events call leaves them
        ev = host[Mx]
        assert np.array_equal(ne.cpu().numpy(), ev.n_events) and np.array_equal(st.cpu().numpy(), ev.status)
        assert np.array_equal(o0.cpu().numpy(), ev.on0)
        assert np.array_equal(te.cpu().numpy().T, ev.t_event, equal_nan=True) and np.array_equal(kd.cpu().numpy().T, ev.kind)
        assert np.array_equal(dv.cpu().numpy(), ev.dv, equal_nan=True) and np.array_equal(bt.cpu().numpy(), ev.burn_time, equal_nan=True)
        assert np.array_equal(pr.cpu().numpy(), ev.propellant, equal_nan=True)
        assert np.array_equal(ds.cpu().numpy().reshape(B, n - 1).T, ev.dv_seg, equal_nan=True)
        assert np.array_equal(dm.cpu().numpy().reshape(B, n - 1).T, ev.dm_seg, equal_nan=True)
        d2 = torch.zeros_like(defect)
        plan.defect(Xd, ldx, tg, B, d2, S)                  # a defect sweep in between: the same as before the events call
        torch.cuda.synchronize()
        assert torch.equal(torch.nan_to_num(d2), torch.nan_to_num(defect))
        again = plan.step_counts()
        assert np.array_equal(again[0], counts[0]) and np.array_equal(again[1], counts[1])
    plan.close()


def test_a_segment_out_of_max_steps(gpu_ctx, oracle):
    import torch
    pats = [R.pat_edges(65, src=LOW), R.pat_holes((30,), 65, src=LOW)]
    XC, T, prms, placed = _problem(pats)
    n, B = 66, 2
    S = (n - 1) * B
    plan = lto.IndirectPlan(gpu_ctx, n, B, prms, lto.integrator(), ndim=14)
    Xd = torch.from_numpy(synth.to_soa_nodes(XC)).cuda()
    tg = torch.from_numpy(np.ascontiguousarray(T.T.reshape(-1))).cuda()
    defect = torch.zeros(14, S, dtype=torch.float64, device="cuda")
    plan.defect(Xd, n * B, tg, B, defect, S)
    torch.cuda.synchronize()
    acc, rej = plan.step_counts()
    plan.close()
    total = (acc + rej).reshape(B, n - 1)
    long_steps = int(acc.reshape(B, n - 1)[1, 30])
    short = int(np.max(np.delete(total.reshape(-1), (n - 1) + 30)))
    max_steps = long_steps // 2                             # the events sweep carries q too and resolves the switch: it takes no fewer
    print("MEASURED defect sweep: short segments up to %d steps, the 6 TU segment %d accepted; max_steps = %d" % (short, long_steps, max_steps))
    assert 4 * short <= max_steps                           # and four times the defect sweep's steps are room for the short ones
    integ = lto.integrator(max_steps=max_steps)
    ev = lto.indirect_events_mass(XC, T, prms, integ=integ, ctx=gpu_ctx)
    assert list(ev.status) == [0, 2]
    one = lto.indirect_events_mass(XC[:, :, :1], T[:, :1], prms[0], integ=integ, ctx=gpu_ctx)
    assert _same_column(ev, 0, one)
    _check(ev, 0, pats[0], placed[0], 64, "rest", "beside a segment out of steps", "C")
    assert ev.n_events[1] == 0 and np.isnan(ev.dv[1]) and np.isnan(ev.propellant[1]) and np.all(np.isnan(ev.t_event[:, 1]))
    assert np.all(np.isnan(ev.dv_seg[:, 1])) and np.all(np.isnan(ev.dm_seg[:, 1]))
