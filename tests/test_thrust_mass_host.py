"""The variable-mass thrust-arc reference (tests/thrust_mass_reference.py) against itself, the Python layers of
hotpath.indirect_events_mass / drivers.thrust_arcs_mass without a device, and the ABI table.

Below them the lifted segment templates and the patterns of tests/test_thrust_mass_shapes_gpu.py.  Measured here, pools
(20 s, 1000 kg) / (2000 s, 700 kg): e_t 8.9e-14 / 1.9e-15 TU (five-crossing template 3.1e-12 / 1.9e-11), e_dv = e_dm 1.0e-9 /
1.5e-9 over the patterns, 7.9e-7 / 8.5e-7 on the all-off ones, 2.6e-11 / 1.3e-10 on the backward class, 1.7e-4 on the ladder's
rungs; autonomy 4.4e-16 TU; p3 at 20 s: 4 of 17 roots with the threshold's rate above half of dg/dt, 7 templates with another
crossing count under a frozen threshold; no template's |dm| within 1 % of half a unit in the last place of m_i (nearest 0.633)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thrust_mass_reference as M  # noqa: E402
import thrust_reference as R  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import _lib, drivers, hotpath  # noqa: E402

SMALL_FIXTURES = [f for f in M.FIXTURES if f[0] in M.SMALL]


def test_two_determinations_agree_and_fixtures_are_admitted(oracle):
    e_t, e_dv, e_dm = M.tolerances(tuple(SMALL_FIXTURES))
    print("MEASURED small fixtures: e_t %.3e TU, e_dv %.3e, e_dm %.3e" % (e_t, e_dv, e_dm))
    assert all(M.admitted(*f) for f in SMALL_FIXTURES)
    assert e_t <= 1e-13 and e_dv <= 1e-8 and e_dm <= 1e-8
    counts = {f: [len(s.roots) for segs, _ in M.case_reference(*f) for s in segs] for f in SMALL_FIXTURES}
    for isp, m0 in M.COMBOS:
        assert counts[("one_crossing", isp, m0)] == [1] and counts[("join_only", isp, m0)] == [0, 0]
        assert counts[("two_crossings", isp, m0)] == [2]
        assert M.case_reference("join_only", isp, m0)[0][1].arcs.n_events == 1            # the join at t[1]


def test_reference_is_autonomous(oracle):
    """A segment started at another t_i has its roots shifted by as much, the same q and dm."""
    XC, T, prms = M.case_problem("two_crossings", 2000.0, 700.0)
    a = M.case_reference("two_crossings", 2000.0, 700.0)[0][0][0]
    b = M.seg_reference(oracle, XC[:, 0, 0], 3.25, 3.25 + (T[1, 0] - T[0, 0]), prms[0])
    d = np.abs(np.array(b.roots) - 3.25 - (np.array(a.roots) - T[0, 0]))
    print("MEASURED shift 3.25 TU: roots %.3e TU, q %.3e, dm %.3e" % (d.max(), abs(a.q - b.q), abs(a.dm - b.dm)))
    assert len(b.roots) == 2 and d.max() <= 1e-12 + 4 * M.EPS * 4.0
    assert abs(a.q - b.q) <= 1e-8 * a.q and abs(a.dm - b.dm) <= 1e-8 * a.dm


def test_rocket_equation_in_the_reference(oracle):
    worst = 0.0
    for f in SMALL_FIXTURES:
        XC, T, prms = M.case_problem(*f)
        for b, (segs, _) in enumerate(M.case_reference(*f)):
            for i, s in enumerate(segs):
                worst = max(worst, abs(M.kappa(prms[b]) * s.q - np.log(XC[6, i, b] / s.m_end)))
    print("MEASURED |kappa q - ln(m_i / m_end)| %.3e" % worst)
    assert worst <= 1e-14


def test_fixtures_tell_the_two_systems_apart(oracle):
    """The 14-row roots lie more than 100 bars from the 12-row roots of the same nodes: the 12-row kernel on the 12 sub-rows
    would not pass."""
    bar = 1e-12

    def gap(name, isp, m0, b, i):
        r14 = M.case_reference(name, isp, m0)[b][0][i].roots
        r12 = R.case_reference(name)[b][0][i].roots
        assert len(r14) == len(r12) > 0
        return np.abs(np.array(r14) - np.array(r12))
    g1 = gap("two_crossings", 2000.0, 700.0, 0, 0)
    print("MEASURED 0.6 TU p = 1 segment at 700 kg: 14-row roots off the 12-row ones by", g1)
    assert g1[1] > 100 * bar
    XC, T, prms = M.case_problem("mixed66", 2000.0, 1000.0)
    assert prms[1][6] == 2.0
    segs14, segs12 = M.case_reference("mixed66", 2000.0, 1000.0)[1][0], R.case_reference("mixed66")[1][0]
    g2 = [abs(a - c) for s, r in zip(segs14, segs12) if len(s.roots) == len(r.roots) for a, c in zip(s.roots, r.roots)]
    print("MEASURED p = 2, 66 nodes: %d roots, off by %.3e .. %.3e TU" % (len(g2), min(g2), max(g2)))
    assert len(g2) > 10 and max(g2) > 100 * bar


def test_shapes_are_validated_without_a_device():
    prm = lto.make_params(lto.MU, lto.DU, lto.TU, 0.05, 2000.0, 1.0, 1.0, 1e-2)
    assert callable(lto.indirect_events_mass) and callable(drivers.thrust_arcs_mass) and callable(lto.IndirectPlan.events_mass)
    with pytest.raises(ValueError):
        lto.indirect_events_mass(np.zeros((12, 3)), np.zeros(3), prm)                 # 12 rows
    with pytest.raises(ValueError):
        lto.indirect_events_mass(np.zeros((14, 3)), np.zeros(2), prm)                 # t of another length
    with pytest.raises(ValueError):
        lto.indirect_events_mass(np.zeros((14, 3, 2)), np.zeros((3, 3)), prm)         # grids of another batch
    with pytest.raises(ValueError):
        lto.indirect_events_mass(np.zeros((14, 3, 4)), np.zeros(3), [prm, prm])       # neither one nor B parameter sets
    with pytest.raises(ValueError):
        lto.indirect_events_mass(np.ones((14, 3)), np.arange(3.0), lto.make_params(lto.MU, lto.DU, lto.TU, 0.05, 0.0, 1.0, 1.0, 1e-2))
    with pytest.raises(ValueError):
        drivers.thrust_arcs_mass(np.zeros((12, 3)), np.zeros(3), lto.MU, lto.DU, lto.TU, 2000.0, 0.05, 1.0, 1e-2)
    with pytest.raises(ValueError):
        drivers.thrust_arcs_mass(np.zeros((14, 3)), np.zeros(4), lto.MU, lto.DU, lto.TU, 2000.0, 0.05, 1.0, 1e-2)
    with pytest.raises(ValueError):
        drivers.thrust_arcs_mass(np.ones((14, 3)), np.arange(3.0), lto.MU, lto.DU, lto.TU, -5.0, 0.05, 1.0, 1e-2)
    with pytest.raises(ValueError):
        drivers.thrust_arcs_mass(np.ones((14, 3, 2)), np.arange(3.0), lto.MU, lto.DU, lto.TU, [2000.0, 0.0], 0.05, 1.0, 1e-2)


def test_the_new_entries_are_in_the_abi_table():
    names = {"lto_indirect_events_mass_batch", "lto_indirect_events_mass", "lto_indirect_events_mass_dev"}
    assert names <= set(_lib.SIGNATURES)
    # propellant and dm_seg behind dv_seg; no ndim in the host forms
    assert len(_lib.SIGNATURES["lto_indirect_events_mass_batch"][1]) == len(_lib.SIGNATURES["lto_indirect_events_batch"][1]) + 1
    assert len(_lib.SIGNATURES["lto_indirect_events_mass"][1]) == len(_lib.SIGNATURES["lto_indirect_events"][1]) + 1
    assert len(_lib.SIGNATURES["lto_indirect_events_mass_dev"][1]) == len(_lib.SIGNATURES["lto_indirect_events_dev"][1]) + 2
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lto.h")).read()
    assert all(("int %s(" % n) in header for n in names)


def test_driver_arcs_and_mass_budget_arithmetic():
    """drivers' clipping and budget on a hand-made ThrustEvents: trajectory 0 starts on, off at 0.2, on at 0.5 (open at tf);
    trajectory 1 starts off, on at 0.3, truncated (status 1: no closing arc)."""
    nan = np.nan
    ev = hotpath.ThrustEvents(np.array([2, 3], dtype=np.int32), np.array([[0.2, 0.3], [0.5, nan], [nan, nan]]),
                              np.array([[-1, 1], [1, 0], [0, 0]], dtype=np.int32), np.array([1, 0], dtype=np.int32),
                              np.array([0.01, 0.02]), np.array([0.7, 0.4]), None, np.array([0, 1], dtype=np.int32),
                              np.array([2.5, 0.0]), None)
    t = np.array([0.0, 0.4, 1.0])
    out = drivers._mass_budget(ev, np.array([1000.0, 700.0]), np.array([2000.0, 20.0]), lto.DU, lto.TU, t, 3)
    assert out[0]["arcs"] == [(0.0, 0.2), (0.5, 1.0)] and out[1]["arcs"] == []
    assert out[0]["propellant_kg"] == 2.5 and out[0]["mass_final_kg"] == 997.5
    assert out[0]["dv_rocket_ms"] == 2000.0 * 9.81 * np.log(1000.0 / 997.5)
    assert out[0]["dv_ms"] == 0.01 * lto.DU / lto.TU * 1e3 and out[0]["burn_days"] == 0.7 * lto.TU / 86400.0
    assert out[1]["mass_final_kg"] == 700.0 and out[1]["dv_rocket_ms"] == 0.0 and out[1]["status"] == 1 and out[1]["n_events"] == 3


# ---- segment templates of the 14-row system and the patterns of tests/test_thrust_mass_shapes_gpu.py ----------------------------
def _arcs(pattern, Mx=64, t0=0.0):
    XC, t, segs = M.place(pattern, t0)
    return XC, t, segs, M.compact(segs, t, Mx)


def _joins(segs):
    return [i + 1 for i, (a, b) in enumerate(zip(segs[:-1], segs[1:])) if a.on_e != b.on_s]


@pytest.mark.parametrize("key", M.POOLS)
def test_lifted_pools_admit_every_class(oracle, key):
    from collections import Counter
    src = M.pools(key)
    for cls, srcs in R.POOL_SRC.items():
        total = sum(R._spec(name)[b].n - 1 for name, b in srcs)
        kinds = Counter(M.klass(tid) for tid in src.pool(cls))
        print("MEASURED pool %s at Isp %g s, %g kg: %d of %d admitted, %s" % ((cls,) + key + (len(src.pool(cls)), total, sorted(kinds.items()))))
        assert len(src.pool(cls)) > 0
        if cls == "p0":
            assert set(kinds) == {(1, 0, 1)}
        else:
            assert {(0, 0, 0), (1, 0, 1), (0, 1, 1), (1, 1, 0)} <= set(kinds), cls
        for tid in src.pool(cls):
            y0, L, prm = M.tmpl_node(tid)
            assert tid[3:] == key and prm[4] == key[0] and y0[6] == key[1] - M.DM_NODE * tid[2] and L > 0
    assert src.FIVE in src.pool("p1") and M.klass(src.FIVE) == (0, 5, 1)
    assert M.klass(("two_crossings", 0, 0) + key) == (1, 2, 1) and ("two_crossings", 0, 0) + key in src.pool("p1")
    assert all(M.tmpl_node(tid)[2][6] == 3.0 for tid in src.pool("p3")) and all(M.tmpl_node(tid)[2][6] == 1.5 for tid in src.pool("p1.5"))
    assert all(M.tmpl_node(tid)[2][5:7] == (-1.0, 1.0) for tid in src.pool("p1back"))
    assert len({M.tmpl_node(tid)[1] for tid in src.pool("p1u")}) == 1
    dropped = [tid for tid in M.prox_ids(key) if tid not in M.prox_admitted(key)]
    print("MEASURED proximity templates dropped:", dropped or "none")
    assert len(dropped) <= 1 and {tid[1] for tid in M.prox_admitted(key)} == {"start", "end"}
    base = M.tmpl_node(R.PROX_BASE + key)[1]
    for tid in M.prox_admitted(key):                        # the crossing lies delta from the segment's start or end
        (root,), L = M.tmpl_seg(tid).roots, M.tmpl_node(tid)[1]
        gap = root if tid[1] == "start" else L - root
        assert abs(gap - tid[2] * base) <= 1e-9 * base, (tid, gap)


@pytest.mark.parametrize("key", M.POOLS)
def test_lifted_pool_tolerances_and_bars(oracle, key):
    e_t, e_five, e_dv, e_dm = M.pool_tolerances(key)
    print("MEASURED pool Isp %g s, %g kg: e_t %.3e TU (five-crossing template %.3e)" % (key + (e_t, e_five)))
    print("MEASURED   e_dv", {k: "%.3e" % v for k, v in e_dv.items()}, "e_dm", {k: "%.3e" % v for k, v in e_dm.items()})
    assert e_t <= 1e-13 and e_five <= 1e-10               # as the 12-row pools: every slope is >= 0.1 and both integrate at 1e-13
    assert e_dv["rest"] <= 1e-7 and e_dm["rest"] <= 1e-7 and e_dv["back"] <= 1e-7 and e_dm["back"] <= 1e-7
    assert e_dv["quiet_off"] <= 1e-5 and e_dm["quiet_off"] <= 1e-5       # dv of an all-off pattern is nearly 0 (12-row docstring)
    fams = {"rest", "quiet_off", "back"} | ({"rung"} if key == M.HIGH else set())
    assert set(e_dv) == set(e_dm) == fams
    if key == M.HIGH:
        assert e_dm["rung"] <= 1e-3                         # one segment whose q is 1e-15, below the integrators' absolute 1e-13
    for fam in fams:
        assert M.sweep_bars(key, fam) == (max(1e-12, 10 * e_t), max(1e-12, 10 * e_dv[fam]), max(1e-12, 10 * e_dm[fam]))
    assert M.five_bar(key) == max(1e-12, 10 * e_five)


@pytest.mark.parametrize("key", M.POOLS)
def test_rocket_form_of_dm_against_the_subtraction(oracle, key):
    """Where m_i - m_end has digits (|dm| > 1e4 eps m) it agrees with -m_i expm1(-kappa q) to 1e-14 m_i = 45 eps m, the bound
    test_rocket_equation_in_the_reference holds kappa q - ln(m_i / m_end) to: the integrator rounds m in every step and controls
    its error relative to m, not to dm."""
    n, worst = 0, 0.0
    for cls in R.POOL_SRC:
        for tid in M.pool(cls, *key):
            s, m_i = M.tmpl_seg(tid), float(M.tmpl_node(tid)[0][6])
            assert (s.dm >= 0.0) == (M.tmpl_node(tid)[2][5] > 0) or s.dm == 0.0
            if abs(s.dm) > 1e4 * M.EPS * m_i:
                n += 1
                worst = max(worst, abs(s.dm - s.dm_sub) / (M.EPS * m_i))
    print("MEASURED pool Isp %g s, %g kg: %d templates with digits in m_i - m_end, |dm - dm_sub| up to %.2f eps m" % (key + (n, worst)))
    assert n > 100 and worst * M.EPS <= 1e-14


def test_lifted_reference_is_autonomous(oracle):
    worst = 0.0
    low, high = M.pools(M.LOW), M.pools(M.HIGH)
    for tid in (low.pick("p3", 0, 1), low.pick("p1", None, 2), high.pick("p2", 1, 1), M.mass_driven(M.LOW)[1][0]):
        y0, L, prm = M.tmpl_node(tid)
        s0 = M.tmpl_seg(tid)
        e_t = M.pool_tolerances(tid[3:])[0]
        for ti in (0.0, 1.7, 12.3):
            s = M.seg_reference(oracle, y0, ti, ti + L, prm)
            assert (s.on_s, len(s.roots), s.on_e) == M.klass(tid)
            if s.roots:
                d = float(np.max(np.abs(np.array(s.roots) - (ti + np.array(s0.roots)))))
                worst = max(worst, d)
                assert d <= e_t + 4 * M.EPS * abs(ti + L), (tid, ti, d)
            assert abs(s.q - s0.q) <= 1e-11 * abs(s0.q)
    print("MEASURED autonomy: largest |root(t_i) - (t_i + tau)| = %.3e TU" % worst)


def test_the_moving_threshold_decides_in_pool_p3_at_low_isp(oracle):
    half, differ = M.mass_driven(M.LOW)
    n_roots = sum(len(M.tmpl_seg(tid).roots) for tid in M.pool("p3", *M.LOW))
    share = max(abs(th) / abs(x) for tid in M.pool("p3", *M.LOW) for x, th in zip(M.tmpl_seg(tid).slopes, M.tmpl_seg(tid).thr))
    burn = [M.tmpl_seg(tid).dm / M.tmpl_node(tid)[0][6] for tid in M.pool("p3", *M.LOW) if M.klass(tid) == (1, 0, 1)]
    print("MEASURED p3 at Isp 20 s: threshold's rate more than half of dg/dt at %d of %d roots (largest share %.2f), %d templates "
          "with another crossing count under a frozen threshold: %s; all-on templates burn %.3f .. %.3f of their mass"
          % (half, n_roots, share, len(differ), [t[2] for t in differ], min(burn), max(burn)))
    assert half >= 3 and len(differ) >= 3
    assert set(differ) <= set(R.pat_cycle("p3", src=M.pools(M.LOW)))        # the GPU pattern holds every one of them
    print("MEASURED p3 at Isp 2000 s: %d roots, %d templates" % (M.mass_driven(M.HIGH)[0], len(M.mass_driven(M.HIGH)[1])))


def test_rounding_ladder_and_every_template_clear_of_half_an_ulp(oracle):
    rungs = M.ladder()
    ratios = [M.ratio(tid) for tid in rungs]
    print("MEASURED ladder on template %s: Isp %s s, |dm| / half-ulp %s" % (rungs[0][:3], ["%.6g" % t[3] for t in rungs], ["%.6g" % r for r in ratios]))
    for tid, r, want in zip(rungs, ratios, M.RUNGS):
        assert abs(r - want) <= 1e-3 * want
    assert ratios[-1] < 1e-20 and rungs[-1][3] == M.ISP_INF
    assert all(abs(r - 1.0) > 0.01 for r in ratios)
    y0, L, prm = M.tmpl_node(rungs[0])
    assert prm[5:7] == (1.0, 1.0) and M.half_ulp(float(y0[6]), 1.0) == 0.5 * (y0[6] - np.nextafter(y0[6], 0.0))
    for tid in rungs:
        y, Lk, _ = M.tmpl_node(tid)
        assert np.array_equal(y, y0) and Lk == L and M.klass(tid) == (0, 0, 0) and M.admitted_tmpl(tid)
    assert [M.ruled_dm(tid) == 0.0 for tid in rungs] == [True, True, False, False, True]
    # every template of both pools: no |dm| within 1 % of half a unit in the last place (fifty times the 1.7e-4 spread of dm)
    for key in M.POOLS:
        rs = [M.ratio(tid) for cls in R.POOL_SRC for tid in M.pool(cls, *key)] + [M.ratio(tid) for tid in M.prox_admitted(key)]
        near = sorted(r for r in rs if 0.5 < r < 2.0)
        print("MEASURED pool Isp %g s, %g kg: smallest |dm| / half-ulp %.3g, between 0.5 and 2: %s, below 1: %d of %d"
              % (key + (min(rs), ["%.3f" % r for r in near], sum(r < 1 for r in rs), len(rs))))
        assert all(abs(r - 1.0) > 0.01 for r in rs)


def test_lifted_patterns_realise_their_features(oracle):
    low, high = M.sweep_patterns(M.LOW), M.sweep_patterns(M.HIGH)
    for n in R.NSEGS:
        for P in (low, high):
            for on in (1, 0):
                _, t, segs, a = _arcs(P["quiet_%s%d" % ("on" if on else "off", n)][1])
                assert len(segs) == n and a.arcs.n_events == 0 and a.arcs.on0 == on and a.arcs.status == 0
                assert (a.propellant > 0.0) if on else (a.propellant >= 0.0)
            _, t, segs, a = _arcs(P["edges%d" % n][1])
            want = sorted({0, 63, 64, n - 1} & set(range(n)))
            assert R.event_owner(segs) == want and not _joins(segs) and [len(s.roots) for s in segs] == [int(i in want) for i in range(n)]
    # all-off at HIGH: from 63 segments on, dm_seg exactly 0 and not 0 side by side
    for n in (63, 64, 65, 128, 129):
        dm = _arcs(high["quiet_off%d" % n][1])[3].dm_seg
        assert 0 < np.sum(dm == 0.0) < n
    assert all(np.all(_arcs(low["quiet_off%d" % n][1])[3].dm_seg > 0.0) for n in R.NSEGS)
    for n in (65, 128, 129):
        _, t, segs, a = _arcs(low["joins%d" % n][1])
        want = [64, 128] if n == 129 else [64]
        assert _joins(segs) == want and not any(s.roots for s in segs) and list(a.arcs.t_event[:len(want)]) == [t[i] for i in want]
        assert a.arcs.n_events == len(want)
    for n in (65, 129):
        _, t, segs, a = _arcs(low["dense%d" % n][1], 300)
        K = a.arcs.n_events
        print("MEASURED dense%d: K = %d events, %d joins" % (n, K, len(_joins(segs))))
        assert all(len(s.roots) in (1, 2) for s in segs) and n - 1 < K < 299 and a.arcs.status == 0 and K > 66
        assert any(len(s.roots) == 2 for s in segs) and _joins(segs)
    for at in R.HOLES:
        pat = low["holes" + "_".join(map(str, at))][1]
        _, t, segs, a = _arcs(pat, 300)
        own = R.event_owner(segs)
        first = own.index(at[0])
        listed = int(np.sum(np.isfinite(a.arcs.t_event)))
        assert [i for i, s in enumerate(segs) if len(s.roots) > R.KEEP] == list(at) and all(pat[i] == M.five(M.LOW) for i in at)
        assert listed == first + R.KEEP and a.arcs.status == 1 and a.arcs.n_events == len(own) > listed + 1
        assert (first > 0) == (at[0] > 0) and own[-1] > at[-1]
        assert np.all(np.isfinite(a.dm_seg)) and a.propellant > 0.0        # the budget is complete whatever the list drops
    for key, P in ((M.LOW, low), (M.HIGH, high)):
        for cls in R.CLASSES:
            _, t, segs, a = _arcs(P["cycle_" + cls][1], 128, 1.7)
            print("MEASURED cycle_%s at Isp %g s: %d events, %d joins, propellant %.6e kg" % (cls, key[0], a.arcs.n_events, len(_joins(segs)), a.propellant))
            if cls == "p0":
                assert a.arcs.n_events == 0 and a.arcs.on0 == 1
            else:
                assert a.arcs.status == 0 and any(s.roots for s in segs) and _joins(segs) and 4 < a.arcs.n_events <= 128
            if cls == "p1back":
                assert np.all(a.dm_seg <= 0.0) and a.propellant < 0.0
            else:
                assert np.all(a.dm_seg >= 0.0) and a.propellant > 0.0
    for tid in M.prox_admitted(M.LOW):
        for n in (1, 65):
            _, t, segs, a = _arcs(low["prox_%s_%g_%d" % (tid[1], tid[2], n)][1])
            assert a.arcs.n_events == 1 and R.event_owner(segs) == [n - 1]
    pl = R.pat_plumbing(src=M.pools(M.HIGH))
    counts = [_arcs(p)[3].arcs for p in pl]
    assert len({a.n_events for a in counts}) >= 5 and [a.status for a in counts] == [1, 0, 0, 0, 1, 0]
    assert counts[0].n_events > 64 and M.five(M.HIGH) in pl[4]
    sh = R.pat_shared_grid(src=M.pools(M.LOW))
    shared = [M.place(p) for p in sh]
    assert all(np.array_equal(s[1], shared[0][1]) for s in shared)
    assert len({tuple(p) for p in sh}) == 6 and len({M.compact(s[2], s[1]).arcs.n_events for s in shared}) >= 3


def test_lifted_rk4_patterns(oracle):
    low = M.pools(M.LOW)
    two = [low.pick("p1", None, 2)]
    counts = {}
    for steps in (1, 2, 16, 64):
        _, t, segs = M.place(two, rk4_steps=steps)
        counts[steps] = len(segs[0].roots)
    print("MEASURED RK4 on the lifted two-crossing template, events per step count:", counts)
    assert counts[1] == 0 and counts[16] == 2 and counts[64] == 2
    _, t, segs = M.place(R.pat_dense(65, src=low), rk4_steps=16)
    a = M.compact(segs, t, 300)
    assert a.arcs.n_events > 64 and a.arcs.status == 0
