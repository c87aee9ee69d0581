"""Thrust arcs, host side: the reference of tests/thrust_reference.py against itself, the conditions its fixtures
have to meet, and the shape validation of the Python entry points -- no GPU.

Measured here: e_t = 4.1e-15 TU (two CPU determinations of the fixture roots), e_dv = 5.5e-9 (reference dv at 1e-13 against 1e-12).
Segment templates and the patterns of the shape sweep: e_t = 4.1e-15 TU over all admitted templates (five-crossing template
3.1e-11), e_dv = 6.6e-9 over the patterns (9.2e-7 on the all-off ones), autonomy of the reference 1.8e-15 TU; no end-proximity
template is dropped."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import thrust_reference as R  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers  # noqa: E402

ALL = list(R.CASES) + list(R.EXTRA)


def test_two_references_agree(oracle):
    e_t, e_dv = R.tolerances()
    print("e_t = %.3e TU, e_dv = %.3e" % (e_t, e_dv))
    assert e_t <= 1e-13            # the roots are well conditioned: both determinations integrate at 1e-13 and every slope is >= 0.1
    assert e_dv <= 1e-7
    bt, bdv = R.bars()
    assert bt == max(1e-12, 10 * e_t) and bdv == max(1e-12, 10 * e_dv)


@pytest.mark.parametrize("name", ALL)
def test_lists_alternate_and_sums_close(oracle, name):
    XC, T, prms = R.case_problem(name)
    for b, (segs, a) in enumerate(R.case_reference(name)):
        for s in segs:
            assert s.on_e == s.on_s ^ (len(s.roots) & 1)          # the integrator saw every crossing it stepped over
        k = min(a.n_events, 64 if a.status == 0 else R.KEEP)
        kinds, times = a.kind[:k], a.t_event[:k]
        assert np.all(kinds[1:] == -kinds[:-1]) and (k == 0 or kinds[0] == (-1 if a.on0 else 1))
        assert np.all(np.diff(times) > 0) and np.all(np.isnan(a.t_event[k:])) and np.all(a.kind[k:] == 0)
        assert a.dv == R.wave_sum(a.dv_seg)
        if a.status == 0:
            edges = np.concatenate([[T[0, b]] if a.on0 else [], times, [T[-1, b]] if (a.on0 + k) % 2 else []])
            arcs = edges.reshape(-1, 2)
            assert abs(np.sum(arcs[:, 1] - arcs[:, 0]) - a.burn_time) <= 1e-13 * (T[-1, b] - T[0, b])


def test_fixture_conditions(oracle):
    for name in ALL:
        for segs, a in R.case_reference(name):
            for s in segs:
                assert all(abs(x) >= R.MIN_SLOPE for x in s.slopes), name     # no grazing roots
    one = R.case_reference("one_crossing")[0]
    assert [len(s.roots) for s in one[0]] == [1] and one[1].n_events == 1
    segs, a = R.case_reference("join_only")[0]
    _, T, _ = R.case_problem("join_only")
    assert [len(s.roots) for s in segs] == [0, 0] and a.n_events == 1 and a.t_event[0] == T[1, 0]
    assert [len(s.roots) for s in R.case_reference("two_crossings")[0][0]] == [2]
    many = R.case_reference("many_crossings")[0]
    assert len(many[0][0].roots) == 5 and many[1].status == 1 and np.sum(np.isfinite(many[1].t_event)) == R.KEEP
    mixed = R.case_reference("mixed66")
    assert [len(s) for s, _ in mixed] == [65, 65, 65]
    assert mixed[0][1].n_events > 4 and mixed[1][1].n_events > 4
    assert any(s.on_e != n.on_s for s, n in zip(mixed[0][0][:-1], mixed[0][0][1:]))      # joins
    assert any(s.roots for s in mixed[0][0]) and any(s.roots for s in mixed[1][0])      # and crossings
    p0 = mixed[2][1]
    assert p0.n_events == 0 and p0.on0 == 1
    # truncation through max_events: the first event only
    segs, full = mixed[0]
    _, T, _ = R.case_problem("mixed66")
    cut = R.compact(segs, T[:, 0], 1)
    assert cut.status == 1 and cut.n_events == full.n_events and cut.t_event[0] == full.t_event[0] and cut.dv == full.dv


def test_rk4_reference_meets_the_adaptive_one(oracle):
    """The RK4 restatement of the device's algorithm finds the adaptive reference's crossing to RK4 x 16's own truncation: the
    state is smooth (h^4 = 8e-9 on the root); the integrand of q is not at this step, 1.5 times the width rho / |dn/dt| of the
    switch, so q is only asked to agree to 1e-4."""
    XC, T, prms = R.case_problem("one_crossing")
    s4 = R.case_reference("one_crossing", rk4_steps=16)[0][0][0]
    s8 = R.case_reference("one_crossing")[0][0][0]
    assert len(s4.roots) == 1 and abs(s4.roots[0] - s8.roots[0]) < 1e-7 and abs(s4.q - s8.q) < 1e-4 * abs(s8.q)


def test_entry_points_validate_shapes():
    prm = lto.make_params(*R.prm_tuple(R.CASES["one_crossing"][0]))
    assert callable(lto.indirect_events) and callable(drivers.thrust_arcs)
    with pytest.raises(ValueError):
        lto.indirect_events(np.zeros(12), np.zeros(2), prm)                      # no node axis
    with pytest.raises(ValueError):
        lto.indirect_events(np.zeros((12, 3)), np.zeros(2), prm)                 # t of another length
    with pytest.raises(ValueError):
        lto.indirect_events(np.zeros((12, 3, 2)), np.zeros((3, 3)), prm)         # grids of another batch
    with pytest.raises(ValueError):
        lto.indirect_events(np.zeros((12, 3, 4)), np.zeros(3), [prm, prm])       # neither one nor B parameter sets
    with pytest.raises(ValueError):
        drivers.thrust_arcs(np.zeros((14, 3)), np.zeros(3), lto.MU, lto.DU, lto.TU, 1000.0, 0.05, 1.0, 1e-2)
    with pytest.raises(ValueError):
        drivers.thrust_arcs(np.zeros((12, 3)), np.zeros(4), lto.MU, lto.DU, lto.TU, 1000.0, 0.05, 1.0, 1e-2)
    from lowthrustopt_amd import _lib
    assert {"lto_indirect_events_batch", "lto_indirect_events", "lto_indirect_events_dev"} <= set(_lib.SIGNATURES)


# ---- segment templates and the patterns of tests/test_thrust_arcs_shapes_gpu.py ----------------------------------------------
MS = (1, 4, 63, 64, 65, 300)


def _arcs(pattern, M=64, t0=0.0):
    XC, t, segs = R.place(pattern, t0)
    return XC, t, segs, R.compact(segs, t, M)


def _joins(segs):
    return [i + 1 for i, (a, b) in enumerate(zip(segs[:-1], segs[1:])) if a.on_e != b.on_s]


def test_template_pools_admit_every_class(oracle):
    from collections import Counter
    for cls, src in R.POOL_SRC.items():
        total = sum(R._spec(name)[b].n - 1 for name, b in src)
        kinds = Counter(R.klass(tid) for tid in R.pool(cls))
        print("pool %s: %d of %d admitted, %s" % (cls, len(R.pool(cls)), total, sorted(kinds.items())))
        assert len(R.pool(cls)) > 0
        if cls != "p0":
            assert {(0, 0, 0), (1, 0, 1), (0, 1, 1), (1, 1, 0)} <= set(kinds), cls      # a join can be forced or excluded anywhere
    kinds = {R.klass(tid) for tid in R.pool("p1")}
    assert any(k[1] == 2 for k in kinds) and R.FIVE in R.pool("p1") and R.klass(R.FIVE)[1] == 5
    assert all(tid[0] == "mixed66" for tid in R.pool("p2")) and all(R.tmpl_node(tid)[2][6] == 2.0 for tid in R.pool("p2"))
    assert all(R.tmpl_node(tid)[2][5:7] == (-1.0, 1.0) for tid in R.pool("p1back"))
    lengths = {R.tmpl_node(tid)[1] for tid in R.pool("p1u")}
    assert len(lengths) == 1
    dropped = [tid for tid in R.PROX if tid not in R.prox_admitted()]
    print("end-proximity templates dropped:", dropped or "none")
    assert len(dropped) <= 1
    base = R.tmpl_node(R.PROX_BASE)[1]
    for tid in R.prox_admitted():                       # the crossing lies delta from the segment's start or end
        (root,), L = R.tmpl_seg(tid).roots, R.tmpl_node(tid)[1]
        gap = root if tid[1] == "start" else L - root
        assert abs(gap - tid[2] * base) <= 1e-9 * base, (tid, gap)


def test_pool_tolerances(oracle):
    e_t, e_dv, e_five = R.pool_tolerances()
    print("pool e_t = %.3e TU (five-crossing template %.3e), e_dv = %.3e (all-off patterns %.3e); existing fixtures %.3e, %.3e"
          % ((e_t, e_five, e_dv["rest"], e_dv["quiet_off"]) + R.tolerances()))
    print("e_dv per family (no bar of its own):", {k: "%.2e" % v for k, v in e_dv["by_family"].items()})
    assert e_t <= 1e-13 and e_five <= 1e-10
    assert e_dv["rest"] <= 1e-7
    assert e_dv["quiet_off"] <= 1e-5        # dv of an all-off trajectory is 1e-7 .. 4e-5: the integrators' absolute 1e-13 weighs more
    assert R.sweep_bars("dense") == R.sweep_bars("cycle_p3") == (max(1e-12, 10 * e_t), max(1e-12, 10 * e_dv["rest"]))
    assert R.sweep_bars("quiet_off")[1] == 10 * e_dv["quiet_off"]


def test_reference_is_autonomous(oracle):
    e_t = R.pool_tolerances()[0]
    worst = 0.0
    for tid in (R.pick("p1", 0, 1), R.pick("p1", None, 2), R.pick("p2", 1, 1)):
        y0, L, prm = R.tmpl_node(tid)
        s0 = R.tmpl_seg(tid)
        for ti in (0.0, 1.7, 12.3):
            s = R.seg_reference(oracle, y0, ti, ti + L, prm)
            assert (s.on_s, len(s.roots), s.on_e) == R.klass(tid)
            d = float(np.max(np.abs(np.array(s.roots) - (ti + np.array(s0.roots)))))
            worst = max(worst, d)
            assert d <= e_t + 4 * R.EPS * abs(ti + L), (tid, ti, d)
            assert abs(s.q - s0.q) <= 1e-11 * abs(s0.q)          # the segment's end moves by the rounding of ti + L only
    print("autonomy: largest |root(t_i) - (t_i + tau)| = %.3e TU" % worst)


def test_patterns_realise_their_features(oracle):
    P = R.sweep_patterns()
    for n in R.NSEGS:
        for on in (1, 0):
            _, t, segs, a = _arcs(P["quiet_%s%d" % ("on" if on else "off", n)][2])
            assert len(segs) == n and a.n_events == 0 and a.on0 == on and a.status == 0 and np.all(np.isnan(a.t_event))
            assert abs(a.burn_time - (t[-1] - t[0])) <= 1e-13 * (t[-1] - t[0]) if on else a.burn_time == 0.0
        _, t, segs, a = _arcs(P["edges%d" % n][2])
        want = sorted({0, 63, 64, n - 1} & set(range(n)))
        assert R.event_owner(segs) == want and not _joins(segs) and [len(s.roots) for s in segs] == [int(i in want) for i in range(n)]
    for n in (65, 128, 129):
        _, t, segs, a = _arcs(P["joins%d" % n][2])
        want = [64, 128] if n == 129 else [64]
        assert _joins(segs) == want and not any(s.roots for s in segs) and list(a.t_event[:len(want)]) == [t[i] for i in want]
        assert a.n_events == len(want)
    for n in (65, 129):
        _, t, segs, a = _arcs(P["dense%d" % n][2], 300)
        K = a.n_events
        print("dense%d: K = %d events, %d joins" % (n, K, len(_joins(segs))))
        assert all(len(s.roots) in (1, 2) for s in segs) and n - 1 < K < 299 and a.status == 0
        assert any(len(s.roots) == 2 for s in segs) and _joins(segs)
        own = R.event_owner(segs)
        assert own[63] < 64 <= own[64] or own[63] == own[64]       # list position 64 is reached inside the second chunk or on its edge
    for at in R.HOLES:
        _, t, segs, a = _arcs(P["holes" + "_".join(map(str, at))][2], 300)
        own = R.event_owner(segs)
        first = own.index(at[0])
        listed = int(np.sum(np.isfinite(a.t_event)))
        assert [i for i, s in enumerate(segs) if len(s.roots) > R.KEEP] == list(at)
        assert listed == first + R.KEEP and a.status == 1 and a.n_events == len(own) > listed + 1
        assert (first > 0) == (at[0] > 0) and own[-1] > at[-1]      # ordinary events ahead of it (but at index 0) and behind it
        if at[0] > 0:
            assert first >= 2                                       # room for a max_events below the hole
    for cls in R.CLASSES:
        _, t, segs, a = _arcs(P["cycle_" + cls][2], 128, 1.7)
        print("cycle_%s: %d events, %d joins" % (cls, a.n_events, len(_joins(segs))))
        if cls == "p0":
            assert a.n_events == 0 and a.on0 == 1
        else:
            assert a.status == 0 and any(s.roots for s in segs) and _joins(segs) and a.n_events > 4
    for tid in R.prox_admitted():
        for n in (1, 65):
            _, t, segs, a = _arcs(P["prox_%s_%g_%d" % (tid[1], tid[2], n)][2])
            assert a.n_events == 1 and R.event_owner(segs) == [n - 1]
    counts = [_arcs(p)[3] for p in R.pat_plumbing()]
    assert len({a.n_events for a in counts}) >= 5 and [a.status for a in counts] == [1, 0, 0, 0, 1, 0]
    assert counts[0].n_events > 64 and R.FIVE in R.pat_plumbing()[4]
    shared = [R.place(p) for p in R.pat_shared_grid()]
    assert all(np.array_equal(s[1], shared[0][1]) for s in shared)
    assert len({tuple(p) for p in R.pat_shared_grid()}) == 6 and len({R.compact(s[2], s[1]).n_events for s in shared}) >= 3


def test_compact_against_a_direct_restatement(oracle):
    n_checked = 0
    for name, (_, _, pat) in R.sweep_patterns().items():
        _, t, segs = R.place(pat)
        for M in MS + (len(R.event_owner(segs)),):
            if M < 1:
                continue
            a = R.compact(segs, t, M)
            n, evs, status = R.compact_direct(segs, t, M)
            assert (a.n_events, a.status) == (n, status), (name, M)
            assert list(a.t_event[:len(evs)]) == [e[0] for e in evs] and list(a.kind[:len(evs)]) == [e[1] for e in evs], (name, M)
            assert np.all(np.isnan(a.t_event[len(evs):])) and np.all(a.kind[len(evs):] == 0), (name, M)
            n_checked += 1
    assert n_checked > 300


def test_rk4_patterns(oracle):
    two = [R.pick("p1", None, 2)]
    counts = {}
    for steps in (1, 2, 16, 64):
        _, t, segs = R.place(two, rk4_steps=steps)
        counts[steps] = len(segs[0].roots)
    print("RK4 on the two-crossing template, events per step count:", counts)
    assert counts[1] == 0 and counts[16] == 2 and counts[64] == 2      # one step sees equal on-states at its ends
    _, t, segs = R.place(R.pat_dense(65), rk4_steps=16)
    a = R.compact(segs, t, 300)
    assert a.n_events > 64 and a.status == 0
