"""Thrust arcs, host side: the reference of tests/thrust_reference.py against itself, the conditions its fixtures
have to meet, and the shape validation of the Python entry points -- no GPU.

Measured here: e_t = 4.1e-15 TU (two CPU determinations of the fixture roots), e_dv = 5.5e-9 (reference dv at 1e-13 against 1e-12)."""
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
