"""The variable-mass thrust-arc reference (tests/thrust_mass_reference.py) against itself, the Python layers of
hotpath.indirect_events_mass / drivers.thrust_arcs_mass without a device, and the ABI table."""
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
