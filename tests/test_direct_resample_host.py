"""CPU checks of the direct method's resampling (lto_direct_resample_batch) on its host restatement
(tests/resample_reference.py) and the CPU oracle: the exponent of the monitor, equidistribution on one thrust arc, the branches of
the node rule, and the interface tables.  tests/test_cabi_symbols.py checks the symbols themselves."""
import os
import re
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import remesh_reference as R  # noqa: E402
import resample_reference as RS  # noqa: E402
from lowthrustopt_amd import _lib, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRM = (MU, DU, TU, 2000.0)
EPS = np.finfo(np.float64).eps


def arc(oracle, x0, u, t):
    """Nodes on ONE thrust arc: constant control u, X[:, k] = the oracle's flow of x0 to t[k] (DOP853 at 1e-13 from node to node)."""
    X = np.zeros((len(x0), t.size), order="F")
    X[:, 0] = x0
    for k in range(1, t.size):
        X[:, k], _ = oracle.flow_prop_ep(X[:, k - 1], u, 1.0, t[k] - t[k - 1], oracle.DOP853_ADAPTIVE, 0, *PRM)
    return X, np.asfortranarray(np.repeat(np.asarray(u, dtype=np.float64)[:, None], t.size, axis=1))


def test_estimate_scales_with_the_eighth_power(oracle):
    """e ~ C h^8: the estimate of a segment against the larger estimate of its two halves, on halo-seeded segments of one arc
    with 0.05 N-scale controls, one RKF7(8) step per half-arc (nsteps = 2).  Seeds whose estimate is at least 1e3 times the
    rounding floor of h 41/840 (F psi) -- four slopes of size |f| at one ulp each -- are decisive.

    h = 0.2 TU, about a segment of the demo's 30-node mesh: every decisive seed is asserted.  Measured ratios, seeds 0 .. 11
    (2^8 = 256): 280 197 188 232 250 255 245 225 225 247 248 192, every estimate between 4.0e-13 and 2.8e-8 against floors of 5e-18.

    h = 0.1 and 0.4 TU: e ~ C h^8 supposes one C for the segment, and the two halves measure it: their estimates are C_1 (h/2)^8
    and C_2 (h/2)^8.  Where they agree within the factor 2 that the check allows, the seed is asserted; the others are printed.
    THE FACTOR 2 FAILS on seeds 1 and 11, the closest lunar pass of the set (0.079 DU from the Moon): 117 and 118 at 0.1 TU, 746 and
    759 at 0.4 TU; their halves differ by 3.3 (0.1 TU) and 23 (0.4 TU).  All other decisive seeds lie within 132 .. 286 at both
    spans, asserted or not.  DESIGN 4.17 has the table; the exponent of the specification stays 8,
    the order the estimates approach as h falls wherever C is settled over the segment."""
    for h in (0.2, 0.1, 0.4):
        rng = np.random.default_rng(17)
        asserted, outside = [], []
        for seed in range(12):
            Xs, _, _ = synth.direct_problem(12, seed=seed, dt_seg=0.4)
            x0 = Xs[:, 1 + seed % 10, 0].copy()
            u = 0.05 / np.sqrt(3.0) * rng.standard_normal(3)
            X, U = arc(oracle, x0, u, np.array([0.0, h / 2, h]))
            e_full = oracle.direct_defect(X[:, [0, 2]], U[:, [0, 2]], np.array([0.0, h]), 2, *PRM)[1][0]
            halves = oracle.direct_defect(X, U, np.array([0.0, h / 2, h]), 2, *PRM)[1]
            f = np.abs(oracle.flow_prop_ep(x0, u, 1.0, 1e-6, oracle.RKF78_FIXED, 1, *PRM)[0] - x0).max() / 1e-6
            floor = (h / 2) * 41.0 / 840.0 * 4.0 * EPS * max(f, np.abs(x0).max())
            ratio, spread = e_full / halves.max(), halves.max() / halves.min()
            decisive = e_full >= 1e3 * floor
            used = decisive and (h == 0.2 or spread <= 2.0)
            print("h %.1f seed %2d: e(h) = %.3e, max e(h/2) = %.3e, ratio %7.1f, halves differ by %5.2f, floor %.1e%s" % (
                h, seed, e_full, halves.max(), ratio, spread, floor,
                "" if used else "  (below 1e3 floors: not used)" if not decisive else "  (C not settled over the segment: not asserted)"))
            if used:
                asserted.append(ratio)
            elif decisive and not 128.0 <= ratio <= 512.0:
                outside.append((seed, round(ratio)))
        print("h %.1f: %d seeds asserted; decisive seeds outside the factor 2, not asserted: %s" % (h, len(asserted), outside))
        assert len(asserted) >= (6 if h == 0.2 else 3)
        assert all(128.0 <= r <= 512.0 for r in asserted), (h, asserted)


def test_points_of_one_arc_stay_on_it_and_share_the_monitor(oracle):
    """Constant control, nodes = the oracle's flow: resampling with caller weights returns points of the same arc, and every new
    segment carries the same share of the monitor."""
    x0 = synth.direct_problem(12, seed=3, dt_seg=0.4)[0][:, 2, 0].copy()
    u = np.array([0.02, -0.03, 0.015])
    t = np.concatenate(([0.0], np.cumsum(np.where(np.arange(9) % 2 == 0, 0.25, 0.06))))
    X, U = arc(oracle, x0, u, t)
    w = np.random.default_rng(5).uniform(0.3, 4.0, t.size - 1)
    for n_new in (7, 10, 23):
        Xn, Un, tn, status = RS.resample(oracle, X, U, t, 10, PRM, n_new, weights=w)
        assert status == 0 and tn[0] == t[0] and tn[-1] == t[-1] and np.all(np.diff(tn) > 0)
        want, _ = arc(oracle, x0, u, tn)
        err = np.abs(Xn - want).max()
        share = R.monitor_share(t, w, tn)
        dev = np.abs(share - w.sum() / (n_new - 1)).max() / w.sum()
        print("n_new = %d: max |X - arc| = %.2e, monitor share off by %.2e of the total" % (n_new, err, dev))
        assert err <= 1e-12
        assert dev <= 1e-12
        assert np.array_equal(Un, np.repeat(u[:, None], n_new, axis=1))       # u + s (u - u)


def test_branches_of_the_node_rule(oracle):
    t = np.array([0.0, 0.3, 0.4, 1.0])
    assert RS.node_rule(t, 0.3, False) == ("copy", 1)                         # coincidence with an old node
    assert RS.node_rule(t, 1.0, True) == ("copy", 3) and RS.node_rule(t, 1.0, False) == ("copy", 3)   # the last node, never a propagation
    tm = 0.4 + (1.0 - 0.4) / 2
    kind, i, span, s = RS.node_rule(t, tm, False)                             # the mid-point: forward, the sweep's own half span
    assert (kind, i) == ("forward", 2) and span == 0.5 * (1.0 - 0.4)
    kind, i, span, s = RS.node_rule(t, np.nextafter(tm, 2.0), False)          # just past it: backward from node 3
    assert (kind, i) == ("backward", 2) and span == 1.0 - np.nextafter(tm, 2.0)
    kind, i, span, s = RS.node_rule(t, 0.1, False)
    assert (kind, i, span) == ("forward", 0, 0.1) and s == 0.1 / 0.3
    # n = 2: uniform weights, three new nodes -> the ends are copies, the middle node is lto_direct_midpoints' forward half-arc
    x0 = synth.direct_problem(12, seed=3, dt_seg=0.4)[0][:, 4, 0].copy()
    X, U = arc(oracle, x0, np.array([0.01, 0.02, -0.03]), np.array([0.0, 0.4]))
    U[:, 1] = [0.03, -0.01, 0.02]
    Xn, Un, tn, status = RS.resample(oracle, X, U, np.array([0.0, 0.4]), 10, PRM, 3, weights=np.ones(1))
    assert status == 0 and np.array_equal(tn, [0.0, 0.2, 0.4])
    assert np.array_equal(Xn[:, [0, 2]], X) and np.array_equal(Un[:, [0, 2]], U)
    mid, _ = oracle.flow_prop_ep(X[:, 0], U[:, 0], 1.0, 0.2, oracle.RKF78_FIXED, 9, *PRM)
    assert np.array_equal(Xn[:, 1], mid)
    um = (U[:, 0] + U[:, 1]) / 2                                              # direct.jl:659, to rounding
    assert np.all(np.abs(Un[:, 1] - um) <= 1e-15 * np.abs(um))
    # the backward arc lands on the same trajectory as the forward one (a consistent segment): one node either side of the middle
    X, U = arc(oracle, x0, np.array([0.01, 0.02, -0.03]), np.array([0.0, 0.4]))
    Xn, _, tn, _ = RS.resample(oracle, X, U, np.array([0.0, 0.4]), 10, PRM, 5, weights=np.ones(1))
    want, _ = arc(oracle, x0, np.array([0.01, 0.02, -0.03]), tn)
    assert RS.node_rule(np.array([0.0, 0.4]), tn[3], False)[0] == "backward"
    assert np.abs(Xn - want).max() <= 1e-12
    # estimates as the monitor, two passes, and a NaN estimate
    Xs, Us, Ts = synth.direct_problem(8, seed=3, dt_seg=0.4)
    Xn, Un, tn, status = RS.resample(oracle, Xs[:, :, 0], Us[:, :, 0], Ts[:, 0], 10, PRM, 8, passes=2)
    assert status == 0 and np.all(np.diff(tn) > 0) and np.isfinite(Xn).all()
    assert RS.weights_from_estimates(np.array([1e-12, np.nan]), 0.1) is None
    assert np.array_equal(RS.weights_from_estimates(np.zeros(3), 0.1), np.ones(3))
    assert np.array_equal(RS.weights_from_estimates(np.array([1.0, 1e-16]), 0.1), [1.0, 0.1])


def test_interface_tables():
    header = open(os.path.join(ROOT, "include", "lto.h")).read()
    julia = open(os.path.join(ROOT, "julia", "LowThrustOptHIP.jl")).read()
    for name in ("lto_direct_resample_batch", "lto_direct_resample"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES
    assert "(:lto_direct_resample_batch, liblto)" in julia and re.search(r"^export[^#]*\bdirect_resample\b", julia, re.S | re.M)
    assert len(_lib.SIGNATURES["lto_direct_resample_batch"][1]) == 20 and len(_lib.SIGNATURES["lto_direct_resample"][1]) == 18


def test_the_restatement_never_loads_the_device_library():
    text = open(os.path.join(ROOT, "tests", "resample_reference.py")).read()
    assert not re.search(r"^\s*(import|from)\s+lowthrustopt_amd", text, flags=re.M)
