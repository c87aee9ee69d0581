"""CPU checks of tests/dense_reference.py, the reference of the dense-output and addTimeFinal shape sweeps: the long-double spline
against two independent statements, the sample assignment on every grid of the sweep, the bars of the sweep kept by the oracle
against itself, and the properties the add-time cases rely on (the coast of the snap cases, both sides of the cost's clamp)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import addtime_reference as R  # noqa: E402
import dense_reference as D  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402


def _rel_rows(a, b):
    return float((np.abs(a - b) / np.maximum(np.abs(b).max(axis=1, keepdims=True), 1e-300)).max())


def _knots(kind, m, rng):
    if kind == "uniform":
        return R.linrange(0.3, 2.1, m)
    return 0.3 + np.concatenate([[0.0], np.cumsum(rng.uniform(0.02, 0.3, m - 1))])


@pytest.mark.parametrize("kind", ["uniform", "nonuniform"])
@pytest.mark.parametrize("m", [3, 4, 5, 17, 64, 257])
def test_spline_three_statements_agree(kind, m):
    from scipy.interpolate import CubicSpline
    rng = np.random.default_rng(100 + m)
    x = _knots(kind, m, rng)
    Y = np.vstack([np.sin(3.0 * x) + 0.2 * x, np.cos(2.0 * x) * x, rng.standard_normal(m)])
    xq = np.sort(np.concatenate([rng.uniform(x[0], x[-1], 40), x[[0, m // 2, -1]], 0.5 * (x[:-1] + x[1:])]))
    got = D.natural_spline_ld(x, Y, xq)
    a = R.natural_spline(x, Y, xq)
    b = CubicSpline(x, Y, axis=1, bc_type="natural")(xq)
    assert _rel_rows(got, a) <= 1e-12 and _rel_rows(got, b) <= 1e-12
    knots = np.isin(xq, x)
    assert knots.sum() >= 3 and np.array_equal(got[:, knots], Y[:, np.searchsorted(x, xq[knots])])   # at a knot the sample itself


def test_spline_two_knots_is_the_chord():
    got = D.natural_spline_ld([1.0, 3.0], [[2.0, 6.0]], [1.0, 1.5, 2.0, 3.0])
    assert np.array_equal(got, [[2.0, 3.0, 4.0, 6.0]])


def _library_ranges(g, td, closing):
    """segment_samples of lto_host_sweeps.hip, loop for loop."""
    first, j = [], 0
    for i in range(len(g) - 1):
        first.append(j)
        while j < len(td) - 1 and td[j] < g[i + 1]:
            j += 1
    return np.array(first + [closing])


@pytest.mark.parametrize("case", D.CASES, ids=[c.name for c in D.CASES])
def test_segment_ranges_on_the_sweeps_grids(case):
    XC, t, _ = D.case_problem(case)
    m, S = case.n_desired, case.n - 1
    td, first = D.case_samples(case, t)
    assert first.size == S + 1 and first[0] == 0 and first[S] == m - 1 and np.all(np.diff(first) >= 0)
    assert np.array_equal(first, _library_ranges(t, td, m - 1))
    assert np.array_equal(D.segment_ranges(t, td, True), _library_ranges(t, td, m))
    for i in range(S):                                   # every sample once, in the segment that holds it
        for j in range(first[i], first[i + 1]):
            assert t[i] <= td[j] < t[i + 1]
    empty = int(np.count_nonzero(np.diff(first) == 0))
    if (case.n, m) == (13, 5):
        assert empty == 8 and np.all(np.diff(first) <= 1)
    if (case.n, m) == (66, 7):
        assert empty == 59
    if case.lin:
        assert np.array_equal(td, t) and np.array_equal(first, np.arange(13))     # every sample is a node, bit for bit
    if m >= 2 * case.n:
        assert empty == 0


@pytest.mark.parametrize("B,n_tgrids", [(3, 1), (3, 3), (5, 1), (5, 5)])
def test_batch_ranges(B, n_tgrids):
    XC, T, prm_l, tds, first, off = D.batch_problem(B, n_tgrids)
    S = D.BATCH_N - 1
    assert first.size == B * S + 1 and np.all(np.diff(first) >= 0) and first[-1] == sum(D.BATCH_COUNTS[:B])
    assert first[S] == first[S + 1]                      # trajectory 1: nothing in its first segment
    for b in range(B):
        t = T[:, b if n_tgrids > 1 else 0]
        assert first[b * S] == off[b] and first[(b + 1) * S] == off[b + 1]
        for i in range(S):
            for j in range(first[b * S + i] - off[b], first[b * S + i + 1] - off[b]):
                assert t[i] <= tds[b][j] and (tds[b][j] < t[i + 1] or (i == S - 1 and tds[b][j] == t[-1]))
    if n_tgrids > 1:
        assert not np.array_equal(T[:, 0], T[:, 1])


def _self_consistency(oracle, XC, t, prm_l, td, first, mname, base=0):
    """The oracle chained hop by hop against the oracle from the node, samples and final state."""
    method, steps = D.METHODS[mname]
    node_ref, hop_ref = D.dense_expected(oracle, XC, t, prm_l, td, first, method, steps, base=base)
    en, _ = D.worst_errors(hop_ref, node_ref, hop_ref, range(first[0] - base, first[-1] - base))
    fn, fh = D.final_expected(oracle, XC, t, prm_l, td, first, method, steps, base=base)
    return max(en, D.rel(fh, fn))


@pytest.mark.parametrize("mname", D.FROM_NODE)
def test_the_reference_keeps_the_bars_against_itself(oracle, mname):
    """The from-the-node expectation is reproduced by chaining the oracle hop by hop, on every case of the sweep, with a decade to
    spare under the bar the device is held to: the bars are ones the reference itself keeps."""
    worst = 0.0
    for case in D.CASES:
        XC, t, prm_l = D.case_problem(case)
        td, first = D.case_samples(case, t)
        worst = max(worst, _self_consistency(oracle, XC, t, prm_l, td, first, mname))
    for B, g in [(3, 1), (3, 3), (5, 1), (5, 5)]:
        XC, T, prm_l, tds, first, off = D.batch_problem(B, g)
        S = D.BATCH_N - 1
        for b in range(B):
            worst = max(worst, _self_consistency(oracle, XC[:, :, b], T[:, b if g > 1 else 0], prm_l[b], tds[b],
                                                 first[b * S:(b + 1) * S + 1], mname, base=off[b]))
    print("%s: the oracle chained against the oracle from the node, worst %.2e (bar %.0e)" % (mname, worst, D.TOL[mname]))
    assert worst <= 0.1 * D.TOL[mname]


def test_case_table_covers_the_parameters():
    assert {(c.n, c.n_desired) for c in D.CASES} == set(D.SHAPES)
    assert {(c.p, c.thrust, c.time_dir) for c in D.CASES} == {(p, th, d) for p in D.PS for th in D.THRUSTS for d in D.DIRS}
    assert all(c.rho >= 0.1 for c in D.CASES) and min(D.BATCH_RHO) >= 0.1
    assert sorted({c.n - 1 for c in D.CASES if c.n >= 64}) == [63, 64, 65, 129]


def test_snap_cases_coast_far_less_than_the_candidate_spacing(oracle):
    times, tab = D.arrival_table()
    S = R.natural_spline(times, tab, np.arange(1001) / 1000.0)
    spacing = np.sqrt(np.sum(np.diff(S, axis=1) ** 2, axis=0)).min()
    prm_l = [MU, DU, TU, 10.0, D.MASS, 1.0, 2.0, 1.0]
    for j in D.SNAP_J:
        y0 = np.concatenate([S[:, j], np.zeros(6)])
        y, rc, _, _ = oracle.flow_state_costate(y0, prm_l, D.SNAP_DT, oracle.DOP853_ADAPTIVE)
        assert rc == 0 and np.all(y[6:] == 0.0)
        assert np.abs(y[:6] - y0[:6]).max() <= 1e-5 * spacing, (j, spacing)
    # the table is closed to 1.6e-9 only (its last column is a propagated state): candidates 0 and 1000 do not tie, and a coast of
    # 1e-11 leaves each its own winner
    gap = np.abs(S[:, 0] - S[:, 1000]).max()
    assert 1e-9 < gap < 1e-8
    assert R.find_tau_from_samples(S, S[:, 1000])[0] == 1000 and R.find_tau_from_samples(S, S[:, 0])[0] == 0


@pytest.mark.parametrize("p,rho,thrust,lam_sigma,seed", [c for c in D.COST_CASES if c[0] > 1.0])
@pytest.mark.parametrize("m", D.COST_M)
def test_cost_cases_sit_on_both_sides_of_the_clamp(oracle, p, rho, thrust, lam_sigma, seed, m):
    """The guess addTimeFinal builds, restated with the oracle alone, densified on its own grid: the p > 1 magnitude is clamped at
    aL at some sample and below it at another, for every flight-time change of the cost cases."""
    XC, t = D.addtime_problem(D.COST_N, seed=seed, lam_sigma=lam_sigma)
    prm_l = [MU, DU, TU, thrust, D.MASS, 1.0, p, rho]
    aL = D.thrust_accel(thrust)
    for dt in D.add_time_dts(D.COST_K):
        G, t_new, _ = D.addtime_guess_host(oracle, XC, t, prm_l, dt, m)
        td = R.linrange(t_new[0], t_new[-1], m)
        _, u = D.dense_cost_ld(D.oracle_dense(oracle, G, t_new, prm_l, td), td, thrust, p, rho, D.MASS, DU, TU)
        hi, lo = D.clamp_sides(u, aL)
        assert hi >= 1 and lo >= 1, (p, m, dt, u / aL)
