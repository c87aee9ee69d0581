"""CPU checks of the host restatement of addTimeFinal's re-mesh and find_tau (tests/addtime_reference.py), which the GPU tests
of lto_indirect_add_time_batch compare against."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import addtime_reference as R  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402


def test_spline_equals_scipy_and_the_drivers_spline():
    interpolate = pytest.importorskip("scipy.interpolate")
    rng = np.random.default_rng(3)
    x = R.linrange(0.3, 3.7, 57)
    Y = np.vstack([np.sin(2.0 * x), np.exp(-x) * np.cos(5.0 * x), rng.standard_normal(x.size)])
    xq = np.sort(np.concatenate([rng.uniform(x[0], x[-1], 40), x[[0, 7, 56]]]))
    got = R.natural_spline(x, Y, xq)
    want = interpolate.CubicSpline(x, Y, axis=1, bc_type="natural")(xq)
    scale = np.abs(Y).max(axis=1, keepdims=True)
    assert np.abs(got - want).max() / scale.max() < 1e-14
    for k, q in enumerate(xq):
        assert np.abs(got[:, k] - drivers._natural_spline(x, Y, q)).max() / scale.max() < 1e-14


def test_spline_reproduces_linear_data():
    x = R.linrange(-1.0, 2.0, 31)
    Y = np.vstack([3.0 * x - 0.5, -0.25 * x + 7.0])
    xq = R.linrange(-1.0, 2.0, 17)
    got = R.natural_spline(x, Y, xq)
    np.testing.assert_allclose(got, np.vstack([3.0 * xq - 0.5, -0.25 * xq + 7.0]), rtol=0, atol=1e-14)


def test_remesh_keeps_both_ends_bit_for_bit():
    t = R.linrange(0.1, 2.9, 200)
    Y = np.vstack([np.cos(t + k) for k in range(12)])
    XC_new, t_new = R.remesh(Y, t, 30)
    assert t_new[0] == t[0] and t_new[-1] == t[-1]
    assert np.array_equal(XC_new[:, 0], Y[:, 0]) and np.array_equal(XC_new[:, -1], Y[:, -1])


@pytest.mark.parametrize("j", [0, 137, 500, 999, 1000])
def test_find_tau_at_a_table_knot(j):
    """A state taken at a candidate τ_j = j / 1000 is found at that τ_j (the halo table's times are LinRange(0, 1, 100))."""
    tab = synth.halo_orbits()[1]
    times = np.linspace(0.0, 1.0, tab.shape[1])
    x = R.natural_spline(times, tab[:6], [j / 1000.0])[:, 0]
    tau, s = R.find_tau(times, tab, x)
    assert tau == j / 1000.0
    assert np.array_equal(s, x)


def test_find_tau_takes_the_first_of_equal_distances():
    S = np.zeros((6, 1001))
    S[0] = np.abs(np.arange(1001) - 500.0)      # d_j = |S[0, j] - 3|: j = 497 and 503 both at distance 0
    j, d = R.find_tau_from_samples(S, np.array([3.0, 0, 0, 0, 0, 0]))
    assert j == 497 and d[503] == d[497] == 0.0


def test_extended_trajectory_leaves_the_callers_array_alone():
    XC = np.arange(12 * 5, dtype=np.float64).reshape(12, 5)
    before = XC.copy()
    XCe, te = R.extended(XC, np.arange(5.0), 0.5)
    assert np.array_equal(XC, before)
    assert XCe.shape == (12, 6) and te[-1] == 4.5
    assert np.all(XCe[6:, 4] == 0.0) and np.array_equal(XCe[:6, 4], XC[:6, 4])
