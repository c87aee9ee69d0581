"""CPU checks for the periodic-orbit generator: the independent reference (tests/halo_reference.py) against the
packaged tables and against itself at looser tolerances -- its own spread has to stay below a tenth of every bound the GPU tests
(tests/test_halo_gpu.py) hold the device to, or those bounds would mean nothing -- the pure-numpy seed helpers of the drivers, and
the argument checks the Python layer makes before any library call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import halo_reference as HR  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU  # noqa: E402

# the bounds of tests/test_halo_gpu.py
GPU_STATE, GPU_M_REL, GPU_NU, GPU_UNKNOWN = 1e-10, 1e-9, 1e-7, 1e-11


@pytest.fixture(scope="module")
def packaged():
    return [np.asarray(tb[:6], dtype=float) for tb in synth.halo_orbits()]


_CACHE = {}


def _corrected(packaged, k, mode, rtol=HR.RTOL):
    key = (k, mode, rtol)
    if key not in _CACHE:
        _CACHE[key] = HR.correct(HR.seed_of(packaged[k]), mode, MU, rtol=rtol, atol=rtol / 10.0)
    return _CACHE[key]


def _table(packaged, k, rtol=HR.RTOL):
    key = ("table", k, rtol)
    if key not in _CACHE:
        c = _corrected(packaged, k, HR.HOLD_X0)
        _CACHE[key] = HR.table(c.state, c.period, 100, MU, rtol=rtol, atol=rtol / 10.0)
    return _CACHE[key]


@pytest.mark.parametrize("k", [0, 1])
@pytest.mark.parametrize("mode", [HR.HOLD_X0, HR.HOLD_Z0])
def test_reference_converges_from_the_packaged_seeds(packaged, k, mode):
    c = _corrected(packaged, k, mode)
    print("orbit %d mode %d: %d steps, history %s, P = %.12f" % (k + 1, mode, c.iterations, c.history, c.period))
    assert c.status == 0 and c.iterations <= 3
    if mode == HR.HOLD_X0:
        assert abs(c.period - (2.908313312205, 3.129634690082)[k]) < 1e-10


@pytest.mark.parametrize("k", [0, 1])
def test_reference_table_matches_the_packaged_table(packaged, k):
    X, _ = _table(packaged, k)
    err = np.abs(X - packaged[k]).max()
    print("orbit %d: 100 samples against the packaged table, max-abs %.3e" % (k + 1, err))
    assert err < 1e-7


def test_reference_march_in_x0_reaches_orbit_2(packaged):
    c1 = _corrected(packaged, 0, HR.HOLD_X0)
    values = np.linspace(packaged[0][0, 0], packaged[1][0, 0], 9)[1:]
    members = HR.family(c1.state, values, "x0", MU)
    print("march: steps per member %s" % [m.iterations for m in members])
    assert all(m.status == 0 for m in members)
    last = members[-1].state
    assert np.abs(last - HR.seed_of(packaged[1])).max() < 1e-7
    assert abs(HR.jacobi(last, MU) - 3.06) < 1e-7


@pytest.mark.parametrize("k", [0, 1])
def test_trace_formula_equals_the_eigenvalue_indices(packaged, k):
    _, M = _table(packaged, k)
    a, b = HR.nu_from_traces(M), HR.nu_from_eigenvalues(M)
    print("orbit %d: nu (traces) %s, (eigenvalues) %s" % (k + 1, a, b))
    assert np.abs(a - b).max() < 1e-8
    if k == 0:
        assert np.abs(a - np.array([-0.901722, 22.590284])).max() < 1e-5


@pytest.mark.parametrize("k", [0, 1])
def test_reference_spread_is_a_tenth_of_the_gpu_bounds(packaged, k):
    """The same corrected orbit integrated at rtol 1e-11 instead of 1e-13, and the corrector run at 1e-11."""
    X, M = _table(packaged, k)
    Xl, Ml = _table(packaged, k, rtol=1e-11)
    e_state = np.abs(X - Xl).max()
    e_M = np.abs(M - Ml).max() / np.abs(M).max()
    e_nu = np.abs(HR.nu_from_traces(M) - HR.nu_from_traces(Ml)).max()
    c, cl = _corrected(packaged, k, HR.HOLD_X0), _corrected(packaged, k, HR.HOLD_X0, rtol=1e-11)
    e_unk = max(np.abs(c.state - cl.state).max(), abs(c.period - cl.period))
    print("orbit %d spread 1e-11 vs 1e-13: samples %.2e, M rel %.2e, nu %.2e, unknowns and P %.2e" % (k + 1, e_state, e_M, e_nu, e_unk))
    assert e_state < 0.1 * GPU_STATE
    assert e_M < 0.1 * GPU_M_REL
    assert e_nu < 0.1 * GPU_NU
    assert e_unk < 0.1 * GPU_UNKNOWN


@pytest.mark.parametrize("hold,mode", [("x0", HR.HOLD_X0), ("z0", HR.HOLD_Z0)])
def test_gpu_seeds_converge_under_the_reference(packaged, hold, mode):
    seeds = HR.gpu_seeds([HR.seed_of(p) for p in packaged], hold)
    assert seeds.shape == (6, 17)
    base = seeds[:, :2]
    steps = []
    for k in range(17):
        nearest = np.abs(seeds[:, [k]] - base).max(axis=0).argmin()
        d = seeds[:, k] - base[:, nearest]
        assert np.abs(d[[0, 2]]).max() <= 1e-4 and abs(d[4]) <= 1e-3
        c = HR.correct(seeds[:, k], mode, MU)
        steps.append(c.iterations)
        assert c.status == 0 and c.iterations <= 4
    print("hold %s: steps %s" % (hold, steps))


def test_libration_points():
    assert abs(drivers.libration_point(1, MU) - 0.8369151258) < 1e-9
    assert abs(drivers.libration_point("L2", MU) - 1.1556821654) < 1e-9
    with pytest.raises(ValueError):
        drivers.libration_point(3, MU)


@pytest.mark.parametrize("which,p_lin", [(1, 2.69158), (2, 3.37326)])
def test_lyapunov_seed_converges_under_the_reference(which, p_lin):
    seed, period = drivers.lyapunov_seed(which, 1e-3, MU)
    assert abs(period - p_lin) < 1e-5
    assert seed[1] == seed[2] == seed[3] == seed[5] == 0.0
    c = HR.correct(seed, HR.PLANAR, MU)
    print("L%d: %d steps, P = %.8f (linear %.8f)" % (which, c.iterations, c.period, period))
    assert c.status == 0 and c.iterations <= 4
    assert abs(c.period - period) < 1e-3


@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("Ax", HR.PLANAR_AX)
def test_planar_gpu_seeds_are_well_conditioned_in_the_reference(which, Ax):
    """The Lyapunov seeds of the GPU tests: the reference converges, and its own spread (rtol 1e-12 against 1e-13) in the unknown and
    the period stays below a tenth of the 1e-11 the device is held to."""
    seed, _ = drivers.lyapunov_seed(which, Ax, MU)
    c = HR.correct(seed, HR.PLANAR, MU)
    cl = HR.correct(seed, HR.PLANAR, MU, rtol=1e-12, atol=1e-13)
    e = max(abs(c.state[4] - cl.state[4]), abs(c.period - cl.period))
    print("L%d Ax = %g: %d steps, spread %.2e" % (which, Ax, c.iterations, e))
    assert c.status == 0 and cl.status == 0 and c.iterations <= 8
    assert e < 0.1 * GPU_UNKNOWN


def test_halo_correct_rejects_malformed_input_before_any_library_call(monkeypatch):
    def no_context():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(lto.hotpath, "default_context", no_context)
    for bad in (np.zeros(5), np.zeros((5, 3)), np.zeros((6, 2, 2)), np.zeros((6, 0)), 1.0):
        with pytest.raises(ValueError):
            lto.halo_correct(bad, "x0")
    with pytest.raises(ValueError):
        lto.halo_correct(np.zeros(6), "y0")
    with pytest.raises(ValueError):
        lto.halo_correct(np.zeros(6), 7)
    with pytest.raises(ValueError):
        lto.halo_correct(np.zeros(6), "x0", max_iter=-1)
    with pytest.raises(ValueError):
        lto.halo_table(np.zeros((6, 2)), 1.0, 1)
    with pytest.raises(ValueError):
        lto.halo_table(np.zeros(7), 1.0, 10)
    with pytest.raises(ValueError):
        drivers.halo_family(np.zeros(6), [1.0], hold="y0")
    with pytest.raises(ValueError):
        drivers.halo_family_fill(np.zeros((6, 1)), 3)
