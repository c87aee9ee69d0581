"""CPU checks for the targeted periodic-orbit corrector: the independent reference (tests/halo_target_reference.py)
converges on every input the GPU tests use (tests/test_halo_target_gpu.py) and its own spread between (1e-13, 1e-14) and
(1e-11, 1e-12) stays below a tenth of every bound the device is held to; its two q rows agree with difference quotients; the inputs
of the singular-step test are what that test takes them for; the pure-numpy parts of the new drivers; and the argument checks the
Python layer makes before any library call."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import halo_reference as HR  # noqa: E402
import halo_target_reference as TR  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU  # noqa: E402

_CACHE = {}


def _bases(planar):
    if planar not in _CACHE:
        if planar:
            got = [HR.correct(drivers.lyapunov_seed(w, 1e-2, MU)[0], HR.PLANAR, MU) for w in (1, 2)]
        else:
            got = [HR.correct(HR.seed_of(np.asarray(tb[:6], dtype=float)), HR.HOLD_X0, MU) for tb in synth.halo_orbits()]
        assert all(g.status == 0 for g in got)
        _CACHE[planar] = [(g.state, g.period) for g in got]
    return _CACHE[planar]


@pytest.mark.parametrize("what", [TR.JACOBI, TR.PERIOD])
@pytest.mark.parametrize("planar", [False, True])
def test_reference_converges_on_the_gpu_inputs_and_its_spread_is_a_tenth_of_the_bounds(planar, what):
    b_state, b_P = TR.BOUNDS[(planar, what)]
    worst = [0.0, 0.0, 0]
    for k, (seed, q) in enumerate(TR.cases(planar, what, _bases(planar), MU)):
        a = TR.target_correct(seed, q, what, planar, MU)
        l = TR.target_correct(seed, q, what, planar, MU, rtol=TR.LOOSE[0], atol=TR.LOOSE[1])
        assert a.status == 0 and l.status == 0, k
        d_state, d_P = np.abs(a.state - l.state).max(), abs(a.period - l.period)
        worst = [max(worst[0], d_state), max(worst[1], d_P), max(worst[2], a.iterations)]
        assert a.iterations <= TR.STEPS[(planar, what)], (k, a.iterations)
        assert d_state < 0.1 * b_state and d_P < 0.1 * b_P, (k, d_state, d_P)
        assert abs((HR.jacobi(a.state, MU) if what == TR.JACOBI else a.period) - q) < 1e-12
    print("%s %s: spread state %.2e (bound %.0e), period %.2e (bound %.0e), at most %d steps" % (
        "planar" if planar else "3-D", ("Jacobi", "period")[what], worst[0], b_state, worst[1], b_P, worst[2]))


def test_the_issue_s_planar_orbits_at_3_15():
    """(x0, vy0) and P of the L1 and L2 Lyapunov orbits at C = 3.15, in one call from the corrected Ax = 1e-2 seeds: 6 and 8 steps."""
    want = ((0.8159585220554, 0.2072659748358, 2.844831406797, 6), (1.1182824419945, 0.186019888512, 3.420569721966, 8))
    for (state, _), (x0, vy0, P, steps) in zip(_bases(True), want):
        a = TR.target_correct(state, TR.C_COMMON, TR.JACOBI, True, MU)
        assert a.status == 0 and a.iterations == steps
        assert abs(a.state[0] - x0) < 1e-12 and abs(a.state[4] - vy0) < 1e-12 and abs(a.period - P) < 1e-11


@pytest.mark.parametrize("K", [3, 4, 8])
def test_reference_march_to_3_15(K):
    b_state, b_P = TR.BOUNDS[(True, TR.JACOBI)]
    ends = []
    for state, _ in _bases(True):
        targets = drivers._step_table([HR.jacobi(state, MU)], TR.C_COMMON, K)[:, 0]
        a = TR.march(state, list(targets), TR.JACOBI, True, MU)
        l = TR.march(state, list(targets), TR.JACOBI, True, MU, rtol=TR.LOOSE[0], atol=TR.LOOSE[1])
        print("K=%d: steps %s" % (K, [m.iterations for m in a]))
        assert all(m.status == 0 for m in a + l) and max(m.iterations for m in a) <= 5 + 2
        for ma, ml in zip(a, l):
            assert np.abs(ma.state - ml.state).max() < 0.1 * b_state and abs(ma.period - ml.period) < 0.1 * b_P
        ends.append(a[-1])
    assert abs(ends[0].period - 2.844831406797) < 1e-11 and abs(ends[1].period - 3.420569721966) < 1e-11


def test_reference_march_of_halo_orbit_1_to_the_jacobi_constant_of_orbit_2():
    (s1, _), (s2, P2) = _bases(False)
    b_state, b_P = TR.BOUNDS[(False, TR.JACOBI)]
    targets = drivers._step_table([HR.jacobi(s1, MU)], HR.jacobi(s2, MU), 4)[:, 0]
    a = TR.march(s1, list(targets), TR.JACOBI, False, MU)
    l = TR.march(s1, list(targets), TR.JACOBI, False, MU, rtol=TR.LOOSE[0], atol=TR.LOOSE[1])
    assert all(m.status == 0 for m in a + l)
    for ma, ml in zip(a, l):
        assert np.abs(ma.state - ml.state).max() < 0.1 * b_state and abs(ma.period - ml.period) < 0.1 * b_P
    print("march to orbit 2: steps %s, end %.2e / %.2e from orbit 2" % (
        [m.iterations for m in a], np.abs(a[-1].state - s2).max(), abs(a[-1].period - P2)))
    assert np.abs(a[-1].state - s2).max() < 0.1 * b_state and abs(a[-1].period - P2) < 0.1 * b_P


def test_march_rules():
    """No predictor between equal targets; a failed member ends the march."""
    s = np.array([1.0, 0.0, 0.1, 0.0, 0.5, 0.0])
    assert np.array_equal(TR.predictor(s, 2.0 * s, 3.0, 2.0, 2.0), s)
    assert np.array_equal(TR.predictor(s, 2.0 * s, 3.0, 2.0, 1.0), s + (s - 2.0 * s) * 1.0)
    (state, _), _ = _bases(True)
    C = HR.jacobi(state, MU)
    m = TR.march(state, [C - 1e-3, np.nan, C - 2e-3], TR.JACOBI, True, MU)
    assert [x.status for x in m] == [0, 2, 2] and np.all(np.isnan(m[2].state))


@pytest.mark.parametrize("planar", [False, True])
def test_jacobi_row_is_the_gradient_of_the_jacobi_constant(planar):
    h = 1e-6
    for state, _ in _bases(planar):
        row = TR.jacobi_row(state[0], state[2], state[4], MU)
        cd = np.array([(HR.jacobi(state + h * np.eye(6)[j], MU) - HR.jacobi(state - h * np.eye(6)[j], MU)) / (2.0 * h) for j in (0, 2, 4)])
        print("dC/d(x0, z0, vy0) = %s, central difference off by %s" % (row, cd - row))
        assert np.abs(cd - row).max() < 1e-8             # h^2 C''' / 6 ~ 1e-11 and 2 ulp(C) / 2h ~ 4e-10


def _richardson(state, h):
    """The central difference quotient of 2 t_c in (x0, z0, vy0) at h and 2h, extrapolated: error O(h^4)."""
    def quotient(step):
        out = []
        for j in (0, 2, 4):
            e = step * np.eye(6)[j]
            out.append(2.0 * (HR.half_flight(state + e, MU)[0] - HR.half_flight(state - e, MU)[0]) / (2.0 * step))
        return np.array(out)
    return (4.0 * quotient(h) - quotient(2.0 * h)) / 3.0


@pytest.mark.parametrize("planar", [False, True])
def test_period_row_is_the_derivative_of_the_crossing_time(planar):
    """The bound is the quotient's own error: the h^4 term left after the extrapolation, measured as the change between the pairs
    (1e-5, 2e-5) and (2e-5, 4e-5) -- 7e-10 (halo) to 1.7e-4 (L2 Lyapunov, a row of 482) -- plus 1e-7 for the rounding of the crossing
    times (~1e-13 each, over 2h = 2e-5, times 2 x 4 / 3)."""
    for state, _ in _bases(planar):
        s = HR.perturbed(state, 3)                         # off the orbit: the row is not the gradient at a special point
        if planar:
            s[2] = 0.0
        _, J, _ = TR.system(s, 1.0, TR.PERIOD, False, MU)
        r1, r2 = _richardson(s, 1e-5), _richardson(s, 2e-5)
        own = np.abs(r1 - r2).max()
        print("d(2 t_c)/d(x0, z0, vy0) = %s, extrapolated quotient off by %s (its own error %.1e)" % (J[2], r1 - J[2], own))
        assert np.abs(r1 - J[2]).max() <= own + 1e-7


def test_the_singular_step_inputs_are_far_from_hadamard_s_bound():
    """tests/test_halo_target_gpu.py asks for sing_tol = 0.999 on these starts and expects status 3: |det| / prod < 0.9."""
    (s1, _), (s2, _) = _bases(False)
    for s, dq in ((s1, 1e-4), (s2, -1e-3)):
        _, J, _ = TR.system(s, HR.jacobi(s, MU) + dq, TR.JACOBI, False, MU)
        ratio = TR.singularity(J)
        print("|det| / product of the row norms = %.4f" % ratio)
        assert 0.0 < ratio < 0.9
        assert TR.target_correct(s, HR.jacobi(s, MU) + dq, TR.JACOBI, False, MU, sing_tol=0.999).status == 3


def test_driver_arithmetic():
    with pytest.raises(ValueError):
        drivers._one_target(None, None)
    with pytest.raises(ValueError):
        drivers._one_target(3.1, 2.9)
    assert drivers._one_target(3.1, None) == ("jacobi", 3.1) and drivers._one_target(None, 2.9) == ("period", 2.9)
    with pytest.raises(ValueError):
        drivers.halo_orbit_at(np.zeros(6))
    with pytest.raises(ValueError):
        drivers.halo_orbit_at(np.zeros(6), jacobi=3.0, period=3.0)
    # matched_orbits' step tables: n equal steps from each orbit's own C to the common one, the last row the target itself
    tab = drivers._step_table([3.18, 3.17, 3.15], 3.15, 4)
    assert tab.shape == (4, 3) and np.array_equal(tab[-1], [3.15, 3.15, 3.15])
    assert np.allclose(np.diff(tab, axis=0), [[-0.0075, -0.005, 0.0]] * 3, atol=1e-15) and np.allclose(tab[0], [3.1725, 3.165, 3.15])
    assert np.array_equal(drivers._step_table([3.18], 3.15, 1), [[3.15]])
    with pytest.raises(ValueError):
        drivers._step_table([3.18], 3.15, 0)
    s = np.array([1.1, 0.0, 0.02, 0.0, 0.2, 0.0])
    assert abs(drivers._jacobi_of(s, MU) - HR.jacobi(s, MU)) < 1e-15
    assert np.allclose(drivers._jacobi_of(np.array([s, s]).T, MU), HR.jacobi(s, MU), atol=1e-15)
    # the refinement window: n phases over centre -+ one previous spacing, ends included; it shrinks by n / 2
    p = drivers._refine_phases(0.5, 1.0 / 64.0, 5)
    assert np.array_equal(p, [0.484375, 0.4921875, 0.5, 0.5078125, 0.515625])
    p = drivers._refine_phases(0.25, 1.0 / 64.0, 16)
    assert p.size == 16 and p[0] == 0.25 - 1.0 / 64.0 and p[-1] == 0.25 + 1.0 / 64.0 and np.allclose(np.diff(p), 1.0 / 480.0, atol=1e-16)
    assert drivers._refine_shrink(1.0 / 64.0, 16) == 1.0 / 512.0
    h = 1.0 / 64.0
    for _ in range(4):
        h = drivers._refine_shrink(h, 16)
    assert h == 1.0 / 64.0 / 8.0 ** 4
    with pytest.raises(ValueError):
        drivers.matched_orbits(np.zeros(6), 3.15)
    with pytest.raises(ValueError):
        drivers.matched_orbits(np.zeros((6, 2)), np.nan)


def test_halo_target_rejects_malformed_input_before_any_library_call(monkeypatch):
    def no_context():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(lto.hotpath, "default_context", no_context)
    for bad in (np.zeros(5), np.zeros((5, 3)), np.zeros((6, 2, 2)), np.zeros((6, 0)), 1.0):
        with pytest.raises(ValueError):
            lto.halo_target(bad, 3.0)
    for bad_q in (np.zeros((2, 3)), np.zeros(0), np.zeros((1, 2, 2))):
        with pytest.raises(ValueError):
            lto.halo_target(np.ones((6, 2)), bad_q)
    with pytest.raises(ValueError):
        lto.halo_target(np.ones(6), np.zeros((2, 1)))        # a target table needs a batch of seeds
    for what in ("energy", 2, -1):
        with pytest.raises(ValueError):
            lto.halo_target(np.ones(6), 3.0, what=what)
    for kw in ({"max_iter": -1}, {"tol": 0.0}, {"tol": np.nan}, {"t_max": np.inf}, {"t_max": 0.0}, {"sing_tol": 1.0}, {"sing_tol": np.nan}):
        with pytest.raises(ValueError):
            lto.halo_target(np.ones(6), 3.0, **kw)
    with pytest.raises(ValueError):
        drivers.halo_family_by(np.ones(6), 3.0, "jacobi")
    with pytest.raises(AssertionError):
        lto.halo_target(np.ones(6), 3.0)                     # well-formed input does go on to the library
