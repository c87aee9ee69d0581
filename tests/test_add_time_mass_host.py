"""CPU checks behind the 14-row addTimeFinal tests (no GPU, no library code under test): the restatement's control-law
magnitude against the oracle's right-hand side, the facts about the tail that the specification states -- the 14-row system's own
flow from a node whose costates are zero -- on the oracle's flow, and the operator norm of the re-mesh map that the GPU bars use.

Measured here: umag14 against -dy[6] / (kappa m) of the oracle 5.9e-16 relative over 600 states; tail: rows 7..13 exactly 0, p > 1 mass
bit-constant, p = 0 loss against thrustLimit / (Isp 9.81) TU dt 1.2e-14 relative, rows 0..5 against the 12-row flow 1.1e-14
(bar 1e-11); Lambda = 1.0000, 1.3000, 1.3884, 1.0000, 1.5484 for (n_desired, n) = (4, 2), (4, 3), (5, 9), (65, 9), (200, 30).

Every test prints its figures before it asserts (MEASURED lines)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import addtime_mass_reference as AM  # noqa: E402
import mass_dense_reference as M  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU, day  # noqa: E402

# (label, thrust N, Isp s, p, rho, |lambda_v| as a multiple of the clamp threshold p (cT / m)^(p-1), or None: free)
CLASSES = (("p0", 10.0, 2000.0, 0.0, 1.0, None),
           ("p1", 10.0, 2000.0, 1.0, 0.5, None),
           ("p2-unclamped", 10.0, 2000.0, 2.0, 1.0, 0.4),
           ("p2-clamped", 10.0, 2000.0, 2.0, 1.0, 2.5),
           ("p1.5-unclamped", 0.05, 300.0, 1.5, 1.0, 0.7),
           ("p3-clamped", 0.05, 300.0, 3.0, 1.0, 1.6))


def _state(rng, thrust, p, factor):
    y = np.zeros(14)
    y[:6] = [1.02 + 0.1 * rng.uniform(-1, 1), 0.05 * rng.uniform(-1, 1), 0.05 * rng.uniform(-1, 1), *(0.3 * rng.uniform(-1, 1, 3))]
    y[6] = rng.uniform(300.0, 1500.0)
    y[7:10] = rng.normal(0.0, 1.0, 3)
    lv = rng.normal(0.0, 1.0, 3)
    lv /= np.linalg.norm(lv)
    if factor is None:
        lv *= rng.uniform(0.0, 3.0)
    else:
        lv *= factor * rng.uniform(0.8, 1.2) * p * (AM.c_thrust(thrust, DU, TU) / y[6]) ** (p - 1.0)
    y[10:13] = lv
    y[13] = rng.uniform(-1.0, 1.0)
    return y


@pytest.mark.parametrize("label,thrust,isp,p,rho,factor", CLASSES, ids=[c[0] for c in CLASSES])
def test_umag14_is_the_oracles(oracle, label, thrust, isp, p, rho, factor):
    rng = np.random.default_rng(11)
    prm = [MU, DU, TU, thrust, isp, 1.0, p, rho]
    kap = AM.kappa(isp, DU, TU)
    worst, clamped = 0.0, 0
    for _ in range(100):
        y = _state(rng, thrust, p, factor)
        dy = oracle.rhs_state_costate_mass(y, prm)
        want = -dy[6] / (kap * y[6])
        got = float(AM.umag14(y[10:13, None], y[6], thrust, p, rho, DU, TU)[0])
        aL = AM.c_thrust(thrust, DU, TU) / y[6]
        clamped += got == aL
        assert got > 0.0
        worst = max(worst, abs(got - want) / abs(want))
    print("MEASURED umag14 %s: worst relative difference from -dy[6] / (kappa m) %.3e (bar 1e-14), %d of 100 at aL" % (label, worst, clamped))
    if factor is not None:
        assert clamped == (100 if factor > 1.0 else 0)               # the class is the one the label names
    if p == 0.0:
        assert clamped == 100
    assert worst <= 1e-14


def test_umag14_counts_a_mass_that_is_not_positive_as_zero():
    """The rule of k_dense_cost_mass for a sample a failed re-solve can leave: no infinite or negative magnitude enters a cost."""
    lv = np.array([[0.3], [0.1], [-0.2]])
    for p, rho in ((0.0, 1.0), (1.0, 0.5), (2.0, 1.0), (3.0, 1.0)):
        for m in (0.0, -3.0, np.nan):
            assert AM.umag14(lv, m, 10.0, p, rho, DU, TU)[0] == 0.0
        assert AM.umag14(lv, 1000.0, 10.0, p, rho, DU, TU)[0] > 0.0


def _tail_node(k):
    X, t, prm = M.fixture(9, k)
    y = np.array(X[:, -1])
    y[7:14] = 0.0
    return y, prm


@pytest.mark.parametrize("k", [0, 1, 2, 3, 5], ids=lambda k: M.SETS[k].name)
def test_tail_facts_on_the_oracle_flow(oracle, k):
    """The tail of step 1 is the 14-row system's own flow from a node with rows 7..13 zero."""
    y, prm = _tail_node(k)
    s = M.SETS[k]
    bar = max(1e-11, 10.0 * M.e_inf())
    prm12 = [MU, DU, TU, s.thrust, y[6], 1.0, s.p, s.rho]
    for dt in np.array([0.25, 1.0]) * day / TU:
        z = M.flow14(oracle, y, prm, dt)
        assert np.all(z[7:14] == 0.0), z[7:14]                          # exactly
        y12, rc, _, _ = oracle.flow_state_costate(y[M.IDX12], prm12, dt, oracle.DOP853_ADAPTIVE)
        assert rc == 0
        e = M.rel_rows(z[:6], y12[:6])
        print("MEASURED tail %s dt %.3f TU: rows 0..5 against the 12-row flow with zero costates %.3e (bar %.1e), mass %.17g -> %.17g"
              % (s.name, dt, e, bar, y[6], z[6]))
        assert e <= bar
        if s.p > 1.0:
            assert z[6] == y[6]                                       # umag(0, m) = 0: bit for bit
        elif s.p == 0.0:
            want = s.thrust / (s.isp * 9.81) * TU * dt
            rel = abs((y[6] - z[6]) - want) / want
            print("MEASURED tail %s dt %.3f TU: loss %.12f kg against thrustLimit / (Isp 9.81) TU dt, relative %.3e (bar 1e-13)" % (s.name, dt, y[6] - z[6], rel))
            assert rel <= 1e-13
        else:
            idle = AM.c_thrust(s.thrust, DU, TU) / (1.0 + np.exp(1.0 / s.rho))      # umag(0, m) m: the law's idle flow, mass-free
            want = AM.kappa(s.isp, DU, TU) * idle * dt
            assert z[6] < y[6]
            # a constant rate: the flow is linear in time, so only the roundings of a mass near m0 remain
            assert abs((y[6] - z[6]) - want) <= 1e-13 * want + 4.0 * M.EPS * y[6]


def test_operator_norm_of_the_remesh_map():
    """Lambda for the demo's (200, 30) and the shapes of the GPU sweep: the factor between an error in the samples and the error of
    a re-meshed node."""
    shapes = tuple((m, n) for n, m in AM.SHAPES)
    assert (200, 30) in shapes
    for m, n in shapes:
        lam = AM.spline_norm(m, n)
        print("MEASURED Lambda(n_desired = %d, n = %d) = %.4f" % (m, n, lam))
        assert np.isfinite(lam) and lam >= 1.0 - 4.0 * M.EPS          # nodes 0 and n-1 are samples: their row sums are 1
