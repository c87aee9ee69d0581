"""Host restatement of addTimeFinal for the 14-row variable-mass system (lto_indirect_add_time_mass_batch) -- CPU only,
plain numpy, no library code under test.  The re-mesh and the snap are addtime_reference.remesh / find_tau_from_samples, which do
not care about the row count; this module adds step 1 (extended14), the 14-row law's magnitude (umag14), the cost of a dense output
in long double (dense_cost14, as dense_reference.dense_cost_ld) and the operator norm of the re-mesh (spline_norm).

Rows: y = (r 0..2, v 3..5, m 6, lambda_r 7..9, lambda_v 10..12, lambda_m 13).  The parameter tuple carries Isp in the mass slot:
(MU, DU, TU, thrustLimit, Isp, time_direction, p, rho)."""
import functools

import numpy as np

import addtime_reference as A

# (n, n_desired) of the spline-shape sweep of tests/test_add_time_mass_shapes_gpu.py
SHAPES = ((2, 4), (3, 4), (9, 5), (9, 65), (30, 200))
SHAPE_K = (1, 4, 5, 9)                               # 14, 56, 70 and 126 lanes in workgroups of 64


def extended14(XC, t, dt):
    """Step 1: a copy of XC [14 x n] with rows 7..13 of its last node zeroed and a tail node at t[-1] + dt (the node's value is never
    used: the tail is the flow of node n-1)."""
    XC = np.array(XC, dtype=np.float64, order="F")
    assert XC.shape[0] == 14
    XC[7:14, -1] = 0.0
    XCe = np.asfortranarray(np.hstack([XC, XC[:, -1:]]))
    te = np.append(np.asarray(t, dtype=np.float64), t[-1] + dt)
    return XCe, te


def c_thrust(thrustLimit, DU, TU):
    """cT = thrustLimit / 1e3 TU^2 / DU: aL = cT / m."""
    return thrustLimit / 1e3 * TU ** 2 / DU


def kappa(Isp, DU, TU, td=1.0):
    """mdot = -kappa umag m."""
    return td * 1e3 * DU / (TU * Isp * 9.81)


def umag14(lam_v, m, thrustLimit, p, rho, DU, TU):
    """Magnitude of the 14-row law's thrust acceleration in DU/TU^2 at |lambda_v| and the state's own mass m: aL = cT / m; p = 0:
    aL; p = 1: 1/2 (1 + tanh((n - 1) / (2 rho))) aL; p > 1: min((n / p)^(1 / (p - 1)), aL).  A NaN counts 0 (as
    addtime_reference.umag), and so does a mass that is not positive."""
    m = np.asarray(m, dtype=np.float64)
    with np.errstate(all="ignore"):
        aL = c_thrust(thrustLimit, DU, TU) / m
    n = np.linalg.norm(np.asarray(lam_v, dtype=np.float64), axis=0)
    with np.errstate(all="ignore"):
        if p == 0:
            u = aL + 0.0 * n
        elif p == 1:
            u = 0.5 * (1.0 + np.tanh((n - 1.0) / (2.0 * rho))) * aL
        else:
            u = np.minimum((n / p) ** (1.0 / (p - 1.0)), aL)
    return np.where(np.isnan(u) | ~(m > 0.0), 0.0, u)


def dense_cost14(XC_dense, t_dense, thrustLimit, p, rho, DU, TU):
    """Trapezoid of umag14 over a 14-row dense output, accumulated in long double, DU/TU.  Returns (cost, u): u the float64
    magnitude at every sample, for the branch checks."""
    Y = np.asarray(XC_dense, dtype=np.float64)
    u = umag14(Y[10:13], Y[6], thrustLimit, p, rho, DU, TU)
    t = np.asarray(t_dense, dtype=np.float64).astype(np.longdouble)
    ul = u.astype(np.longdouble)
    return float(np.sum(np.diff(t) * (ul[1:] + ul[:-1]) / np.longdouble(2.0))), u


@functools.lru_cache(maxsize=None)
def spline_norm(m, n):
    """Lambda: the infinity-operator norm of the re-mesh map, samples on LinRange (m knots) -> values at LinRange (n new nodes) --
    the largest row sum of |natural_spline(td, I, t_new)|.  An input error of e in the samples moves a re-meshed node by at most
    Lambda e.  The map does not depend on the interval (the knots are uniform)."""
    td = A.linrange(0.0, 1.0, m)
    W = A.natural_spline(td, np.eye(m), A.linrange(0.0, 1.0, n))        # [m x n]: column k = the weights of new node k
    return float(np.abs(W).sum(axis=0).max())
