"""Independent host reference of the periodic-orbit corrector and table: scipy's DOP853 on the 42-component system
(state + state-transition matrix) at rtol 1e-13 / atol 1e-14, a terminal event on y for the first return to the xz-plane, the same
Newton rule as the device (residual (vx, vz), Jacobian corrected for the moving crossing time), eigenvalues by numpy.  Nothing here
comes from the product; MU and the packaged tables are passed in by the tests."""
import collections

import numpy as np
from scipy.integrate import solve_ivp

HOLD_Z0, HOLD_X0, PLANAR = 0, 1, 2
RTOL, ATOL = 1e-13, 1e-14


def rhs42(MU):
    def f(t, w):
        x, y, z, vx, vy, vz = w[:6]
        a, b = x + MU, x + MU - 1.0
        r1 = np.sqrt(a * a + y * y + z * z)
        r2 = np.sqrt(b * b + y * y + z * z)
        c1, c2 = (1.0 - MU) / r1 ** 3, MU / r2 ** 3
        q1, q2 = 3.0 * (1.0 - MU) / r1 ** 5, 3.0 * MU / r2 ** 5
        out = np.empty(42)
        out[0:3] = (vx, vy, vz)
        out[3] = x + 2.0 * vy - c1 * a - c2 * b
        out[4] = y - 2.0 * vx - (c1 + c2) * y
        out[5] = -(c1 + c2) * z
        G = np.array([[1.0 - c1 - c2 + q1 * a * a + q2 * b * b, (q1 * a + q2 * b) * y, (q1 * a + q2 * b) * z],
                      [(q1 * a + q2 * b) * y, 1.0 - c1 - c2 + (q1 + q2) * y * y, (q1 + q2) * y * z],
                      [(q1 * a + q2 * b) * z, (q1 + q2) * y * z, -c1 - c2 + (q1 + q2) * z * z]])
        A = np.zeros((6, 6))
        A[0:3, 3:6] = np.eye(3)
        A[3:6, 0:3] = G
        A[3, 4], A[4, 3] = 2.0, -2.0
        out[6:] = (A @ w[6:].reshape(6, 6)).ravel()
        return out
    return f


def start42(state):
    return np.concatenate([np.asarray(state, dtype=float), np.eye(6).ravel()])


def half_flight(state, MU, t_max=10.0, rtol=RTOL, atol=ATOL):
    """(t, x [6], Phi [6 x 6], f [6]) at the first return of y to 0 after t = 0; None if there is none before t_max."""
    def ev(t, w):
        return w[1]
    ev.terminal = True
    ev.direction = -1.0 if state[4] > 0.0 else 1.0
    sol = solve_ivp(rhs42(MU), (0.0, t_max), start42(state), method="DOP853", rtol=rtol, atol=atol, events=ev)
    if sol.t_events[0].size == 0:
        return None
    w = sol.y_events[0][0]
    return sol.t_events[0][0], w[:6], w[6:].reshape(6, 6), rhs42(MU)(0.0, w)[:6]


Corrected = collections.namedtuple("Corrected", "state period resid iterations history status")


def correct(seed, mode, MU, tol=1e-12, max_iter=15, t_max=10.0, rtol=RTOL, atol=ATOL):
    """The corrector: status 0 converged, 1 max_iter reached, 2 no crossing."""
    x0, z0, vy0 = float(seed[0]), float(seed[2]), float(seed[4])
    hist, it = [], 0
    while True:
        state = np.array([x0, 0.0, z0, 0.0, vy0, 0.0])
        fl = half_flight(state, MU, t_max, rtol, atol)
        if fl is None:
            return Corrected(state * np.nan, np.nan, np.nan, it, hist, 2)
        tc, xc, Phi, f = fl
        r = np.array([xc[3]]) if mode == PLANAR else np.array([xc[3], xc[5]])
        res = np.abs(r).max()
        hist.append(res)
        if res < tol:
            return Corrected(state, 2.0 * tc, res, it, hist, 0)
        if it >= max_iter:
            return Corrected(state, 2.0 * tc, res, it, hist, 1)
        rows = [3] if mode == PLANAR else [3, 5]
        cols = [4] if mode == PLANAR else ([0, 4] if mode == HOLD_Z0 else [2, 4])
        J = Phi[np.ix_(rows, cols)] - np.outer(f[rows], Phi[1, cols]) / f[1]
        d = np.linalg.solve(J, r)
        if mode == PLANAR:
            vy0 -= d[0]
        else:
            if mode == HOLD_Z0:
                x0 -= d[0]
            else:
                z0 -= d[0]
            vy0 -= d[1]
        it += 1


def count_is_safe(history, tol):
    """No residual of a reference run lies within [tol / 10, 10 tol]: the device, whose residuals are this reference's to 1e-11 and
    in practice to 1e-13, then stops at the same iteration, and its count is held to this one exactly, not to within one."""
    return not any(0.1 * tol <= h <= 10.0 * tol for h in history)


def same_count(iterations, ref_iterations, ref_history, tol):
    """The device's iteration count against a reference run's: equal where the count is safe, within one elsewhere."""
    if count_is_safe(ref_history, tol):
        return int(iterations) == int(ref_iterations)
    return abs(int(iterations) - int(ref_iterations)) <= 1


def jacobi(state, MU):
    x, y, z, vx, vy, vz = state
    r1 = np.sqrt((x + MU) ** 2 + y * y + z * z)
    r2 = np.sqrt((x + MU - 1.0) ** 2 + y * y + z * z)
    return x * x + y * y + 2.0 * (1.0 - MU) / r1 + 2.0 * MU / r2 - (vx * vx + vy * vy + vz * vz)


def table(state0, period, n, MU, rtol=RTOL, atol=ATOL):
    """(X [6 x n] at t_i = i P / (n - 1), M = Phi(P)) once round the orbit, stopping at every sample (no interpolant)."""
    t = np.linspace(0.0, period, n)
    X = np.empty((6, n))
    w = start42(state0)
    X[:, 0] = w[:6]
    for i in range(1, n):
        s = solve_ivp(rhs42(MU), (t[i - 1], t[i]), w, method="DOP853", rtol=rtol, atol=atol)
        w = s.y[:, -1]
        X[:, i] = w[:6]
    return X, w[6:].reshape(6, 6)


def nu_from_traces(M):
    """The two stability indices from tr M and tr M^2 (NaN for a negative discriminant)."""
    alpha = 2.0 - np.trace(M)
    beta = 0.5 * (alpha * alpha + 2.0 - np.trace(M @ M))
    disc = alpha * alpha - 4.0 * beta + 8.0
    root = np.sqrt(disc) if disc >= 0.0 else np.nan
    return np.array([-0.25 * (alpha + root), -0.25 * (alpha - root)])


def nu_from_eigenvalues(M):
    """(lambda + 1 / lambda) / 2 of the two non-trivial reciprocal pairs, in the order of nu_from_traces."""
    lam = np.linalg.eigvals(M)
    lam = lam[np.argsort(np.abs(lam - 1.0))][2:]              # drop the pair at 1
    nus = np.real(0.5 * (lam + 1.0 / lam))
    nus = np.sort(nus)
    return np.array([nus[0], nus[-1]])


def family(seed, values, hold, MU, tol=1e-12):
    """Natural-parameter continuation with a secant predictor through the last two points (the seed counts as the first; the first
    step starts from the seed itself); returns the list of Corrected members."""
    ip = 0 if hold == "x0" else 2
    mode = HOLD_X0 if hold == "x0" else HOLD_Z0
    members, pts = [], [np.array(seed, dtype=float)]
    for v in values:
        b = pts[-1]
        if len(pts) >= 2 and pts[-2][ip] != b[ip]:
            a = pts[-2]
            guess = b + (b - a) * (v - b[ip]) / (b[ip] - a[ip])
        else:
            guess = b.copy()
        guess[ip] = v
        m = correct(guess, mode, MU, tol=tol)
        members.append(m)
        pts.append(m.state)
    return members


def seed_of(tab):
    """The packaged seed: column 1 of a table with y, vx and vz zeroed."""
    s = np.array(tab[:6, 0], dtype=float)
    s[[1, 3, 5]] = 0.0
    return s


def perturbed(seed, k):
    """Deterministic copies of a seed moved by at most 1e-4 in position and 1e-3 in vy0."""
    rng = np.random.RandomState(1234 + k)
    s = seed.copy()
    s[0] += 1e-4 * rng.uniform(-1, 1)
    s[2] += 1e-4 * rng.uniform(-1, 1)
    s[4] += 1e-3 * rng.uniform(-1, 1)
    return s


def gpu_seeds(base, hold):
    """The 17 halo seeds the GPU tests correct (tests/test_halo_gpu.py), vetted on the host (tests/test_halo_host.py: each converges
    under this reference in <= 4 steps): the two packaged seeds `base` and 15 perturbed copies.  Holding x0 the copies alternate
    between the two orbits; holding z0 they are all copies of orbit 1 -- near orbit 2 the family is so steep in (z0, x0) that the
    fixed-z0 Newton iteration leaves it from offsets of this size, in this reference as anywhere (4 of 7 such copies did)."""
    return np.array(list(base) + [perturbed(base[k % 2 if hold == "x0" else 0], k) for k in range(15)]).T


# x-amplitudes of the Lyapunov seeds the GPU tests correct at L1 and L2, vetted on the host (tests/test_halo_host.py).  The period of
# a small planar orbit is ill-conditioned -- the crossing time moves by dy / vy with vy ~ 2 Ax, and y inherits the absolute error of
# x ~ 1 -- so that at Ax = 1e-4 and 1e-3 this reference's own period moves by 1e-11 and 2.5e-12 between tolerances, no better than
# the bound the device is held to; from Ax = 3e-3 on it moves by less than a tenth of it.
PLANAR_AX = (3e-3, 5e-3, 1e-2)
