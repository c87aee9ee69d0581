"""Independent host reference of the invariant-manifold calls.  Nothing here comes from the product; MU, the orbits
and their monodromy matrices are passed in by the tests.

  eigen      mpmath.eig at 50 digits on the same M the device is given, for both eigenvalues and both vectors
  transport  scipy's DOP853 at rtol 1e-13 / atol 1e-14 on the 12-component system (state + one variational vector), forward for v_u
             over tau P, backward for v_s over (1 - tau) P
  flights    solve_ivp with an event on the section, terminal = n_cross and direction (the integer form of `terminal`); a backward
             arc is the time-reversed system over a positive span, so `direction` is in the order the flight visits the points, as
             the device counts it; r_min by a scan of the accepted steps
  match      numpy with the summation order of include/lto.h"""
import collections

import mpmath
import numpy as np
from scipy.integrate import solve_ivp

RTOL, ATOL = 1e-13, 1e-14
LOOSE = (1e-11, 1e-12)


# ------------------------------------------------------------------------------------------------------------------------ eigen
def sign_rule(v):
    v = np.array(v, dtype=float)
    s = v[0] if v[0] != 0.0 else v[np.argmax(np.abs(v))]
    return -v if s < 0.0 else v


EigPair = collections.namedtuple("EigPair", "lam_u lam_s v_u v_s")


def eig_pair(M, digits=50):
    """(lambda_u, lambda_s, v_u, v_s) of M at `digits` digits: the eigenvalue of largest and of smallest modulus, unit vectors with
    the sign rule (v_x > 0); None if the dominant eigenvalue is not real (a complex pair) or M is not finite."""
    M = np.asarray(M, dtype=float)
    if not np.all(np.isfinite(M)):
        return None
    with mpmath.workdps(digits):
        E, ER = mpmath.eig(mpmath.matrix(M.tolist()))
        mods = [abs(e) for e in E]
        iu = max(range(6), key=lambda i: mods[i])
        i_s = min(range(6), key=lambda i: mods[i])
        tol = mpmath.mpf(10) ** (-(digits - 10))
        if abs(mpmath.im(E[iu])) > tol * mods[iu] or not mods[iu] > 1:
            return None
        out = []
        for i in (iu, i_s):
            col = [ER[r, i] for r in range(6)]
            big = max(col, key=abs)                                  # a real eigenvector up to a complex factor: take it out
            col = [mpmath.re(x / big) for x in col]
            n = mpmath.sqrt(sum(x * x for x in col))
            out.append(sign_rule([float(x / n) for x in col]))
        return EigPair(float(mpmath.re(E[iu])), float(mpmath.re(E[i_s])), out[0], out[1])


# -------------------------------------------------------------------------------------------------------------------- transport
def rhs12(MU, sgn=1.0):
    def f(t, w):
        x, y, z, vx, vy, vz = w[:6]
        a, b = x + MU, x + MU - 1.0
        r1 = np.sqrt(a * a + y * y + z * z)
        r2 = np.sqrt(b * b + y * y + z * z)
        c1, c2 = (1.0 - MU) / r1 ** 3, MU / r2 ** 3
        q1, q2 = 3.0 * (1.0 - MU) / r1 ** 5, 3.0 * MU / r2 ** 5
        out = np.empty(12)
        out[0:3] = (vx, vy, vz)
        out[3] = x + 2.0 * vy - c1 * a - c2 * b
        out[4] = y - 2.0 * vx - (c1 + c2) * y
        out[5] = -(c1 + c2) * z
        qa, qs = q1 * a + q2 * b, q1 + q2
        G = np.array([[1.0 - c1 - c2 + q1 * a * a + q2 * b * b, qa * y, qa * z],
                      [qa * y, 1.0 - c1 - c2 + qs * y * y, qs * y * z],
                      [qa * z, qs * y * z, -c1 - c2 + qs * z * z]])
        c = w[6:]
        out[6:9] = c[3:6]
        out[9:12] = G @ c[0:3] + np.array([2.0 * c[4], -2.0 * c[3], 0.0])
        return sgn * out
    return f


def transport(state0, period, v, tau, kind, MU, rtol=RTOL, atol=ATOL):
    """(x [6], v [6] unit) at phase tau: kind 0 forward over tau P, kind 1 backward over (1 - tau) P; tau = 0 flies nothing."""
    w = np.concatenate([np.asarray(state0, dtype=float), np.asarray(v, dtype=float)])
    span = 0.0 if tau == 0.0 else (tau * period if kind == 0 else (1.0 - tau) * period)
    if span > 0.0:
        s = solve_ivp(rhs12(MU, 1.0 if kind == 0 else -1.0), (0.0, span), w, method="DOP853", rtol=rtol, atol=atol)
        w = s.y[:, -1]
    return w[:6], w[6:] / np.linalg.norm(w[6:])


def seeds(state0, period, M, taus, MU, rtol=RTOL, atol=ATOL):
    """(lam [2], X [6 x 2 x P], V [6 x 2 x P]) of one orbit, the layout of the device's outputs."""
    e = eig_pair(M)
    P = len(taus)
    X, V = np.empty((6, 2, P)), np.empty((6, 2, P))
    for j, tau in enumerate(taus):
        for kind, v in enumerate((e.v_u, e.v_s)):
            X[:, kind, j], V[:, kind, j] = transport(state0, period, v, tau, kind, MU, rtol, atol)
    return np.array([e.lam_u, e.lam_s]), X, V


def starts_of(X, V, eps):
    """[6 x 4 x P] = X +- eps V in the order (u+, u-, s+, s-)."""
    return np.stack([X[:, 0] + eps * V[:, 0], X[:, 0] - eps * V[:, 0], X[:, 1] + eps * V[:, 1], X[:, 1] - eps * V[:, 1]], axis=1)


# ---------------------------------------------------------------------------------------------------------------------- flights
def rhs6(MU, sgn=1.0):
    def f(t, w):
        x, y, z, vx, vy, vz = w
        a, b = x + MU, x + MU - 1.0
        r1 = np.sqrt(a * a + y * y + z * z)
        r2 = np.sqrt(b * b + y * y + z * z)
        c1, c2 = (1.0 - MU) / r1 ** 3, MU / r2 ** 3
        return sgn * np.array([vx, vy, vz, x + 2.0 * vy - c1 * a - c2 * b, y - 2.0 * vx - (c1 + c2) * y, -(c1 + c2) * z])
    return f


Flight = collections.namedtuple("Flight", "x_end t_end count status closest")


def flight(y0, t_max, axis, value, MU, sec_dir=0, n_cross=1, rtol=RTOL, atol=ATOL):
    """One arc over the signed time t_max to the n_cross-th crossing of y[axis] = value: x_end, t_end (signed), count, status 0
    (crossing, or t_max with n_cross = 0) or 1 (t_max first), closest [2] = the smallest distances from the two primaries over the
    start and the accepted step ends (a located crossing is not a step end)."""
    sgn = -1.0 if t_max < 0.0 else 1.0
    events = None
    if n_cross > 0:
        def ev(t, w):
            return w[axis] - value
        ev.terminal = int(n_cross)
        ev.direction = float(sec_dir)
        events = ev
    s = solve_ivp(rhs6(MU, sgn), (0.0, abs(t_max)), np.asarray(y0, dtype=float), method="DOP853", rtol=rtol, atol=atol, events=events)
    Y = s.y[:, :-1] if s.status == 1 else s.y          # ended by the event: the last column is the located crossing, not a step end
    d1 = np.sqrt((Y[0] + MU) ** 2 + Y[1] ** 2 + Y[2] ** 2)
    d2 = np.sqrt((Y[0] + MU - 1.0) ** 2 + Y[1] ** 2 + Y[2] ** 2)
    closest = np.array([d1.min(), d2.min()])
    if n_cross > 0:
        count = int(s.t_events[0].size)
        if s.status == 1:
            return Flight(s.y_events[0][-1], sgn * s.t_events[0][-1], count, 0, closest)
        return Flight(s.y[:, -1], sgn * s.t[-1], count, 1, closest)
    return Flight(s.y[:, -1], sgn * s.t[-1], 0, 0, closest)


def flight_samples(y0, t_max, n, MU, rtol=RTOL, atol=ATOL):
    """[6 x n]: the arc stopped at t_k = k |t_max| / (n - 1), every interval a solve of its own (no interpolant)."""
    sgn = -1.0 if t_max < 0.0 else 1.0
    T = abs(t_max)
    dt = T / (n - 1)
    X = np.empty((6, n))
    w = np.asarray(y0, dtype=float)
    X[:, 0] = w
    tp = 0.0
    for i in range(1, n):
        ti = T if i == n - 1 else i * dt
        w = solve_ivp(rhs6(MU, sgn), (tp, ti), w, method="DOP853", rtol=rtol, atol=atol).y[:, -1]
        X[:, i] = w
        tp = ti
    return X


# ------------------------------------------------------------------------------------------------------------------------ match
def match_distances(A, Bs, w):
    """(d, dr, dv) [nA x nB] in the summation order of include/lto.h; numpy rounds every product and every sum on its own."""
    q = (A[:, :, None] - Bs[:, None, :]) ** 2
    dr2 = (q[0] + q[1]) + q[2]
    dv2 = (q[3] + q[4]) + q[5]
    return np.sqrt(dr2 + (w * w) * dv2), np.sqrt(dr2), np.sqrt(dv2)


def match(A, Bs, w):
    """(index [nA], dist, dr, dv): the lowest index of the smallest distance, NaN never wins, -1 and NaN for an all-NaN row."""
    d, dr, dv = match_distances(A, Bs, w)
    nA = A.shape[1]
    idx = np.full(nA, -1, dtype=np.int64)
    out = np.full((3, nA), np.nan)
    for i in range(nA):
        if not np.all(np.isnan(d[i])):
            j = int(np.nanargmin(d[i]))
            idx[i] = j
            out[:, i] = d[i, j], dr[i, j], dv[i, j]
    return idx, out[0], out[1], out[2]


def second_best_gap(A, Bs, w):
    """The smallest relative gap between the best and the second-best distance over the rows of A (inf with one candidate)."""
    d, _, _ = match_distances(A, Bs, w)
    if d.shape[1] < 2:
        return np.inf
    s = np.sort(d, axis=1)
    return float(np.min((s[:, 1] - s[:, 0]) / s[:, 0]))


# ------------------------------------------------------------------------------------------------------- the tests' shared inputs
_SHARED = {}


def packaged_orbits(tables, MU):
    """[(state0, period, M)] of the packaged orbits, corrected holding x0 and tabled by tests/halo_reference.py; computed once."""
    import halo_reference as HR
    if "orbits" not in _SHARED:
        out = []
        for tb in tables:
            c = HR.correct(HR.seed_of(np.asarray(tb[:6], dtype=float)), HR.HOLD_X0, MU)
            _, M = HR.table(c.state, c.period, 100, MU)
            out.append((c.state, c.period, M))
        _SHARED["orbits"] = out
    return _SHARED["orbits"]


def shared_seeds(orbits, k, n_phase, MU, rtol=RTOL, atol=ATOL):
    """seeds() of orbit k at the phases j / n_phase; computed once per (k, n_phase, tolerance)."""
    key = ("seeds", k, n_phase, rtol)
    if key not in _SHARED:
        s, P, M = orbits[k]
        _SHARED[key] = seeds(s, P, M, np.arange(n_phase) / float(n_phase), MU, rtol, atol)
    return _SHARED[key]


def vetted_starts(orbits, eps, MU):
    """The 64 starts of the flight tests: both orbits, phases j / 8, the four branches -- arc = 32 k + 4 j + m, m in the order (u+,
    u-, s+, s-) -- and the sign of their flight time (stable arcs fly backward)."""
    key = ("starts", eps)
    if key not in _SHARED:
        cols = []
        for k in range(2):
            _, X, V = shared_seeds(orbits, k, 8, MU)
            st = starts_of(X, V, eps)
            cols += [st[:, m, j] for j in range(8) for m in range(4)]
        sign = np.array([1.0 if (i % 4) < 2 else -1.0 for i in range(64)])
        _SHARED[key] = (np.array(cols).T.copy(), sign)
    return _SHARED[key]


def shared_flight(y0, t_max, axis, value, MU, sec_dir=0, n_cross=1, rtol=RTOL, atol=ATOL):
    key = ("flight", tuple(y0), t_max, axis, value, sec_dir, n_cross, rtol)
    if key not in _SHARED:
        _SHARED[key] = flight(y0, t_max, axis, value, MU, sec_dir, n_cross, rtol, atol)
    return _SHARED[key]
