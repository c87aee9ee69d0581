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


def eig_pair(M, digits=50, reciprocal=False):
    """(lambda_u, lambda_s, v_u, v_s) of M at `digits` digits: the eigenvalue of largest and of smallest modulus, unit vectors with
    the sign rule (v_x > 0); None if the dominant eigenvalue is not real (a complex pair) or M is not finite.  reciprocal: lambda_s
    is the eigenvalue nearest 1 / lambda_u instead, what inverse iteration with that shift looks for -- the same one for a
    monodromy matrix, another for a matrix without reciprocal pairs."""
    M = np.asarray(M, dtype=float)
    if not np.all(np.isfinite(M)):
        return None
    with mpmath.workdps(digits):
        E, ER = mpmath.eig(mpmath.matrix(M.tolist()))
        mods = [abs(e) for e in E]
        iu = max(range(6), key=lambda i: mods[i])
        i_s = min(range(6), key=(lambda i: abs(E[i] - 1 / E[iu])) if reciprocal else (lambda i: mods[i]))
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


def synthetic_monodromy(seed, lam_u, second, negative=False, mix=0.3, detune=0.0):
    """Q D Q^-1 with the reciprocal pairs (lam_u, 1 / lam_u), (second, 1 / second) and the rotation pair e^{+-i}; lam_u < 0 with
    `negative`.  Q = I + mix U(-1, 1) is a generic matrix, so v_s is NOT the mirrored v_u (the pattern of test_manifold_host's
    synthetic_M, with the spectrum and the seed free).  detune: lambda_s = (1 + detune) / lam_u, so the inverse iteration's shift
    1 / lambda_u misses it by that much and more than one solve is needed (with an exact shift a single solve of the nearly
    singular system returns v_s from ANY right-hand side, and nothing the solve does to it can be seen)."""
    rng = np.random.RandomState(seed)
    Q = np.eye(6) + mix * rng.uniform(-1.0, 1.0, (6, 6))
    c, s = np.cos(1.0), np.sin(1.0)
    lam = -float(lam_u) if negative else float(lam_u)
    D = np.zeros((6, 6))
    D[0, 0], D[1, 1] = lam, (1.0 + detune) / lam
    D[2, 2], D[3, 3] = float(second), 1.0 / float(second)
    D[4:, 4:] = np.array([[c, -s], [s, c]])
    return Q @ D @ np.linalg.inv(Q)


def permuted(M, perm):
    """P M P^T for the permutation matrix P = I[perm]: row i of the result is row perm[i] of M, and the columns alike."""
    p = np.asarray(perm)
    return np.asarray(M, dtype=float)[np.ix_(p, p)]


def permuted_pair(e, perm):
    """The 50-digit reference of P M P^T from that of M: the eigenvalues are M's, the vectors P v followed by the sign rule."""
    p = np.asarray(perm)
    return EigPair(e.lam_u, e.lam_s, sign_rule(e.v_u[p]), sign_rule(e.v_s[p]))


POWER_CAP, INVERSE_CAP = 500, 8                      # LTO_MANIFOLD_POWER_CAP, LTO_MANIFOLD_INVERSE_CAP of include/lto.h
Restated = collections.namedtuple("Restated", "status power_its last_move pivots margin inverse_its lam_u lam_s v_u v_s")


def _unit_step(w, v):
    """sign w / |w| with the sign that makes w . v >= 0, and how far that is from v in max-abs."""
    s = -1.0 if float(w @ v) < 0.0 else 1.0
    u = s * (w / np.sqrt(float(w @ w)))
    return u, float(np.abs(u - v).max())


def eigen_restatement(M, power_cap=POWER_CAP, inverse_cap=INVERSE_CAP):
    """The eigen step as include/lto.h words it, in numpy: power iteration from the fixed start (1, .9, .8, .7, .6, .5) / |.|, the
    iterate's sign aligned with the one before it, converged when it moves by < 1e-15 in max-abs, at most power_cap iterations;
    lambda_u its Rayleigh quotient; inverse iteration on M - I / lambda_u from v_u mirrored in the xz-plane, a 6 x 6 LU with partial
    pivoting (the first of equal maxima), at most inverse_cap solves; lambda_s the Rayleigh quotient of v_s; the sign rule last.

    Written from the header, not from the kernel; numpy rounds every product on its own where the device may fuse, so the two need
    not agree to the bit.  It vets inputs -- which rows the LU exchanges (pivots [6], pivots[k] = the row exchanged with row k;
    margin = the smallest ratio of a chosen pivot to the runner-up, so a near-tie is seen), how many iterations are taken and how
    far the iterate still moves at the end (last_move) -- and measures what the documented algorithm delivers.  It is never the
    expected value of a comparison with the device."""
    A = np.asarray(M, dtype=float)
    nan6 = np.full(6, np.nan)
    if not np.all(np.isfinite(A)):
        return Restated(1, 0, np.nan, None, np.nan, 0, np.nan, np.nan, nan6, nan6)
    vu = np.array([1.0, 0.9, 0.8, 0.7, 0.6, 0.5])
    vu = vu / np.sqrt(float(vu @ vu))
    conv, its, move = False, 0, np.inf
    while its < power_cap and not conv:
        vu, move = _unit_step(A @ vu, vu)
        its += 1
        conv = move < 1e-15
    lam_u = float(vu @ (A @ vu))
    if not conv or not abs(lam_u) > 1.0:
        return Restated(1, its, move, None, np.nan, 0, lam_u, np.nan, nan6, nan6)
    C = A - np.eye(6) / lam_u
    piv, margin = [], np.inf
    for k in range(6):
        col = np.abs(C[k:, k])
        p = k + int(np.argmax(col))                                  # argmax: the first of equal maxima
        if col.size > 1:
            rest = np.delete(col, p - k).max()
            margin = min(margin, col[p - k] / rest if rest > 0.0 else np.inf)
        piv.append(p)
        C[[k, p]] = C[[p, k]]
        if C[k, k] == 0.0:
            C[k, k] = 2.220446049250313e-16 * abs(lam_u)
        for r in range(k + 1, 6):
            ell = C[r, k] / C[k, k]
            C[r, k] = ell
            C[r, k + 1:] = C[r, k + 1:] - ell * C[k, k + 1:]
    vs = np.where(np.arange(6) & 1, -vu, vu)
    iits, conv = 0, False
    while iits < inverse_cap and not conv:
        x = vs.copy()
        for k in range(6):                                           # P x: every exchange, in the order they were made (whole rows
            x[[k, piv[k]]] = x[[piv[k], k]]                          # of C were exchanged, the multipliers left of k with them)
        for k in range(6):                                           # L y = P x
            x[k + 1:] = x[k + 1:] - C[k + 1:, k] * x[k]
        for k in range(5, -1, -1):                                   # U z = y
            x[k] = (x[k] - float(C[k, k + 1:] @ x[k + 1:])) / C[k, k]
        vs, imove = _unit_step(x, vs)
        iits += 1
        conv = imove < 1e-15
    lam_s = float(vs @ (A @ vs))
    if not np.all(np.isfinite(vs)) or not np.isfinite(lam_s):
        return Restated(1, its, move, tuple(piv), margin, iits, lam_u, np.nan, nan6, nan6)
    return Restated(0, its, move, tuple(piv), float(margin), iits, lam_u, lam_s, sign_rule(vu), sign_rule(vs))


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


def sign_changes(y0, t_max, axis, value, MU, until, dt=0.005, rtol=RTOL, atol=ATOL):
    """(times [n], slopes [n]) of the sign changes of g = y[axis] - value along the arc over the first `until` time units (at most
    |t_max|), from the dense output of one solve without an event, sampled every dt: times count from the start and are positive,
    located by linear interpolation between two samples; slopes are dg/ds along the flight at those times.  Two sign changes
    closer than dt are missed; the callers ask for a distance forty times that."""
    sgn = -1.0 if t_max < 0.0 else 1.0
    T = min(abs(t_max), until)
    f = rhs6(MU, sgn)
    s = solve_ivp(f, (0.0, T), np.asarray(y0, dtype=float), method="DOP853", rtol=rtol, atol=atol, dense_output=True)
    tt = np.linspace(0.0, T, int(np.ceil(T / dt)) + 1)
    g = s.sol(tt)[axis] - value
    k = np.nonzero(g[:-1] * g[1:] < 0.0)[0]
    tc = tt[k] + (tt[k + 1] - tt[k]) * g[k] / (g[k] - g[k + 1])
    slopes = np.array([f(0.0, s.sol(t))[axis] for t in tc])
    return tc, slopes


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
