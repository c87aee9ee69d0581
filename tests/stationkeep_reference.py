"""Independent host reference of the station-keeping calls.  Nothing here comes from the product; MU, the orbits and
their monodromy matrices are passed in by the tests.

  gains    plain Python loops over binary64 scalars in the order include/lto.h states (every product, sum and quotient rounded on
           its own, sums left to right from the first term), so the device is compared bit for bit
  flight   scipy's DOP853 at rtol 1e-13 / atol 1e-14, one solve_ivp per span, or a plain RK4 of a given step count per span; the
           feedback, the dead band, the clip, the execution error and the lost test as the header states them
  law      the Floquet-mode law of a packaged orbit at given phases: manifold_reference's 50-digit eigen pair carried round the
           orbit by its 12-component transport, then the gains loops"""
import collections
import math

import numpy as np
from scipy.integrate import solve_ivp

import manifold_reference as MR

RTOL, ATOL = 1e-13, 1e-14
LOOSE = (1e-12, 1e-13)
TAUS3 = (0.1, 0.35, 0.8)

OMEGA = np.array([[0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
S = np.block([[2.0 * OMEGA, -np.eye(3)], [np.eye(3), np.zeros((3, 3))]])


def variational_matrix(x, MU):
    """A = [[0, I], [U_xx, 2 Omega]] of the CRTBP at the state x."""
    X, Y, Z = x[:3]
    a, b = X + MU, X + MU - 1.0
    r1, r2 = math.sqrt(a * a + Y * Y + Z * Z), math.sqrt(b * b + Y * Y + Z * Z)
    c1, c2 = (1.0 - MU) / r1 ** 3, MU / r2 ** 3
    q1, q2 = 3.0 * (1.0 - MU) / r1 ** 5, 3.0 * MU / r2 ** 5
    qa, qs = q1 * a + q2 * b, q1 + q2
    U = np.array([[1.0 - c1 - c2 + q1 * a * a + q2 * b * b, qa * Y, qa * Z],
                  [qa * Y, 1.0 - c1 - c2 + qs * Y * Y, qs * Y * Z],
                  [qa * Z, qs * Y * Z, -c1 - c2 + qs * Z * Z]])
    return np.block([[np.zeros((3, 3)), np.eye(3)], [U, 2.0 * OMEGA]])


# ------------------------------------------------------------------------------------------------------------------------ gains
def gains_record(vu, vs, sing_tol):
    """(W [6], G [3 x 6], alpha, status) of one (phase, orbit) record, in the order of include/lto.h."""
    vu = [float(v) for v in vu]
    vs = [float(v) for v in vs]
    nanW, nanG = np.full(6, np.nan), np.full((3, 6), np.nan)
    if not all(math.isfinite(v) for v in vu + vs):
        return nanW, nanG, np.nan, 2
    w = [2.0 * vs[1] - vs[3], -2.0 * vs[0] - vs[4], -vs[5], vs[0], vs[1], vs[2]]
    p, ns2, nu2 = w[0] * vu[0], w[0] * w[0], vu[0] * vu[0]
    for i in range(1, 6):
        p = p + w[i] * vu[i]
        ns2 = ns2 + w[i] * w[i]
        nu2 = nu2 + vu[i] * vu[i]
    ns, nu = math.sqrt(ns2), math.sqrt(nu2)
    with np.errstate(all="ignore"):
        W = [float(np.float64(w[i]) / np.float64(p)) for i in range(6)]          # numpy's division: inf / nan instead of raising
        wn2 = W[0] * W[0]
        for i in range(1, 6):
            wn2 = wn2 + W[i] * W[i]
        wv2 = (W[3] * W[3] + W[4] * W[4]) + W[5] * W[5]
        alpha = float(np.sqrt(np.float64(wv2)) / np.sqrt(np.float64(wn2)))
        if abs(p) <= (sing_tol * ns) * nu or not alpha > sing_tol:
            return nanW, nanG, np.nan, 3
        G = np.empty((3, 6))
        for c in range(6):
            for r in range(3):
                G[r, c] = (-(W[3 + r] * W[c])) / wv2
    return np.array(W), G, alpha, 0


def gains(V, sing_tol=1e-8):
    """(W [6 x P x B], G [3 x 6 x P x B], alpha [P x B], status [P x B]) of V [6 x 2 x P x B], record by record."""
    V = np.asarray(V, dtype=float)
    P, B = V.shape[2], V.shape[3]
    W, G = np.empty((6, P, B)), np.empty((3, 6, P, B))
    alpha, status = np.empty((P, B)), np.empty((P, B), dtype=np.int32)
    for b in range(B):
        for j in range(P):
            W[:, j, b], G[:, :, j, b], alpha[j, b], status[j, b] = gains_record(V[:, 0, j, b], V[:, 1, j, b], sing_tol)
    return W, G, alpha, status


# ----------------------------------------------------------------------------------------------------------------------- flight
def rk4(f, w, span, n):
    h = span / n
    for _ in range(n):
        k1 = f(0.0, w)
        k2 = f(0.0, w + 0.5 * h * k1)
        k3 = f(0.0, w + 0.5 * h * k2)
        k4 = f(0.0, w + h * k3)
        w = w + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)
    return w


Run = collections.namedtuple("Run", "x_final dv_total n_burn dev dv_hist dev_final status lost_at cmd")


def flight(MU, X_ref, dt, G, x0, n_rev, nav=None, exe=None, dv_min=0.0, dv_max=0.0, r_lost=0.0, rtol=RTOL, atol=ATOL, rk4_steps=0):
    """One run: X_ref [6 x n_man], dt [n_man], G [3 x 6 x n_man], x0 [6], nav [6 x n_upd] / exe [4 x n_upd] or None.  Returns Run;
    cmd [n_upd] is the commanded |c| before dead band and clip (NaN past the run's end), for vetting thresholds."""
    X_ref, dt, G = np.asarray(X_ref, dtype=float), np.asarray(dt, dtype=float), np.asarray(G, dtype=float)
    n_man = dt.size
    n_upd = n_rev * n_man
    f = MR.rhs6(MU)
    x = np.array(x0, dtype=float)
    dev, hist, cmd = np.full((2, n_upd), np.nan), np.full(n_upd, np.nan), np.full(n_upd, np.nan)
    total, n_burn, status, lost_at = 0.0, 0, 0, -1
    nan6 = np.full(6, np.nan)
    if not np.all(np.isfinite(x)):
        return Run(nan6, np.nan, 0, dev, hist, np.full(2, np.nan), 2, -1, cmd)
    for u in range(n_upd):
        j = u % n_man
        d = x - X_ref[:, j]
        dev[:, u] = np.linalg.norm(d[:3]), np.linalg.norm(d[3:])
        if r_lost > 0.0 and dev[0, u] > r_lost:
            status, lost_at = 1, u
            break
        c = G[:, :, j] @ (d + (nav[:, u] if nav is not None else 0.0))
        m = np.linalg.norm(c)
        cmd[u] = m
        if not np.isfinite(m):
            status = 2
            break
        if m < dv_min:
            hist[u] = 0.0
        else:
            if dv_max > 0.0 and m > dv_max:
                c = c * (dv_max / m)
            if exe is not None:
                c = (1.0 + exe[0, u]) * c + exe[1:4, u]
            a = np.linalg.norm(c)
            if not np.isfinite(a):
                status = 2
                break
            x = x.copy()
            x[3:] += c
            total += a
            n_burn += 1
            hist[u] = a
        if rk4_steps:
            x = rk4(f, x, dt[j], rk4_steps)
        else:
            x = solve_ivp(f, (0.0, dt[j]), x, method="DOP853", rtol=rtol, atol=atol).y[:, -1]
        if not np.all(np.isfinite(x)):
            status = 2
            break
    if status == 2:
        dev[:, u:], hist[u:] = np.nan, np.nan
        return Run(nan6, np.nan, n_burn, dev, hist, np.full(2, np.nan), 2, -1, cmd)
    if status == 1:
        return Run(x, total, n_burn, dev, hist, dev[:, lost_at].copy(), 1, lost_at, cmd)
    d = x - X_ref[:, 0]
    return Run(x, total, n_burn, dev, hist, np.array([np.linalg.norm(d[:3]), np.linalg.norm(d[3:])]), 0, -1, cmd)


# ------------------------------------------------------------------------------------------------------- the tests' shared inputs
_SHARED = {}
Law = collections.namedtuple("Law", "tau X_ref dt G W alpha V lam period")


def spans(taus, period):
    """dt_j = ((tau_{j+1} - tau_j) mod 1) P, the wrap-round span last; one phase: P."""
    t = np.asarray(taus, dtype=float)
    d = np.mod(np.roll(t, -1) - t, 1.0)
    if t.size == 1:
        d[0] = 1.0
    return d * period


def law(orbits, k, taus, MU):
    """The Floquet-mode law of orbit k at the phases taus, all from this reference; computed once per (k, taus)."""
    key = ("law", k, tuple(taus))
    if key not in _SHARED:
        s, P, M = orbits[k]
        lam, X, V = MR.seeds(s, P, M, taus, MU)
        W, G, alpha, status = gains(V[..., None])
        assert np.all(status == 0)
        _SHARED[key] = Law(np.asarray(taus, dtype=float), X[:, 1, :].copy(), spans(taus, P), G[..., 0], W[..., 0], alpha[:, 0], V, lam, P)
    return _SHARED[key]


def draws(n_runs, n_upd, seed, inj=(2.6e-6, 1e-5), nav=(7.8e-7, 3e-6), exe=(0.01, 1e-7)):
    """(x_err [6 x n_runs], nav [6 x n_upd x n_runs], exe [4 x n_upd x n_runs]) in DU and DU/TU: by default about 1 km / 1 cm/s of
    injection error, 0.3 km / 3 mm/s of navigation error, 1 % and 0.1 mm/s of execution error (Earth-Moon units)."""
    rng = np.random.RandomState(seed)
    e = rng.standard_normal((6, n_runs))
    e[:3] *= inj[0]
    e[3:] *= inj[1]
    n = rng.standard_normal((6, n_upd, n_runs))
    n[:3] *= nav[0]
    n[3:] *= nav[1]
    x = rng.standard_normal((4, n_upd, n_runs))
    x[0] *= exe[0]
    x[1:] *= exe[1]
    return e, n, x


def shared_flight(key, *args, **kw):
    """flight(*args, **kw), computed once per key (the tests name their cases)."""
    key = ("flight",) + tuple(key)
    if key not in _SHARED:
        _SHARED[key] = flight(*args, **kw)
    return _SHARED[key]


Case = collections.namedtuple("Case", "X_ref dt G x0 nav exe n_rev n_orb")


def case(orbits, MU, B, n_man, n_rev, errors, per_run, seed=11, random_gain=0.0, scales=None):
    """The inputs of a flight test in the device's layouts: B runs about packaged orbit 1 (per_run: about orbits 1 and 2
    alternating, n_orb = B) at the uneven phases TAUS3 (n_man = 3) or at 0.1 alone (n_man = 1), injected with draws(seed)'s errors;
    errors: nav and exe given.  random_gain > 0 replaces the law by Gaussian matrices of that size (velocity columns; the position
    columns 10 times it).  scales [B] multiplies run b's injection, navigation and execution-bias draws: runs of very different
    sizes, so that a dead band or a clip can lie far from every commanded burn."""
    taus = TAUS3[:n_man]
    n_orb = B if per_run else 1
    laws = [law(orbits, (b % 2) if per_run else 0, taus, MU) for b in range(n_orb)]
    X_ref = np.stack([L.X_ref for L in laws], axis=2)
    dt = np.stack([L.dt for L in laws], axis=1)
    G = np.stack([L.G for L in laws], axis=3)
    if random_gain > 0.0:
        rng = np.random.RandomState(seed + 1)
        G = rng.standard_normal(G.shape) * random_gain
        G[:, :3] *= 10.0
    e, nav, exe = draws(B, n_man * n_rev, seed)
    if scales is not None:
        sc = np.asarray(scales, dtype=float)
        e, nav = e * sc, nav * sc
        exe[1:] *= sc
    x0 = np.stack([laws[b if per_run else 0].X_ref[:, 0] for b in range(B)], axis=1) + e
    return Case(X_ref, dt, G, x0, nav if errors else None, exe if errors else None, n_rev, n_orb)


Batch = collections.namedtuple("Batch", "x_final dv_total n_burn dev dv_hist dev_final status lost_at cmd")


def fly(key, c, MU, **kw):
    """flight() of every run of the Case c, stacked in the device's layouts; computed once per key."""
    key = ("fly",) + tuple(key)
    if key not in _SHARED:
        runs = []
        for b in range(c.x0.shape[1]):
            o = b if c.n_orb > 1 else 0
            runs.append(flight(MU, c.X_ref[:, :, o], c.dt[:, o], c.G[:, :, :, o], c.x0[:, b], c.n_rev,
                               None if c.nav is None else c.nav[:, :, b], None if c.exe is None else c.exe[:, :, b], **kw))
        _SHARED[key] = Batch(*[np.stack([np.asarray(getattr(r, f)) for r in runs], axis=-1) for f in Run._fields])
    return _SHARED[key]
