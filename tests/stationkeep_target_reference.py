"""Independent host reference of the target-point station-keeping calls.  Nothing here comes from the product; MU,
the orbits and the weights are passed in by the tests.

  stm      Phi(t_j + h_k P, t_j) by scipy's DOP853 at rtol 1e-13 / atol 1e-14: a coast of the six-component state over tau_j P
           (manifold_reference.rhs6), then one solve_ivp per target span on the 42-component system (halo_reference.rhs42), Phi
           carried from one span into the next; or a plain RK4 of a given step count per span, the coast counting as one
  gains    plain Python loops over binary64 scalars in the order include/lto.h states (every product, sum, difference and quotient
           rounded on its own, math.sqrt), so the device is compared bit for bit
  law      the target-point law of a packaged orbit at given phases from those two"""
import collections
import math

import numpy as np
from scipy.integrate import solve_ivp

import halo_reference as HR
import manifold_reference as MR
import stationkeep_reference as SR

RTOL, ATOL = 1e-13, 1e-14
LOOSE = (1e-12, 1e-13)
TAUS3 = SR.TAUS3
TAUS4 = (0.0, 0.25, 0.5, 0.75)
HORIZONS = (0.5, 1.0)
Q = 1e-2


# -------------------------------------------------------------------------------------------------------------------------- STMs
def stm(state0, period, tau, horizons, MU, rtol=RTOL, atol=ATOL, rk4_steps=0):
    """(X [6], Phi [6 x 6 x K], X_tgt [6 x K]) of one (phase, orbit) record."""
    x = np.array(state0, dtype=float)
    coast = tau * period
    if coast > 0.0:
        if rk4_steps:
            x = SR.rk4(MR.rhs6(MU), x, coast, rk4_steps)
        else:
            x = solve_ivp(MR.rhs6(MU), (0.0, coast), x, method="DOP853", rtol=rtol, atol=atol).y[:, -1]
    K = len(horizons)
    Phi, Xt = np.empty((6, 6, K)), np.empty((6, K))
    w = HR.start42(x)
    f = HR.rhs42(MU)
    hprev = 0.0
    for k, h in enumerate(horizons):
        span = (h - hprev) * period
        hprev = h
        if rk4_steps:
            w = SR.rk4(f, w, span, rk4_steps)
        else:
            w = solve_ivp(f, (0.0, span), w, method="DOP853", rtol=rtol, atol=atol).y[:, -1]
        Xt[:, k] = w[:6]
        Phi[:, :, k] = w[6:].reshape(6, 6)
    return x, Phi, Xt


_SHARED = {}
Stms = collections.namedtuple("Stms", "X Phi X_tgt")


def stms(orbits, ks, taus, horizons, MU, rtol=RTOL, atol=ATOL, rk4_steps=0):
    """stm() of the packaged orbits ks at the phases taus in the device's layouts: X [6 x P x B], Phi [6 x 6 x K x P x B], X_tgt [6
    x K x P x B].  Every record is computed once per (orbit, phase, horizons, tolerance)."""
    P, K, B = len(taus), len(horizons), len(ks)
    X, Phi, Xt = np.empty((6, P, B)), np.empty((6, 6, K, P, B)), np.empty((6, K, P, B))
    for b, k in enumerate(ks):
        for j, tau in enumerate(taus):
            key = ("stm", k, tau, tuple(horizons), rtol, rk4_steps)
            if key not in _SHARED:
                s, per, _ = orbits[k]
                _SHARED[key] = stm(s, per, tau, horizons, MU, rtol, atol, rk4_steps)
            X[:, j, b], Phi[:, :, :, j, b], Xt[:, :, j, b] = _SHARED[key]
    return Stms(X, Phi, Xt)


# ------------------------------------------------------------------------------------------------------------------------- gains
def _div(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))            # numpy's division: inf / nan instead of raising


def _sqrt(a):
    return math.sqrt(a) if a >= 0.0 else float("nan")          # a NaN compares False: NaN


def gains_record(Phi, q, r, sing_tol):
    """(G [3 x 6], pivot, status) of one record Phi [6 x 6 x K], in the order of include/lto.h."""
    Phi = np.asarray(Phi, dtype=float)
    K = Phi.shape[2]
    nanG = np.full((3, 6), np.nan)
    if not np.all(np.isfinite(Phi)):
        return nanG, np.nan, 2
    n = [[0.0] * 6 for _ in range(3)]
    h = [[0.0] * 3 for _ in range(3)]
    for k in range(K):
        T = [[float(Phi[m, c, k]) for c in range(6)] for m in range(3)]
        rk = float(r[k])
        for i in range(3):
            for c in range(6):
                s = T[0][3 + i] * T[0][c]
                s = s + T[1][3 + i] * T[1][c]
                s = s + T[2][3 + i] * T[2][c]
                t = rk * s
                n[i][c] = t if k == 0 else n[i][c] + t
            for j in range(i + 1):
                s = T[0][3 + i] * T[0][3 + j]
                s = s + T[1][3 + i] * T[1][3 + j]
                s = s + T[2][3 + i] * T[2][3 + j]
                t = rk * s
                h[i][j] = t if k == 0 else h[i][j] + t
    q = float(q)
    h00, h10, h11, h20, h21, h22 = q + h[0][0], h[1][0], q + h[1][1], h[2][0], h[2][1], q + h[2][2]
    hmax = max(max(h00, h11), h22)
    lim = sing_tol * hmax
    d0 = h00
    l00 = _sqrt(d0)
    l10, l20 = _div(h10, l00), _div(h20, l00)
    d1 = h11 - l10 * l10
    l11 = _sqrt(d1)
    l21 = _div(h21 - l20 * l10, l11)
    d2 = (h22 - l20 * l20) - l21 * l21
    l22 = _sqrt(d2)
    if not d0 > lim or not d1 > lim or not d2 > lim:
        return nanG, np.nan, 3
    G = np.empty((3, 6))
    for c in range(6):
        z0 = n[0][c] / l00
        z1 = (n[1][c] - l10 * z0) / l11
        z2 = ((n[2][c] - l20 * z0) - l21 * z1) / l22
        x2 = z2 / l22
        x1 = (z1 - l21 * x2) / l11
        x0 = ((z0 - l10 * x1) - l20 * x2) / l00
        G[0, c], G[1, c], G[2, c] = -x0, -x1, -x2
    return G, min(min(d0, d1), d2) / hmax, 0


def gains(Phi, q, r, sing_tol=1e-12):
    """(G [3 x 6 x ...], pivot [...], status [...]) of Phi [6 x 6 x K x ...], record by record."""
    Phi = np.asarray(Phi, dtype=float)
    tail = Phi.shape[3:]
    flat = Phi.reshape(6, 6, Phi.shape[2], -1, order="F")
    n = flat.shape[3]
    G, pivot, status = np.empty((3, 6, n)), np.empty(n), np.empty(n, dtype=np.int32)
    for g in range(n):
        G[:, :, g], pivot[g], status[g] = gains_record(flat[:, :, :, g], q, r, sing_tol)
    return G.reshape((3, 6) + tail, order="F"), pivot.reshape(tail, order="F"), status.reshape(tail, order="F")


def normal_matrices(Phi, q, r):
    """(H [3 x 3], N [3 x 6]) of one record by numpy, for checking the loops."""
    H, N = q * np.eye(3), np.zeros((3, 6))
    for k in range(Phi.shape[2]):
        T = Phi[:3, :, k]
        H = H + r[k] * T[:, 3:].T @ T[:, 3:]
        N = N + r[k] * T[:, 3:].T @ T
    return H, N


def cost(Phi, q, r, dx, dv):
    """J = q |dv|^2 + sum_k r_k |A_k p + B_k (e + dv)|^2."""
    J = q * float(dv @ dv)
    for k in range(Phi.shape[2]):
        m = Phi[:3, :3, k] @ dx[:3] + Phi[:3, 3:, k] @ (dx[3:] + dv)
        J += r[k] * float(m @ m)
    return J


# --------------------------------------------------------------------------------------------------------------------------- law
Law = collections.namedtuple("Law", "tau X_ref dt G Phi pivot period")


def law(orbits, k, taus, MU, horizons=HORIZONS, q=Q, r=None, rtol=RTOL, atol=ATOL):
    """The target-point law of packaged orbit k at the phases taus, all from this reference; computed once per argument set."""
    r = tuple([1.0] * len(horizons) if r is None else r)
    key = ("law", k, tuple(taus), tuple(horizons), q, r, rtol)
    if key not in _SHARED:
        s = stms(orbits, [k], taus, horizons, MU, rtol, atol)
        G, pivot, status = gains(s.Phi[..., 0], q, r)
        assert np.all(status == 0)
        per = orbits[k][1]
        _SHARED[key] = Law(np.asarray(taus, dtype=float), s.X[:, :, 0].copy(), SR.spans(taus, per), G, s.Phi[..., 0], pivot, per)
    return _SHARED[key]


def case(orbits, MU, B, n_rev, errors, per_run, seed=11, taus=TAUS3):
    """stationkeep_reference.case with the target-point law in place of the Floquet-mode law: B runs about packaged orbit 1
    (per_run: about orbits 1 and 2 alternating), the same draws."""
    n_orb = B if per_run else 1
    laws = [law(orbits, (b % 2) if per_run else 0, taus, MU) for b in range(n_orb)]
    X_ref = np.stack([L.X_ref for L in laws], axis=2)
    dt = np.stack([L.dt for L in laws], axis=1)
    G = np.stack([L.G for L in laws], axis=3)
    e, nav, exe = SR.draws(B, len(taus) * n_rev, seed)
    x0 = np.stack([laws[b if per_run else 0].X_ref[:, 0] for b in range(B)], axis=1) + e
    return SR.Case(X_ref, dt, G, x0, nav if errors else None, exe if errors else None, n_rev, n_orb)
