"""Host restatement of addTimeFinal's steps 2-4 (src/HelperFunctions.jl:196-250 as re-specified in DESIGN 4.12): the natural
cubic spline re-mesh of a densified trajectory onto the new grid, and find_tau's snap of the last node onto the arrival orbit.
Plain numpy; the GPU tests compare lto_indirect_add_time_batch against it."""
import numpy as np


def linrange(a, b, n):
    """Julia's LinRange(a, b, n) in the library's form (1 - tau) a + tau b, tau = k / (n - 1): both ends exact."""
    tau = np.arange(n, dtype=np.float64) / float(n - 1)
    return (1.0 - tau) * a + tau * b


def natural_spline_moments(x, Y):
    """Second derivatives M [rows x n] of the natural cubic spline through (x, Y[r, :]) (M = 0 at both ends)."""
    x = np.asarray(x, dtype=np.float64)
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    n = x.size
    h = np.diff(x)
    M = np.zeros_like(Y)
    if n < 3:
        return M
    A = np.zeros((n - 2, n - 2))
    R = np.zeros((n - 2, Y.shape[0]))
    slope = np.diff(Y, axis=1) / h
    for i in range(1, n - 1):
        A[i - 1, i - 1] = 2.0 * (h[i - 1] + h[i])
        if i > 1:
            A[i - 1, i - 2] = h[i - 1]
        if i < n - 2:
            A[i - 1, i] = h[i]
        R[i - 1] = 6.0 * (slope[:, i] - slope[:, i - 1])
    M[:, 1:-1] = np.linalg.solve(A, R).T
    return M


def natural_spline_eval(x, Y, M, xq):
    """The spline of natural_spline_moments at the points xq: [rows x len(xq)]; at a knot the sample itself."""
    x = np.asarray(x, dtype=np.float64)
    Y = np.atleast_2d(np.asarray(Y, dtype=np.float64))
    xq = np.atleast_1d(np.asarray(xq, dtype=np.float64))
    n = x.size
    out = np.zeros((Y.shape[0], xq.size))
    for k, q in enumerate(xq):
        i = int(np.clip(np.searchsorted(x, q, side="right") - 1, 0, n - 2))
        if q == x[i]:
            out[:, k] = Y[:, i]
            continue
        if q == x[i + 1]:
            out[:, k] = Y[:, i + 1]
            continue
        h = x[i + 1] - x[i]
        a, b = x[i + 1] - q, q - x[i]
        out[:, k] = (M[:, i] * a ** 3 + M[:, i + 1] * b ** 3) / (6.0 * h) + (Y[:, i] - M[:, i] * h * h / 6.0) * a / h + \
            (Y[:, i + 1] - M[:, i + 1] * h * h / 6.0) * b / h
    return out


def natural_spline(x, Y, xq):
    return natural_spline_eval(x, Y, natural_spline_moments(x, Y), xq)


def remesh(XC_dense, t_dense, n):
    """Step 3: each row's natural spline through (t_dense, XC_dense[r]) at LinRange(t_dense[0], t_dense[-1], n).
    Returns (XC_new [rows x n], t_new [n])."""
    t_new = linrange(t_dense[0], t_dense[-1], n)
    return natural_spline(t_dense, XC_dense, t_new), t_new


def find_tau_from_samples(S, x):
    """find_tau's choice given the table's spline at the 1001 candidates, S [6 x 1001]: the first j of the smallest
    |S[:, j] - x|_2 (tau_trial[d .== minimum(d)][1]).  Returns (j, d)."""
    d = np.sqrt(np.sum((np.asarray(S)[:6] - np.asarray(x)[:6, None]) ** 2, axis=0))
    j = int(np.flatnonzero(d == d.min())[0])
    return j, d


def find_tau(Xf_times, Xf_states, x):
    """Step 4: tau* = j / 1000 and s(tau*) for the arrival table (Xf_times in [0, 1], Xf_states [6 x nf])."""
    taus = np.arange(1001) / 1000.0
    S = natural_spline(Xf_times, np.asarray(Xf_states)[:6], taus)
    j, _ = find_tau_from_samples(S, x)
    return taus[j], S[:, j]


def extended(XC, t, dt):
    """Step 1: a copy of XC with its end costates zeroed and a tail node at t[-1] + dt (the node's value is never used)."""
    XC = np.array(XC, dtype=np.float64, order="F")
    XC[6:12, -1] = 0.0
    XCe = np.asfortranarray(np.hstack([XC, XC[:, -1:]]))
    te = np.append(np.asarray(t, dtype=np.float64), t[-1] + dt)
    return XCe, te


def umag(lam_v, thrustLimit, p, rho, mass, DU, TU):
    """Magnitude of the control law's thrust acceleration (controlLaw_cart, indirect.jl:389-440, before the conversion to N)."""
    aL = thrustLimit / mass / 1e3 * TU ** 2 / DU
    n = np.linalg.norm(np.asarray(lam_v, dtype=np.float64), axis=0)
    with np.errstate(all="ignore"):
        if p == 0:
            u = np.full_like(n, aL)
        elif p == 1:
            u = 0.5 * (1.0 + np.tanh((n - 1.0) / (2.0 * rho))) * aL
        else:
            u = np.minimum((n / p) ** (1.0 / (p - 1.0)), aL)
    return np.where(np.isnan(u), 0.0, u)


def dense_cost(XC_dense, t_dense, thrustLimit, p, rho, mass, DU, TU):
    """Trapezoid of umag over a dense output, DU/TU."""
    u = umag(np.asarray(XC_dense)[9:12], thrustLimit, p, rho, mass, DU, TU)
    t = np.asarray(t_dense, dtype=np.float64)
    return float(np.sum(np.diff(t) * (u[1:] + u[:-1]) / 2.0))
