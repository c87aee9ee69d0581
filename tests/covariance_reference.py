"""Host reference for the linear covariance of guided flights (k_guidance_covariance, lto_guidance_covariance_batch)
-- CPU only, no library code under test.

Four determinations of the node covariances P_k of a (trajectory, case), NX = 6 (12 rows) or 7 (14 rows), ND = 2 NX:
  loops           the recursion of include/lto.h as plain Python loops over binary64 scalars, in the header's order: every product
                  and every sum rounded on its own, every dot product from its first product over j = 0, 1, ..; (P + R) formed
                  first.  The device is held to it bit for bit.
  longdouble      the same recursion in numpy.longdouble matrix products.
  differences     P_k = G_0 P0 G_0^T + sum_j G_j R G_j^T with G_0 = d x_k / d x_0 and G_j = d x_k / d e_j from central differences
                  (eps = 1e-6, for 14 rows times X_SCALE) of guided flights: 2 NX (1 + n_upd) flights.  The flights are whoever's:
                  the oracle's (guidance_reference.fly, guidance_mass_reference.fly) or the device's in one call.
  closed form     update_every = 1: rows 0..5 of the arrival state are -A_{n-2}[0:6, :] e_{n-2} whatever came before, so the
                  arrival covariance of (r, v) is A_{n-2}[0:6, :] R A_{n-2}[0:6, :]^T, A the upper left block of the last STM."""
import numpy as np

EPS = 1e-6
NAN = float("nan")


def finite(v):
    return (v - v) == 0.0


def sym_load(a, nx):
    """a[r][c] <- 0.5 * (a[r][c] + a[c][r]) as lists of Python floats."""
    return [[0.5 * (float(a[r][c]) + float(a[c][r])) for c in range(nx)] for r in range(nx)]


def loops(Phi, K, P0, R, every):
    """(P_nodes [nx x nx x n], status) of one (trajectory, case): Phi [nd x nd x S], K [nx x nx x S], P0 and R [nx x nx], in the
    header's arithmetic order.  status 2: a non-finite P0 or R (node 0), Phi_k or applied K_k (node k): NaN from node k + 1 on."""
    nd, S = Phi.shape[0], Phi.shape[2]
    nx = nd // 2
    n = S + 1
    out = np.full((nx, nx, n), NAN)
    P = sym_load(P0, nx)
    Rs = sym_load(R, nx)
    for r in range(nx):
        for c in range(nx):
            out[r, c, 0] = P[r][c]
    if not all(finite(P[r][c]) and finite(Rs[r][c]) for r in range(nx) for c in range(nx)):
        return out, 2
    Z = [[0.0] * nd for _ in range(nd)]
    for r in range(nx):
        for c in range(nx):
            Z[r][c] = P[r][c]
    for k in range(S):
        F = [[float(Phi[r, c, k]) for c in range(nd)] for r in range(nd)]
        upd = every > 0 and k % every == 0
        ok = all(finite(F[r][c]) for r in range(nd) for c in range(nd))
        if upd:
            Kk = [[float(K[r, c, k]) for c in range(nx)] for r in range(nx)]
            ok = ok and all(finite(Kk[r][c]) for r in range(nx) for c in range(nx))
        if not ok:
            return out, 2
        if upd:
            Sm = [[Z[r][c] + Rs[r][c] for c in range(nx)] for r in range(nx)]
            U = [[0.0] * nx for _ in range(nx)]
            V = [[0.0] * nx for _ in range(nx)]
            for r in range(nx):
                for c in range(nx):
                    u = Kk[r][0] * Z[0][c]
                    v = Kk[r][0] * Sm[0][c]
                    for j in range(1, nx):
                        u = u + Kk[r][j] * Z[j][c]
                        v = v + Kk[r][j] * Sm[j][c]
                    U[r][c], V[r][c] = u, v
            for r in range(nx):
                for c in range(nx):
                    l = V[r][0] * Kk[c][0]
                    for j in range(1, nx):
                        l = l + V[r][j] * Kk[c][j]
                    Z[nx + r][c] = U[r][c]
                    Z[c][nx + r] = U[r][c]
                    Z[nx + r][nx + c] = l
        T = [[0.0] * nd for _ in range(nd)]
        for r in range(nd):
            for c in range(nd):
                t = F[r][0] * Z[0][c]
                for j in range(1, nd):
                    t = t + F[r][j] * Z[j][c]
                T[r][c] = t
        W = [[0.0] * nd for _ in range(nd)]
        for r in range(nd):
            for c in range(nd):
                z = T[r][0] * F[c][0]
                for j in range(1, nd):
                    z = z + T[r][j] * F[c][j]
                W[r][c] = z
        Z = [[0.5 * (W[r][c] + W[c][r]) for c in range(nd)] for r in range(nd)]
        for r in range(nx):
            for c in range(nx):
                out[r, c, k + 1] = Z[r][c]
    return out, 0


def recursion_ld(Phi, K, P0, R, every):
    """P_nodes [nx x nx x n] of the same recursion in numpy.longdouble (regular inputs only)."""
    f = np.longdouble
    nd, S = Phi.shape[0], Phi.shape[2]
    nx = nd // 2
    P = np.asarray(P0, dtype=f)
    Rs = np.asarray(R, dtype=f)
    P, Rs = (P + P.T) / 2, (Rs + Rs.T) / 2
    Z = np.zeros((nd, nd), dtype=f)
    Z[:nx, :nx] = P
    out = np.empty((nx, nx, S + 1), dtype=f)
    out[:, :, 0] = P
    for k in range(S):
        F = np.asarray(Phi[:, :, k], dtype=f)
        if every > 0 and k % every == 0:
            Kk = np.asarray(K[:, :, k], dtype=f)
            U = Kk @ Z[:nx, :nx]
            Z[nx:, :nx] = U
            Z[:nx, nx:] = U.T
            Z[nx:, nx:] = Kk @ (Z[:nx, :nx] + Rs) @ Kk.T
        Z = F @ Z @ F.T
        Z = (Z + Z.T) / 2
        out[:, :, k + 1] = Z[:nx, :nx]
    return out


def node_error(P, P_ref):
    """Per node, max |P - P_ref| over that node's largest |P_ref|: [n]."""
    Pr = np.asarray(P_ref, dtype=np.longdouble)
    d = np.max(np.abs(np.asarray(P, dtype=np.longdouble) - Pr), axis=(0, 1))
    return (d / np.max(np.abs(Pr), axis=(0, 1))).astype(np.float64)


def sigma_scaled_error(P, P_ref):
    """max over the elements of |P[i][j] - P_ref[i][j]| / (sigma_i sigma_j), sigma_i = sqrt(P_ref[i][i]), over the trailing axes
    (nodes) of P: [...]."""
    P, Pr = np.asarray(P, dtype=np.float64), np.asarray(P_ref, dtype=np.float64)
    s = np.sqrt(np.einsum("ii...->i...", Pr))
    return np.max(np.abs(P - Pr) / (s[:, None] * s[None, :]), axis=(0, 1))


def n_updates(n, every):
    return (n - 2) // every + 1 if every > 0 else 0


def cd_perturbations(nx, n, every, scale=None, eps=EPS):
    """(dx0 [nx x M], nav [nx x n_upd x M]) of the M = 2 nx (1 + n_upd) flights of the central differences: block 0 perturbs the
    start, block 1 + j the navigation error of update j; within a block +eps and -eps on every row, times scale[row]."""
    nu = n_updates(n, every)
    sc = np.ones(nx) if scale is None else np.asarray(scale, dtype=np.float64)
    M = 2 * nx * (1 + nu)
    dx0 = np.zeros((nx, M), order="F")
    nav = np.zeros((nx, max(nu, 1), M), order="F")[:, :nu]
    for blk in range(1 + nu):
        for i in range(nx):
            for s, sign in enumerate((1.0, -1.0)):
                m = (blk * nx + i) * 2 + s
                if blk == 0:
                    dx0[i, m] = sign * eps * sc[i]
                else:
                    nav[i, blk - 1, m] = sign * eps * sc[i]
    return dx0, np.asfortranarray(nav)


def cd_assemble(nodes, n, every, P0, R, scale=None, eps=EPS):
    """P_nodes [nx x nx x n] from the node states [nx x n x M] of the flights of cd_perturbations: P_k = G_0 P0 G_0^T + sum_j G_j
    R G_j^T, with P0 and R symmetrised as the call does."""
    nx = nodes.shape[0]
    nu = n_updates(n, every)
    sc = np.ones(nx) if scale is None else np.asarray(scale, dtype=np.float64)
    P0s, Rs = 0.5 * (P0 + P0.T), 0.5 * (R + R.T)
    out = np.zeros((nx, nx, n))
    for blk in range(1 + nu):
        G = np.empty((nx, nx, n))                 # G[:, i, k] = d x_k / d (row i)
        for i in range(nx):
            m = (blk * nx + i) * 2
            G[:, i, :] = (nodes[:, :, m] - nodes[:, :, m + 1]) / (2.0 * eps * sc[i])
        C = P0s if blk == 0 else Rs
        for k in range(n):
            out[:, :, k] += G[:, :, k] @ C @ G[:, :, k].T
    return out


def closed_form(Phi, R):
    """The arrival covariance of (r, v) [6 x 6] for update_every = 1: A R A^T, A = rows 0..5 of the upper left block of the last
    STM, in longdouble."""
    nx = Phi.shape[0] // 2
    A = np.asarray(Phi[0:6, 0:nx, -1], dtype=np.longdouble)
    Rs = np.asarray(R, dtype=np.longdouble)
    return A @ ((Rs + Rs.T) / 2) @ A.T


def spd(sig, seed, skew=0.0):
    """A full covariance with the per-row sigmas sig [nx] (each times a factor in 0.5 .. 1.5) and random correlations from
    numpy.random.default_rng(seed); skew > 0 adds an antisymmetric part of that relative size, which the call's symmetrisation has
    to remove again."""
    sig = np.asarray(sig, dtype=np.float64)
    nx = sig.shape[0]
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((nx, 2 * nx))
    C = A @ A.T
    d = 1.0 / np.sqrt(np.diag(C))
    C = C * d[:, None] * d[None, :]
    s = sig * (0.5 + rng.random(nx))
    P = C * s[:, None] * s[None, :]
    P = 0.5 * (P + P.T)
    if skew > 0.0:
        N = rng.standard_normal((nx, nx)) * skew * np.outer(s, s)
        P = P + (N - N.T)
    return np.asfortranarray(P)


def start_sigmas(nx, DU, TU):
    """Per-row sigmas of the size the drivers are used with: 1 km, 1 cm/s and (nx = 7) 1 kg, in DU, DU/TU and kg.  The navigation
    covariances of the tests are a tenth of it.  With them the central differences' own truncation (the costate moves by K eps,
    about 0.1 for eps = 1e-6, and the free final mass answers to that beyond first order) stays inside their bar."""
    return np.array([1.0 / DU] * 3 + [0.01 / 1e3 * TU / DU] * 3 + [1.0] * (nx - 6))
