"""Independent host reference of the targeted periodic-orbit corrector: the 3 x 3 Newton rule -- unknowns (x0, z0, vy0),
residual (vx, vz, q - q*) at the first return to y = 0, q the Jacobi constant of the start or the period 2 t_c -- in numpy on
scipy's DOP853 with a terminal event on y (halo_reference.half_flight), and the march with the secant predictor in the target value.
Nothing here comes from the product; MU and the seeds are passed in by the tests."""
import collections

import numpy as np

import halo_reference as HR

JACOBI, PERIOD = 0, 1
RTOL, ATOL = HR.RTOL, HR.ATOL
LOOSE = (1e-11, 1e-12)                      # the second pair of tolerances: the reference's own spread is measured between the two

Targeted = collections.namedtuple("Targeted", "state period jacobi resid iterations history status")


def jacobi_row(x0, z0, vy0, MU):
    """dC / d(x0, z0, vy0) at (x0, 0, z0, 0, vy0, 0)."""
    a, b = x0 + MU, x0 + MU - 1.0
    r1, r2 = np.sqrt(a * a + z0 * z0), np.sqrt(b * b + z0 * z0)
    return np.array([2.0 * x0 - 2.0 * (1.0 - MU) * a / r1 ** 3 - 2.0 * MU * b / r2 ** 3,
                     -2.0 * z0 * ((1.0 - MU) / r1 ** 3 + MU / r2 ** 3),
                     -2.0 * vy0])


def system(state, qstar, what, planar, MU, t_max=10.0, rtol=RTOL, atol=ATOL):
    """(r, J, t_c) of one flight from state = (x0, 0, z0, 0, vy0, 0): the residual and the Jacobian in the unknowns (x0, z0, vy0),
    or (x0, vy0) when planar; None without a crossing before t_max."""
    fl = HR.half_flight(state, MU, t_max, rtol, atol)
    if fl is None:
        return None
    tc, xc, Phi, f = fl
    cols = [0, 4] if planar else [0, 2, 4]
    rows = [3] if planar else [3, 5]
    Jv = Phi[np.ix_(rows, cols)] - np.outer(f[rows], Phi[1, cols]) / f[1]
    if what == JACOBI:
        q = HR.jacobi(state, MU)
        row = jacobi_row(state[0], state[2], state[4], MU)
        Jq = row[[0, 2]] if planar else row
    else:
        q = 2.0 * tc
        Jq = -2.0 * Phi[1, cols] / f[1]
    r = np.concatenate([xc[rows], [q - qstar]])
    return r, np.vstack([Jv, Jq]), tc


def singularity(J):
    """|det J| / the product of J's row 2-norms (Hadamard: <= 1)."""
    return abs(np.linalg.det(J)) / np.prod(np.linalg.norm(J, axis=1))


def target_correct(seed, qstar, what, planar, MU, tol=1e-12, max_iter=15, t_max=10.0, sing_tol=1e-12, rtol=RTOL, atol=ATOL):
    """The targeted corrector: status 0 converged, 1 max_iter reached, 2 unusable, 3 singular step."""
    x0, z0, vy0 = float(seed[0]), float(seed[2]), float(seed[4])
    nan6 = np.full(6, np.nan)
    hist, it = [], 0
    if (not np.isfinite(x0 + z0 + vy0 + qstar) or vy0 == 0.0 or (planar and z0 != 0.0) or (what == PERIOD and not qstar > 0.0)):
        return Targeted(nan6, np.nan, np.nan, np.nan, 0, hist, 2)
    while True:
        state = np.array([x0, 0.0, z0, 0.0, vy0, 0.0])
        sysm = system(state, qstar, what, planar, MU, t_max, rtol, atol)
        if sysm is None:
            return Targeted(nan6, np.nan, np.nan, np.nan, it, hist, 2)
        r, J, tc = sysm
        res = np.abs(r).max()
        hist.append(res)
        if res < tol or it >= max_iter:
            return Targeted(state, 2.0 * tc, HR.jacobi(state, MU), res, it, hist, 0 if res < tol else 1)
        det = np.linalg.det(J)
        if not np.isfinite(det) or abs(det) <= sing_tol * np.prod(np.linalg.norm(J, axis=1)):
            return Targeted(nan6, np.nan, np.nan, np.nan, it, hist, 3)
        d = np.linalg.solve(J, r)
        if planar:
            x0, vy0 = x0 - d[0], vy0 - d[1]
        else:
            x0, z0, vy0 = x0 - d[0], z0 - d[1], vy0 - d[2]
        it += 1


def predictor(s1, s2, q, q1, q2):
    """The start of member k >= 2 from the last two members s1 = s_(k-1), s2 = s_(k-2) and their targets: s1 + (s1 - s2) w with
    w = (q - q1) / (q1 - q2), each operation rounded once; s1 itself where q1 = q2."""
    s1, s2 = np.asarray(s1, dtype=float), np.asarray(s2, dtype=float)
    if q1 == q2:
        return s1.copy()
    w = (q - q1) / (q1 - q2)
    return s1 + (s1 - s2) * w


def march(seed, targets, what, planar, MU, **kw):
    """Members k = 0 .. K - 1 one after another: member 0 from the seed, member 1 from member 0, member k >= 2 from the predictor.
    A member of status 2 or 3 ends the march: the rest is NaN with status 2."""
    members = []
    for k, q in enumerate(targets):
        if members and members[-1].status >= 2:
            members.append(Targeted(np.full(6, np.nan), np.nan, np.nan, np.nan, 0, [], 2))
            continue
        if k == 0:
            start = np.asarray(seed, dtype=float)
        elif k == 1:
            start = members[0].state
        else:
            start = predictor(members[-1].state, members[-2].state, q, targets[k - 1], targets[k - 2])
        members.append(target_correct(start, q, what, planar, MU, **kw))
    return members


def planar_perturbed(seed, k):
    """HR.perturbed kept in the plane."""
    s = HR.perturbed(seed, k)
    s[2] = 0.0
    return s


# The targets of the GPU tests (tests/test_halo_target_gpu.py), as offsets from the base orbit's own C or P, in the order the 17
# seeds of a batch cycle through them; vetted on the host (tests/test_halo_target_host.py).  No period target below the L2 Lyapunov
# family's minimum: the L2 seeds only go up in period.
HALO_DC = (1e-4, -1e-3, 5e-3)
HALO_DP = (1e-3, -1e-2)
PLANAR_DC = (-1e-3, -5e-3)
PLANAR_DP = {1: (1e-2, -1e-2), 2: (1e-2,)}
C_COMMON = 3.15                             # the Jacobi constant of the L1 / L2 Lyapunov pair of the marches


# The bounds the device is held to against this reference, (state, period) per case class (planar, what): ten times this
# reference's own spread between (1e-13, 1e-14) and LOOSE over the class's cases, rounded up to a power of ten.  The spreads
# (tests/test_halo_target_host.py holds them to a tenth of the bound):
#   3-D    Jacobi   state 1.5e-13   period 4.1e-13          planar Jacobi   state 1.0e-14   period 1.6e-12
#   3-D    period   state 8.5e-14   period 2.0e-14          planar period   state 2.4e-12   period 1.6e-13
BOUNDS = {(False, JACOBI): (1e-11, 1e-11), (False, PERIOD): (1e-12, 1e-12),
          (True, JACOBI): (1e-12, 1e-10), (True, PERIOD): (1e-10, 1e-11)}
# Newton steps of this reference the host test allows per class: the issue's counts + 2
STEPS = {(False, JACOBI): 6, (False, PERIOD): 5, (True, JACOBI): 10, (True, PERIOD): 9}


def cases(planar, what, bases, MU, n=17):
    """The n (seed [6], target) pairs of one GPU batch.  bases: two converged orbits as (state, period) -- 3-D: the packaged halo
    orbits corrected holding x0; planar: the Lyapunov orbits at L1 and L2.  Case k starts from base k % 2 (planar period targets:
    from L1 for k >= 2), itself for k < 2 and a perturbed copy after that, and asks for that base's own C or P plus an offset from
    the lists above (planar Jacobi targets also take C_COMMON in turn)."""
    out = []
    for k in range(n):
        # Planar period targets: the L2 orbit itself, no perturbed copy of it.  The L2 Lyapunov family's period has its minimum
        # (3.3732) close by, and from copies moved by 1e-3 in vy0 this reference needs 6 to 12 steps or wanders off (4 of 8 did).
        which = 0 if (planar and what == PERIOD and k >= 2) else k % 2
        state, period = bases[which]
        state = np.asarray(state, dtype=float)
        if planar:
            seed = state.copy() if k < 2 else planar_perturbed(state, k)
        else:
            seed = state.copy() if k < 2 else HR.perturbed(state, k)
        if what == JACOBI:
            offs = PLANAR_DC + (None,) if planar else HALO_DC
            off = offs[(k // 2) % len(offs)]
            out.append((seed, C_COMMON if off is None else HR.jacobi(state, MU) + off))
        else:
            if planar:                      # L1: P - 1e-2 for k = 2, 6, 10, 14, P + 1e-2 otherwise (copies 11, 13 and 16 take 12
                off = PLANAR_DP[1 + which][1 if k % 4 == 2 else 0]         # steps or more towards P - 1e-2 in this reference)
            else:
                off = HALO_DP[(k // 2) % len(HALO_DP)]
            out.append((seed, period + off))
    return out

