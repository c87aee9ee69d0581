"""Host reference for the thrust-arc kernels (k_indirect_events, k_events_compact) -- CPU only, no library code under test.

Per segment scipy.integrate.solve_ivp(method="DOP853", rtol = atol = 1e-13, events = g) on the 13-dimensional augmented system
(y, q), q' = umag(|lambda_v|), with the oracle's RHS and addtime_reference.umag; the join events and the compaction in numpy, as
include/lto.h defines them.  A second, independent determination of the same roots: scipy.optimize.brentq on
g(oracle.flow_state_costate(y_i, prm, tau, DOP853_ADAPTIVE)).  For LTO_RK4 the same algorithm as the device's, restated in numpy:
`steps` classical RK4 steps of (y, q), the on-state compared after every step, the crossing bracketed by trial steps from the
step's start state.

Fixtures: the nodes of synth.indirect_problem with every node's costates rescaled -- lambda_v to a level around the threshold of
g, lambda_r to a norm that sets how fast |lambda_v| moves.  Only the seeds and scalars below are stored; the searches that found
them ran on the CPU."""
import functools
from collections import namedtuple

import numpy as np

import addtime_reference as A
from lowthrustopt_amd import synth
from lowthrustopt_amd.constants import MU, DU, TU

KEEP = 4                    # events a segment keeps
MIN_SLOPE = 0.1             # |dn/dt| at every fixture root, per TU
MASS = 1000.0

Traj = namedtuple("Traj", "n seed dt lev lam_r p rho thrust")     # lev = (lo, hi): |lambda_v| / threshold per node; dt: a length or (lo, hi)
# name -> trajectories of the case (B = len)
CASES = {
    "one_crossing": [Traj(2, 2, 0.15, (0.7, 1.3), 2.0, 1.0, 1e-2, 0.05)],
    "join_only": [Traj(3, 0, 0.05, (0.6, 1.4), 2.0, 1.0, 1e-2, 0.05)],
    "two_crossings": [Traj(2, 2, 0.6, (1.02, 1.25), 2.0, 1.0, 1e-2, 0.05)],
    "mixed66": [Traj(66, 11, (0.03, 0.06), (0.7, 1.3), 2.0, 1.0, 1e-2, 0.05),
                Traj(66, 12, (0.03, 0.06), (0.7, 1.3), 0.5, 2.0, 1.0, 0.05),
                Traj(66, 13, (0.03, 0.06), (0.7, 1.3), 2.0, 0.0, 1.0, 0.05)],
}
# A segment holding five crossings.  It is 6 TU long, forty times the demo's: the two CPU determinations of its roots differ by
# 3e-11 TU, thirty times the floor of the bar, so it is kept out of CASES (and of e_t) and checked against its own measured error.
EXTRA = {"many_crossings": [Traj(2, 20, 6.0, (0.9, 1.1), 0.3, 1.0, 1e-2, 0.05)]}


def _spec(name):
    return CASES[name] if name in CASES else EXTRA[name]


def prm_tuple(tr):
    return (MU, DU, TU, tr.thrust, MASS, 1.0, tr.p, tr.rho)


def accel_limit(prm):
    return prm[3] / prm[4] / 1e3 * prm[2] ** 2 / prm[1]


def threshold(prm):
    """g = |lambda_v| - threshold; None: p = 0, always on."""
    p = prm[6]
    if p == 0:
        return None
    return 1.0 if p == 1 else p * accel_limit(prm) ** (p - 1.0)


def make_traj(tr):
    """(XC [12 x n], t [n]) of one fixture trajectory."""
    kw = dict(dt_range=tr.dt) if isinstance(tr.dt, tuple) else dict(dt_seg=tr.dt)
    XC, T = synth.indirect_problem(tr.n, 1, seed=tr.seed, **kw)
    XC = np.array(XC[:, :, 0], order="F")
    thr = threshold(prm_tuple(tr)) or 1.0
    rng = np.random.default_rng(tr.seed + 7919)
    lev = rng.uniform(tr.lev[0], tr.lev[1], tr.n)
    for k in range(tr.n):
        XC[9:12, k] *= thr * lev[k] / np.linalg.norm(XC[9:12, k])
        XC[6:9, k] *= tr.lam_r / np.linalg.norm(XC[6:9, k])
    return XC, np.array(T[:, 0])


def case_problem(name):
    """(XC [12 x n x B], T [n x B], [params tuples]) of a case."""
    parts = [make_traj(tr) for tr in _spec(name)]
    XC = np.asfortranarray(np.stack([p[0] for p in parts], axis=2))
    T = np.asfortranarray(np.stack([p[1] for p in parts], axis=1))
    return XC, T, [prm_tuple(tr) for tr in _spec(name)]


def g_of(y, prm):
    return float(np.linalg.norm(y[9:12]) - threshold(prm))


def is_on(y, prm):
    return 1 if threshold(prm) is None else int(g_of(y, prm) > 0.0)


def _umag(y, prm):
    return float(A.umag(np.asarray(y[9:12]).reshape(3, 1), prm[3], prm[6], prm[7], prm[4], prm[1], prm[2])[0])


def rhs13(O, z, prm):
    out = np.empty(13)
    out[:12] = O.rhs_state_costate(z[:12], np.array(prm))
    out[12] = _umag(z, prm)
    return out


def slope(O, y, prm):
    """dn/dt at a state."""
    dy = O.rhs_state_costate(y[:12], np.array(prm))
    return float(np.dot(y[9:12], dy[9:12]) / np.linalg.norm(y[9:12]))


Seg = namedtuple("Seg", "roots q on_s on_e ont slopes")


def _on_time(roots, on_s, ta, tb):
    on, mark, ont = on_s, ta, 0.0
    for r in roots:
        if on:
            ont += r - mark
        else:
            mark = r
        on ^= 1
    return ont + (tb - mark if on else 0.0)


def seg_reference(O, y0, ta, tb, prm, tol=1e-13):
    """One segment by solve_ivp with events."""
    from scipy.integrate import solve_ivp
    z0 = np.append(np.asarray(y0, dtype=np.float64), 0.0)
    ev = None if threshold(prm) is None else (lambda t, z: g_of(z, prm))
    sol = solve_ivp(lambda t, z: rhs13(O, z, prm), (ta, tb), z0, method="DOP853", rtol=tol, atol=tol, events=ev)
    assert sol.success
    roots = [] if ev is None else [float(r) for r in sol.t_events[0]]
    slopes = [] if ev is None else [slope(O, z, prm) for z in sol.y_events[0]]
    on_s, on_e = is_on(z0, prm), is_on(sol.y[:, -1], prm)
    return Seg(roots, float(sol.y[12, -1]), on_s, on_e, _on_time(roots, on_s, ta, tb), slopes)


def roots_brentq(O, y0, ta, prm, roots, tb, half=1e-4):
    """The same roots from the oracle's own flow of the node."""
    from scipy.optimize import brentq

    def f(tau):
        y, rc, _, _ = O.flow_state_costate(y0, np.array(prm), tau - ta, O.DOP853_ADAPTIVE, 0, 1e-13, 1e-13)
        assert rc == 0
        return g_of(y, prm)
    out = []
    for r in roots:
        lo, hi = max(ta + 1e-9, r - half), min(tb, r + half)
        out.append(float(brentq(f, lo, hi, xtol=1e-16, rtol=8.9e-16)))
    return out


def _rk4(O, z, h, prm):
    k1 = rhs13(O, z, prm)
    k2 = rhs13(O, z + 0.5 * h * k1, prm)
    k3 = rhs13(O, z + 0.5 * h * k2, prm)
    k4 = rhs13(O, z + h * k3, prm)
    return z + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)


def seg_reference_rk4(O, y0, ta, tb, prm, steps):
    """One segment the way the device steps it with LTO_RK4."""
    z = np.append(np.asarray(y0, dtype=np.float64), 0.0)
    h = (tb - ta) / steps
    on_s = on = is_on(z, prm)
    roots = []
    for k in range(steps):
        z0, t0 = z, ta + k * h
        z = _rk4(O, z0, h, prm)
        on1 = is_on(z, prm)
        if on1 != on:
            lo, hi, t_hi = 0.0, 1.0, t0 + h
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                if is_on(_rk4(O, z0, mid * h, prm), prm) == on:
                    lo = mid
                else:
                    hi = mid
                t_lo, t_hi = t0 + lo * h, t0 + hi * h
                if not t_hi > np.nextafter(t_lo, np.inf):
                    break
            roots.append(float(t_hi))
            on = on1
    return Seg(roots, float(z[12]), on_s, on, _on_time(roots, on_s, ta, tb), [])


def wave_sum(v):
    """Sum in the order of k_events_compact: lane l adds the entries l, l + 64, .. in turn, then a butterfly over the 64 lanes."""
    v = np.asarray(v, dtype=np.float64)
    part = np.zeros(64)
    for i, x in enumerate(v):
        part[i % 64] += x
    idx = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        part = part + part[idx ^ off]
    return float(part[0])


Arcs = namedtuple("Arcs", "n_events t_event kind on0 dv burn_time dv_seg status")


def compact(segs, t, max_events=64):
    """The trajectory's lists from its segments' records, as k_events_compact defines them."""
    times, kinds, limit, over = [], [], max_events, False
    for i, s in enumerate(segs):
        on = s.on_s
        if len(s.roots) > KEEP:
            over = True
            limit = min(limit, len(times) + KEEP)
        for r in s.roots:
            times.append(r); kinds.append(-1 if on else 1)
            on ^= 1
        if i + 1 < len(segs) and s.on_e != segs[i + 1].on_s:
            times.append(float(t[i + 1])); kinds.append(1 if segs[i + 1].on_s else -1)
    n = len(times)
    te, kd = np.full(max_events, np.nan), np.zeros(max_events, dtype=np.int32)
    m = min(n, limit)
    te[:m] = times[:m]; kd[:m] = kinds[:m]
    dv_seg = np.array([s.q for s in segs])
    status = 1 if (n > max_events or over) else 0
    return Arcs(n, te, kd, segs[0].on_s, wave_sum(dv_seg), wave_sum([s.ont for s in segs]), dv_seg, status)


def traj_segments(O, XC, t, prm, tol=1e-13, rk4_steps=None):
    n = XC.shape[1]
    if rk4_steps:
        return [seg_reference_rk4(O, XC[:, i], t[i], t[i + 1], prm, rk4_steps) for i in range(n - 1)]
    return [seg_reference(O, XC[:, i], t[i], t[i + 1], prm, tol) for i in range(n - 1)]


@functools.lru_cache(maxsize=None)
def case_reference(name, tol=1e-13, rk4_steps=None, max_events=64):
    """[(segments, Arcs)] per trajectory of a case; computed once per process."""
    from oracle import oracle as O
    XC, T, prms = case_problem(name)
    out = []
    for b, prm in enumerate(prms):
        segs = traj_segments(O, XC[:, :, b], T[:, b], prm, tol, rk4_steps)
        out.append((segs, compact(segs, T[:, b], max_events)))
    return out


def tolerances(names=None):
    """(e_t, e_dv) measured on the fixtures (all of CASES unless named): the largest difference between the two CPU determinations
    of any fixture root, and the largest relative difference of the reference dv between rtol = atol = 1e-13 and 1e-12."""
    return _tolerances(tuple(CASES) if names is None else tuple(names))


@functools.lru_cache(maxsize=None)
def _tolerances(names):
    from oracle import oracle as O
    e_t, e_dv = 0.0, 0.0
    for name in names:
        XC, T, prms = case_problem(name)
        fine, coarse = case_reference(name), case_reference(name, 1e-12)
        for b, prm in enumerate(prms):
            segs = fine[b][0]
            for i, s in enumerate(segs):
                if s.roots:
                    r2 = roots_brentq(O, XC[:, i, b], T[i, b], prm, s.roots, T[i + 1, b])
                    e_t = max(e_t, float(np.max(np.abs(np.array(r2) - np.array(s.roots)))))
            e_dv = max(e_dv, abs(fine[b][1].dv - coarse[b][1].dv) / abs(fine[b][1].dv))
    return e_t, e_dv


def bars(names=None):
    """(bar on |t_event - ref| in TU, relative bar on dv)."""
    e_t, e_dv = tolerances(names)
    return max(1e-12, 10.0 * e_t), max(1e-12, 10.0 * e_dv)
