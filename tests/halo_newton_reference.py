"""One iteration of the three periodic-orbit correctors, restated on the independent references: what one
pass of the device loops of lto_halo_correct_batch, lto_halo_target_batch and lto_halo_arclength_batch decides from one iterate
u = (x0, z0, vy0) -- the residual vector and its largest component, the Jacobian, the Newton step d, the singularity measure
|det| / prod |row|_2, the period 2 t_c and, for the arclength kind, the tangent, det and t_new . t_row -- from
halo_reference.half_flight, halo_target_reference.system / singularity and halo_arclength_reference.system / tangent.  Every
function takes (rtol, atol), so that the reference's own spread can be taken between two pairs of tolerances; replay() does that for
a sequence of iterates the device produced and returns the per-step bound the device's step is held to.  Nothing here comes from the
product; MU and the seeds are passed in by the tests.

The cases of tests/test_halo_newton_steps_gpu.py are defined here too (families), and vetted by tests/test_halo_newton_host.py."""
import collections

import numpy as np

import halo_reference as HR
import halo_target_reference as TR
import halo_arclength_reference as AR

TIGHT = (HR.RTOL, HR.ATOL)
LOOSE = (10.0 * HR.RTOL, 10.0 * HR.ATOL)    # the pair ten times looser: the reference's own spread is taken between the two
RES_BOUND = 1e-11                           # what the suite holds a device residual to against this reference
COUNT_CAP = 1e-4                            # a step is counted where its bound is at most this fraction of |d|_inf
TOL, MAX_ITER = 1e-12, 15

CORRECT, TARGET, ARCLENGTH = "correct", "target", "arclength"

# One record's problem.  u0: the first iterate.  correct: mode.  target: qstar, what, planar.  arclength: u_prev, t_row (dir0 where
# orient), ds, planar, orient (the seed's own correction: ds = 0 and the row vector is the first flight's tangent towards t_row).
Problem = collections.namedtuple("Problem", "kind u0 mode qstar what planar u_prev t_row ds orient", defaults=(None,) * 8)
# One pass.  r, J in the kind's own unknowns; d [3] in (x0, z0, vy0) with zeros in what is held; sing: |det| / prod |row|_2 (the planar
# form of the corrector: |J|, which the kernel only compares with 0); t_row: the row vector used; t_raw, t_new, det, dots: arclength.
Pass = collections.namedtuple("Pass", "r res J d sing period jacobi jinv t_row t_raw t_new det dots", defaults=(None,) * 5)
Step = collections.namedtuple("Step", "res d bound counted spread_res spread_d jinv ref loose")
Run = collections.namedtuple("Run", "iterates history iterations status period")

_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _state(u):
    return np.array([u[0], 0.0, u[1], 0.0, u[2], 0.0])


def _key(u):
    return tuple(float(v) for v in u)


def half_flight(u, MU, pair, t_max=10.0):
    """halo_reference.half_flight from (x0, 0, z0, 0, vy0, 0), one flight per (start, tolerances)."""
    return _cached(("flight", _key(u), MU, pair, t_max), lambda: HR.half_flight(_state(u), MU, t_max, pair[0], pair[1]))


def _full(d, cols):
    out = np.zeros(3)
    out[list(cols)] = d
    return out


def correct_pass(u, mode, MU, pair=TIGHT, t_max=10.0, mut=None):
    """One pass of k_halo_correct's loop from u; None without a crossing."""
    fl = half_flight(u, MU, pair, t_max)
    if fl is None:
        return None
    tc, xc, Phi, f = fl
    mut = mut or {}
    rows = [3] if mode == HR.PLANAR else [3, 5]
    cols = [4] if mode == HR.PLANAR else ([0, 4] if mode == HR.HOLD_Z0 else [2, 4])
    J = (Phi[np.ix_(rows, cols)] - np.outer(f[rows], Phi[1, cols]) / f[1] * mut.get("time", 1.0)) * mut.get("J", 1.0)
    r = xc[rows]
    d = np.linalg.solve(J, r)
    sing = abs(J[0, 0]) if mode == HR.PLANAR else TR.singularity(J)
    return Pass(r, np.abs(r).max(), J, _full(d, [c // 2 for c in cols]), sing, 2.0 * tc, HR.jacobi(_state(u), MU),
                np.abs(np.linalg.inv(J)).sum(axis=1).max())


def target_pass(u, qstar, what, planar, MU, pair=TIGHT, t_max=10.0, mut=None):
    """One pass of k_halo_target's loop from u towards q* (halo_target_reference.system); None without a crossing."""
    def make():
        return TR.system(_state(u), qstar, what, planar, MU, t_max, pair[0], pair[1])
    sysm = _cached(("flight", _key(u), MU, pair, t_max, "target", qstar, what, planar), make)
    if sysm is None:
        return None
    r, J, tc = sysm
    mut = mut or {}
    J = J * mut.get("J", 1.0)
    if what == TR.PERIOD:
        J[-1] = J[-1] * mut.get("period_row", 1.0)
    d = np.linalg.solve(J, r)
    return Pass(r, np.abs(r).max(), J, _full(d, [0, 2] if planar else [0, 1, 2]), TR.singularity(J), 2.0 * tc, HR.jacobi(_state(u), MU),
                np.abs(np.linalg.inv(J)).sum(axis=1).max())


def rotated(t, angle):
    """t turned by `angle` towards the unit vector across it that lies nearest the vy0 axis."""
    t = np.asarray(t, dtype=float)
    e = np.array([0.0, 0.0, 1.0]) - t[2] * t / (t @ t)
    e *= np.linalg.norm(t) / np.linalg.norm(e)
    return np.cos(angle) * t + np.sin(angle) * e


def arclength_pass(u, u_prev, t_row, ds, planar, MU, pair=TIGHT, t_max=10.0, orient=False, mut=None):
    """One pass of k_halo_arclength's inner loop from u, the member being the step from u_prev along t_row by ds.  orient: t_row is
    the caller's dir0 and the row vector is this flight's tangent with the sign that makes its product with dir0 positive (the first
    pass of the seed's own correction).  None without a crossing or without a tangent."""
    def make():
        return AR.system(np.asarray(u, dtype=float), planar, MU, t_max, pair[0], pair[1])
    sysm = _cached(("flight", _key(u), MU, pair, t_max, "arclength", planar), make)
    if sysm is None:
        return None
    F, DF, tc = sysm
    t_row = np.asarray(t_row, dtype=float)
    if orient:
        tg = AR.tangent(DF, t_row)
        if tg is None:
            return None
        t_row = tg[0]
    tg = AR.tangent(DF, t_row)
    if tg is None:
        return None
    t_new, det, _ = tg
    c = np.cross(DF[0], DF[1])
    u_pred = np.asarray(u_prev, dtype=float) + ds * t_row
    r = np.array([F[0], F[1], float(t_row @ (np.asarray(u, dtype=float) - u_pred))])
    mut = mut or {}
    J = np.vstack([DF, rotated(t_row, mut["t_row_rot"]) if "t_row_rot" in mut else t_row]) * mut.get("J", 1.0)
    d = np.linalg.solve(J, r)
    res = max(abs(r[0]), abs(r[2])) if planar else np.abs(r).max()
    sing = abs(np.linalg.det(J)) / np.prod(np.linalg.norm(J, axis=1))
    return Pass(r, res, J, d, sing, 2.0 * tc, HR.jacobi(_state(u), MU), np.abs(np.linalg.inv(J)).sum(axis=1).max(), t_row,
                c / np.linalg.norm(c), t_new, det, float(t_new @ t_row))


def one_pass(p, u, MU, pair=TIGHT, t_row=None, mut=None, t_max=10.0):
    """The pass of problem p's kind from iterate u.  t_row: the arclength kind's row vector once the first pass has made it."""
    if p.kind == CORRECT:
        return correct_pass(u, p.mode, MU, pair, t_max, mut)
    if p.kind == TARGET:
        return target_pass(u, p.qstar, p.what, p.planar, MU, pair, t_max, mut)
    if p.orient:
        if t_row is None:
            return arclength_pass(u, p.u_prev, p.t_row, 0.0, p.planar, MU, pair, t_max, True, mut)
        return arclength_pass(u, p.u_prev, t_row, 0.0, p.planar, MU, pair, t_max, False, mut)
    return arclength_pass(u, p.u_prev, p.t_row, p.ds, p.planar, MU, pair, t_max, False, mut)


def first_iterate(p):
    """The loop's first iterate: the seed, or the arclength predictor u_prev + ds t_row (product and sum rounded one by one)."""
    if p.kind == ARCLENGTH and not p.orient:
        return np.asarray(p.u_prev, dtype=float) + p.ds * np.asarray(p.t_row, dtype=float)
    return np.asarray(p.u0, dtype=float)


def newton(p, MU, pair=TIGHT, mut=None, tol=TOL, max_iter=MAX_ITER, t_max=10.0):
    """The whole loop by this restatement (mut: a deliberately wrong Jacobian, for the tests of the tests): the iterates u_0 .. u_K,
    the history, and status 0 converged, 1 max_iter reached, 2 no crossing."""
    u, t_row = first_iterate(p), None
    its, hist = [u.copy()], []
    while True:
        ps = one_pass(p, u, MU, pair, t_row, mut, t_max)
        if ps is None:
            return Run(its, hist, len(hist), 2, np.nan)
        t_row = ps.t_row
        hist.append(ps.res)
        if ps.res < tol or len(hist) - 1 >= max_iter:
            return Run(its, hist, len(hist) - 1, 0 if ps.res < tol else 1, ps.period)
        u = u - ps.d
        its.append(u.copy())


def replay(p, iterates, MU, res_bound=RES_BOUND, pairs=(TIGHT, LOOSE), d_extra=0.0, t_max=10.0):
    """Per iterate u_k of a loop that someone else ran (the device; a mutated newton()): the reference's res_k and d_k from u_k at
    pairs[0], their spread against pairs[1], the bound the step u_(k+1) - u_k + d_k is held to,
        |J^-1|_inf res_bound + 10 |d_k(pairs[0]) - d_k(pairs[1])|_inf + d_extra,
    and whether the step is counted (bound <= COUNT_CAP |d_k|_inf).  d_extra: RK4's own truncation error in d."""
    out, rows = [], [None, None]
    for u in iterates:
        a, b = (one_pass(p, u, MU, pair, rows[i], None, t_max) for i, pair in enumerate(pairs))
        rows = [a.t_row, b.t_row]
        s_res, s_d = abs(a.res - b.res), np.abs(a.d - b.d).max()
        bound = a.jinv * res_bound + 10.0 * s_d + d_extra
        out.append(Step(a.res, a.d, bound, bool(bound <= COUNT_CAP * np.abs(a.d).max()), s_res, s_d, a.jinv, a, b))
    return out


# ---------------------------------------------------------------------------- the cases of the GPU tests, vetted on the host
B = 9                                       # one full wavefront of 8 groups and one group in a second
REPLAYED = (0, 3, 7, 8)                     # the records replayed against this reference: rough seeds all
NEAR, NAN_SEED, STILL = 1, 2, 5             # a nearly converged record, a NaN seed, vy0 = 0: all in the first wavefront
Family = collections.namedtuple("Family", "name kind problems seeds kw")
FAMILIES = ("correct_x0", "correct_z0", "correct_planar", "target_jacobi", "target_period", "target_planar_jacobi",
            "target_planar_period", "arc_seed", "arc_seed_planar", "arc_step", "arc_step_planar")

# The spread of this reference between TIGHT and LOOSE over the iterates of its own loops on the replayed records of each family,
# as tests/test_halo_newton_host.py measures and holds them (res_k, |d_k|_inf, 2 t_c, tangent, det relative), and RK4's own
# truncation error at RK4_STEPS steps over RK4_T_MAX against scipy from the same start (residual, |d|_inf), by a plain numpy RK4.
#                                res_k    |d_k|    2 t_c    tangent  det (relative)        measured
SPREAD = {"correct_x0":           (1e-13, 2e-14, 1e-13, 0.0, 0.0),          # 5.2e-14  1.3e-14  4.8e-14
          "correct_z0":           (1e-13, 1e-14, 1e-13, 0.0, 0.0),          # 6.1e-14  4.0e-15  3.4e-14
          "correct_planar":       (1e-13, 1e-14, 1e-12, 0.0, 0.0),          # 6.9e-14  3.6e-15  6.1e-13
          "target_jacobi":        (1e-13, 5e-14, 2e-13, 0.0, 0.0),          # 5.0e-14  2.1e-14  8.4e-14
          "target_period":        (1e-13, 2e-14, 1e-13, 0.0, 0.0),          # 4.0e-14  1.0e-14  4.1e-14
          "target_planar_jacobi": (1e-12, 1e-14, 1e-12, 0.0, 0.0),          # 5.4e-13  6.2e-15  5.9e-13
          "target_planar_period": (5e-13, 1e-12, 5e-13, 0.0, 0.0),          # 2.3e-13  4.6e-13  2.3e-13
          "arc_seed":             (1e-13, 1e-14, 1e-13, 5e-13, 2e-12),      # 6.2e-14  4.1e-15  4.0e-14  3.3e-13  1.5e-12
          "arc_seed_planar":      (1e-13, 2e-15, 1e-12, 2e-14, 5e-12),      # 5.0e-14  8.8e-16  6.4e-13  1.3e-14  2.8e-12
          "arc_step":             (5e-14, 1e-14, 2e-13, 2e-14, 5e-13),      # 2.5e-14  5.0e-15  9.6e-14  1.4e-14  3.8e-13
          "arc_step_planar":      (1e-13, 2e-15, 1e-12, 1e-14, 5e-12)}      # 7.6e-14  1.0e-15  5.6e-13  7.7e-15  2.6e-12
# What the device's 2 t_c, tangent and det (relative) are held to against this reference from the device's own iterate: ten times the
# largest spread of any family, rounded up to a power of ten (the project's rule; the flights are the same whatever the family).
PERIOD_BOUND, TANGENT_BOUND, DET_BOUND = 1e-11, 1e-11, 1e-10
RK4_STEPS, RK4_T_MAX = 4000, 2.9
# (residual, |d|_inf, 2 t_c, tangent, det relative): twice the measured 5.2e-12 / 2.5e-13 / 8.4e-12, 5.5e-12 / 3.7e-12 / 8.8e-12 and
# 7.0e-12 / 2.7e-13 / 1.0e-11 / 3.6e-12 / 4.1e-11 -- the error is smooth in the start, and the device's iterates lie within the
# step bound of the host's
RK4_ERR = {"correct_x0": (1.1e-11, 6e-13, 1.7e-11, 0.0, 0.0), "target_jacobi": (1.2e-11, 8e-12, 1.8e-11, 0.0, 0.0),
           "arc_step": (1.5e-11, 6e-13, 2.1e-11, 7.2e-12, 8.3e-11)}


def res_bound(name):
    """The residual bound of a family: RES_BOUND for the corrector; else ten times the spread of res_k, not below RES_BOUND."""
    if name.startswith("correct") or name not in SPREAD:
        return RES_BOUND
    return max(RES_BOUND, 10.0 * SPREAD[name][0])


def _with_failures(seeds):
    seeds = np.array(seeds, dtype=float)
    seeds[NAN_SEED, 0] = np.nan
    seeds[STILL, 4] = 0.0
    return seeds.T


def _near(p, MU):
    """The point this restatement's own loop reaches from p, moved by 1e-8 in vy0: one iteration from there."""
    run = newton(p, MU)
    assert run.status == 0
    return run.iterates[-1] + np.array([0.0, 0.0, 1e-8])


def _u(seed):
    return np.array([seed[0], seed[2], seed[4]], dtype=float)


def family(name, base, MU):
    """One family of B records.  base: the two packaged halo seeds (halo_reference.seed_of).  Records REPLAYED are rough seeds, NEAR
    is one step from converged, NAN_SEED and STILL fail at once, the others are rough seeds held to their single calls."""
    return _cached(("family", name, MU), lambda: _family(name, base, MU))


def _halo_bases(base, MU):
    got = [HR.correct(s, HR.HOLD_X0, MU) for s in base]
    assert all(g.status == 0 for g in got)
    return [(g.state, g.period) for g in got]


def _lyapunov_bases(MU):
    got = [HR.correct(AR.lyapunov_seed_np(w, 1e-2, MU), HR.PLANAR, MU) for w in (1, 2)]
    assert all(g.status == 0 for g in got)
    return [(g.state, g.period) for g in got]


def _family(name, base, MU):
    kind = {"c": CORRECT, "t": TARGET, "a": ARCLENGTH}[name[0]]
    if kind == CORRECT:
        mode = {"correct_x0": HR.HOLD_X0, "correct_z0": HR.HOLD_Z0, "correct_planar": HR.PLANAR}[name]
        if mode == HR.PLANAR:                   # linear Lyapunov seeds from HR.PLANAR_AX up, where the period is well-conditioned: 4 to 6 steps
            rough = [AR.lyapunov_seed_np(w, ax, MU) for w, ax in ((1, 3e-3), (2, 3e-3), (2, 3e-3), (2, 5e-3), (2, 3e-3), (2, 3e-3), (2, 1e-2),
                                                                  (2, 2e-2), (1, 5e-3))]
        else:
            rough = list(HR.gpu_seeds(base, "x0" if mode == HR.HOLD_X0 else "z0")[:, 2:2 + B].T)
        seeds = [s.copy() for s in rough]
        probs = [Problem(CORRECT, _u(s), mode=mode) for s in seeds]
        near = _near(probs[0], MU)
        seeds[NEAR] = _state(near)
        probs[NEAR] = Problem(CORRECT, near, mode=mode)
        return Family(name, kind, probs, _with_failures(seeds), {"mode": {HR.HOLD_X0: "x0", HR.HOLD_Z0: "z0", HR.PLANAR: "planar"}[mode]})
    if kind == TARGET:
        planar, what = "planar" in name, TR.PERIOD if name.endswith("period") else TR.JACOBI
        bases = _lyapunov_bases(MU) if planar else _halo_bases(base, MU)
        cs = TR.cases(planar, what, bases, MU)[2:2 + B]
        seeds, q = [c[0].copy() for c in cs], np.array([c[1] for c in cs])
        probs = [Problem(TARGET, _u(s), qstar=float(q[b]), what=what, planar=planar) for b, s in enumerate(seeds)]
        near = _near(probs[0], MU)
        seeds[NEAR], q[NEAR] = _state(near), q[0]
        probs[NEAR] = Problem(TARGET, near, qstar=float(q[0]), what=what, planar=planar)
        return Family(name, kind, probs, _with_failures(seeds), {"targets": q, "what": "period" if what == TR.PERIOD else "jacobi", "planar": planar})
    planar, step = "planar" in name, "step" in name
    orbit = (_lyapunov_bases(MU)[1] if planar else _halo_bases(base, MU)[0])[0]
    dir0 = np.array([0.0, 0.0, 1.0])
    pert = AR.planar_perturbed if planar else HR.perturbed
    seeds = [pert(orbit, k) for k in range(2, 2 + B)]
    if not step:
        probs = [Problem(ARCLENGTH, _u(s), planar=planar, u_prev=_u(s), t_row=dir0, ds=0.0, orient=True) for s in seeds]
        near = _near(probs[0], MU)
        seeds[NEAR] = _state(near)
        probs[NEAR] = Problem(ARCLENGTH, near, planar=planar, u_prev=near, t_row=dir0, ds=0.0, orient=True)
        return Family(name, kind, probs, _with_failures(seeds), {"planar": planar, "dir0": dir0, "dir_is_tangent": False, "ds": ARC_DS})
    # a member step: from perturbed copies of the orbit along the orbit's own tangent (towards larger vy0) by ARC_DS
    t_row = arclength_pass(_u(orbit), _u(orbit), dir0, 0.0, planar, MU, orient=True).t_new
    mk = lambda s: Problem(ARCLENGTH, None, planar=planar, u_prev=_u(s), t_row=t_row, ds=ARC_DS, orient=False)      # noqa: E731
    probs = [mk(s) for s in seeds]
    seeds[NEAR] = _state(_near(probs[0], MU) - ARC_DS * t_row)
    probs[NEAR] = mk(seeds[NEAR])
    return Family(name, kind, probs, _with_failures(seeds), {"planar": planar, "dir0": t_row, "dir_is_tangent": True, "ds": ARC_DS})


ARC_DS = 0.02                               # the member steps' ds (= ds_min = ds_max: an attempt is not tried again)
ARC_DS_LONG = 0.08                          # the deliberately long predictor of the B = 1 case


def long_step(base, MU):
    """The B = 1 member step with a long predictor: from the corrected packaged orbit 1 along its tangent by ARC_DS_LONG."""
    orbit = _halo_bases(base, MU)[0][0]
    t_row = arclength_pass(_u(orbit), _u(orbit), np.array([0.0, 0.0, 1.0]), 0.0, False, MU, orient=True).t_new
    return Problem(ARCLENGTH, None, planar=False, u_prev=_u(orbit), t_row=t_row, ds=ARC_DS_LONG, orient=False), orbit


def target_march(base, MU):
    """(seed [6], targets [3]) of the march whose member 2 starts from the secant point: orbit 1 towards smaller C."""
    state, _ = _halo_bases(base, MU)[0]
    C = HR.jacobi(state, MU)
    return HR.perturbed(state, 2), np.array([C - 1e-3, C - 2e-3, C - 4e-3])


# ---------------------------------------------------------------------------- RK4 of the 42-component system in numpy
def rk4_half_flight(u, MU, steps, t_max):
    """The correctors' RK4 flight in numpy on halo_reference.rhs42: `steps` steps over t_max, the first step at whose end y has left
    the side vy0 sent it to, the crossing by bisection over trial steps from that step's start.  (t, x, Phi, f) as half_flight."""
    f = HR.rhs42(MU)

    def step(w, h):
        k1 = f(0.0, w)
        k2 = f(0.0, w + 0.5 * h * k1)
        k3 = f(0.0, w + 0.5 * h * k2)
        k4 = f(0.0, w + h * k3)
        return w + h / 6.0 * (k1 + 2.0 * k2 + 2.0 * k3 + k4)

    w, h = HR.start42(_state(u)), t_max / steps
    side = 1.0 if u[2] > 0.0 else -1.0
    for k in range(steps):
        ws, w = w, step(w, h)
        if not side * w[1] > 0.0:
            lo, hi = 0.0, 1.0
            for _ in range(60):
                mid = 0.5 * (lo + hi)
                if side * step(ws, mid * h)[1] > 0.0:
                    lo = mid
                else:
                    hi = mid
            wc = step(ws, hi * h)
            return k * h + hi * h, wc[:6], wc[6:].reshape(6, 6), f(0.0, wc)[:6]
    return None


def rk4_pass(p, u, MU, t_row=None, steps=RK4_STEPS, t_max=RK4_T_MAX):
    """one_pass with rk4_half_flight in halo_reference.half_flight's place: what the pass decides under the correctors' RK4 flight."""
    keep = HR.half_flight
    HR.half_flight = lambda state, mu, tm, rtol, atol: rk4_half_flight(_u(state), mu, steps, t_max)
    try:
        return one_pass(p, u, MU, ("rk4", steps), t_row, None, t_max)
    finally:
        HR.half_flight = keep


def rk4_cases(base, MU):
    """The RK4 case of each kernel: record 0 of a family that starts from packaged orbit 1 (half period 1.454 of RK4_T_MAX = 2.9)."""
    return {name: family(name, base, MU).problems[0] for name in ("correct_x0", "target_jacobi", "arc_step")}
