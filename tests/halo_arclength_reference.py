"""Independent host reference of the pseudo-arclength continuation of periodic-orbit families: the rule of
lto_halo_arclength_batch -- tangent from the cross product of DF's two rows, its orientation, the predictor, the Newton step on
[DF; t_row], step halving and growth, both start modes -- in numpy (numpy.cross, numpy.linalg.solve) on scipy's DOP853 with a
terminal event on y (halo_reference.half_flight).  Nothing here comes from the product; MU and the seeds are passed in by the tests."""
import collections

import numpy as np

import halo_reference as HR

RTOL, ATOL = HR.RTOL, HR.ATOL
LOOSE = (1e-11, 1e-12)                      # the second pair of tolerances: the reference's own spread is measured between the two

Member = collections.namedtuple("Member", "state tangent det ds halvings period jacobi resid iterations history status dots")
NAN3, NAN6 = np.full(3, np.nan), np.full(6, np.nan)


def system(u, planar, MU, t_max=10.0, rtol=RTOL, atol=ATOL):
    """(F [2], DF [2 x 3], t_c) of one flight from (x0, 0, z0, 0, vy0, 0), u = (x0, z0, vy0); None without a crossing before t_max.
    Planar: the z0 row and column are the identity's."""
    fl = HR.half_flight(np.array([u[0], 0.0, u[1], 0.0, u[2], 0.0]), MU, t_max, rtol, atol)
    if fl is None:
        return None
    tc, xc, Phi, f = fl
    if not np.all(np.isfinite(xc)) or not np.all(np.isfinite(Phi)):
        return None
    rows, cols = [3, 5], [0, 2, 4]
    DF = Phi[np.ix_(rows, cols)] - np.outer(f[rows], Phi[1, cols]) / f[1]
    F = np.array(xc[rows])
    if planar:
        DF[0, 1] = 0.0
        DF[1] = (0.0, 1.0, 0.0)
        F[1] = 0.0
    return F, DF, tc


def tangent(DF, t_row):
    """(t, det, c . t_row): t = sigma c / |c|, det = sigma |c| with c = DF_0 x DF_1 and sigma the sign of c . t_row; None where |c| or
    the dot product is zero or not finite."""
    c = np.cross(DF[0], DF[1])
    n, d = np.linalg.norm(c), float(c @ t_row)
    if not np.isfinite(n) or n == 0.0 or not np.isfinite(d) or d == 0.0:
        return None
    sg = 1.0 if d > 0.0 else -1.0
    return sg * c / n, sg * n, d


def singular(J, sing_tol):
    det = np.linalg.det(J)
    return not np.isfinite(det) or abs(det) <= sing_tol * np.prod(np.linalg.norm(J, axis=1))


def attempt(u_prev, t_row, ds, orient, planar, MU, tol=1e-12, max_iter=15, t_max=10.0, sing_tol=1e-12, cos_min=0.0, rtol=RTOL, atol=ATOL):
    """One attempt at a member from u_prev along t_row by ds.  orient: the seed is yet to be put on the family -- ds = 0 and the row
    vector is the tangent of the first flight's DF with the sign that makes its product with t_row (the caller's dir0) positive.
    Returns Member (ds and halvings as passed / 0); dots = the member's t_new . t_row_used."""
    u_prev, t_row = np.asarray(u_prev, dtype=float), np.asarray(t_row, dtype=float)
    u_pred = u_prev + ds * t_row
    u = u_pred.copy()
    hist, it = [], 0
    oriented = not orient

    def bad(status):
        return Member(NAN6, NAN3, np.nan, ds, 0, np.nan, np.nan, np.nan, it, hist, status, np.nan)

    if not np.all(np.isfinite(u)) or u[2] == 0.0 or (planar and u[1] != 0.0):
        return bad(2)
    while True:
        sysm = system(u, planar, MU, t_max, rtol, atol)
        if sysm is None:
            return bad(2)
        F, DF, tc = sysm
        if not oriented:
            c = np.cross(DF[0], DF[1])
            d = float(c @ t_row)
            if not np.isfinite(d) or d == 0.0:
                return bad(2)
            tg = tangent(DF, t_row)
            if tg is None:
                return bad(3)
            t_row = tg[0]
            oriented = True
        r2 = float(t_row @ (u - u_pred))
        res = max(abs(F[0]), abs(r2)) if planar else max(abs(F[0]), abs(F[1]), abs(r2))
        hist.append(res)
        if res < tol or it >= max_iter:
            tg = tangent(DF, t_row)
            if tg is None:
                return bad(3)
            t_new, det, _ = tg
            dots = float(t_new @ t_row)
            status = 0 if res < tol else 1
            if status == 0 and dots < cos_min:
                return Member(NAN6, NAN3, np.nan, ds, 0, np.nan, np.nan, np.nan, it, hist, 4, dots)
            state = np.array([u[0], 0.0, u[1], 0.0, u[2], 0.0])
            return Member(state, t_new, det, ds, 0, 2.0 * tc, HR.jacobi(state, MU), res, it, hist, status, dots)
        J = np.vstack([DF, t_row])
        if singular(J, sing_tol):
            return bad(3)
        u = u - np.linalg.solve(J, np.array([F[0], F[1], r2]))
        it += 1


def usable_start(seed, dir0, planar):
    u, d = np.array([seed[0], seed[2], seed[4]], dtype=float), np.asarray(dir0, dtype=float)
    return bool(np.all(np.isfinite(u)) and np.all(np.isfinite(d)) and u[2] != 0.0 and not (planar and u[1] != 0.0) and np.any(d != 0.0))


def march(seed, dir0, ds0, n_members, planar, MU, dir_is_tangent=False, ds_min=None, ds_max=None, grow=1.0, fast_iter=3, trace=None, **kw):
    """n_members members one after another with the step control of the issue: a failed attempt (status not 0, status 4 included) is
    tried again with ds / 2 until ds < ds_min, then the member keeps the last attempt's status and the rest is NaN with status 2;
    after an accepted member of <= fast_iter steps ds <- min(ds grow, ds_max).  trace: a list that receives (k, ds, Member) of every
    attempt."""
    ds_min = ds0 / 1024.0 if ds_min is None else ds_min
    ds_max = ds0 if ds_max is None else ds_max
    dead_member = Member(NAN6, NAN3, np.nan, np.nan, 0, np.nan, np.nan, np.nan, 0, [], 2, np.nan)
    members = []
    dead = not usable_start(seed, dir0, planar)
    u_prev, t_row, ds = np.array([seed[0], seed[2], seed[4]], dtype=float), np.asarray(dir0, dtype=float), float(ds0)
    for k in range(n_members):
        if dead:
            members.append(dead_member)
            continue
        orient = k == 0 and not dir_is_tangent
        dsa, halv = (0.0 if orient else ds), 0
        while True:
            m = attempt(u_prev, t_row, dsa, orient, planar, MU, **kw)
            if trace is not None:
                trace.append((k, dsa, m))
            if m.status == 0 or orient or 0.5 * dsa < ds_min:
                break
            dsa, halv = 0.5 * dsa, halv + 1
        m = m._replace(halvings=halv)
        members.append(m)
        if m.status != 0:
            dead = True
            continue
        u_prev, t_row = m.state[[0, 2, 4]], m.tangent
        if not orient:
            ds = dsa
            if m.iterations <= fast_iter:
                ds = min(ds * grow, ds_max)
    return members


def family_bifurcations(members):
    det = np.array([m.det for m in members])
    return [k for k in range(1, len(det)) if det[k] * det[k - 1] < 0.0]


def family_folds(members, j):
    t = np.array([m.tangent[j] for m in members])
    return [k for k in range(1, len(t)) if t[k] * t[k - 1] < 0.0]


def branch_point(members, k, planar, MU, max_trials=8, **kw):
    """The point between members k - 1 and k where det = 0: a secant in the arclength s from member k - 1 on det(s), each trial a
    one-member step from member k - 1 along its tangent; stops at |det| < 1e-9 |det_(k-1)| or after max_trials.  Returns (Member,
    trials [(s, det)])."""
    a, b = members[k - 1], members[k]
    u, t = a.state[[0, 2, 4]], a.tangent
    s0, d0, s1, d1 = 0.0, a.det, b.ds, b.det
    trials, best = [], None
    for _ in range(max_trials):
        s = s1 - d1 * (s1 - s0) / (d1 - d0)
        m = attempt(u, t, s, False, planar, MU, **kw)
        assert m.status == 0
        trials.append((s, m.det))
        best = m
        if abs(m.det) < 1e-9 * abs(a.det):
            break
        s0, d0, s1, d1 = s1, d1, s, m.det
    return best, trials


def halo_from_lyapunov(which, n_members, ds, MU, north=True, Ax=1e-2, ds_switch=1e-2, ds_lyap=1e-2, block=16, max_blocks=8, **kw):
    """MU alone -> the planar Lyapunov orbit of x-amplitude Ax, the family in the 3-unknown form with z0 = 0 (towards larger orbits: the
    tangent's vy0 component has the sign of vy0) in blocks of `block` members up to the first sign change of det, the branch point,
    the step off the plane by ds_switch along (0, +-1, 0), and n_members members up the halo family.  `seed` is the Lyapunov orbit.
    Returns (branch point Member, [switch member] + halo members)."""
    seed = HR.correct(lyapunov_seed_np(which, Ax, MU), HR.PLANAR, MU).state
    dir0 = np.array([0.0, 0.0, np.sign(seed[4])])
    fam = march(seed, dir0, ds_lyap, block, False, MU, **kw)
    for _ in range(max_blocks):
        flips = family_bifurcations(fam)
        if flips:
            break
        last = fam[-1]
        fam = fam[-1:] + march(last.state, last.tangent, ds_lyap, block, False, MU, dir_is_tangent=True, **kw)
    bp, _ = branch_point(fam, flips[0], False, MU, **kw)
    z = 1.0 if north else -1.0
    sw = march(bp.state, np.array([0.0, z, 0.0]), ds_switch, 1, False, MU, dir_is_tangent=True, **kw)[0]
    halo = march(sw.state, sw.tangent, ds, n_members, False, MU, dir_is_tangent=True, **kw)
    return bp, [sw] + halo


def lyapunov_seed_np(which, Ax, MU):
    """The linear planar Lyapunov seed of x-amplitude Ax about L1 / L2 (Richardson's first order), formed here in numpy."""
    rh = (MU / 3.0) ** (1.0 / 3.0)
    x = 1.0 - MU - rh if which == 1 else 1.0 - MU + rh
    for _ in range(60):
        a, b = x + MU, x - 1.0 + MU
        x -= (x - (1.0 - MU) * a / abs(a) ** 3 - MU * b / abs(b) ** 3) / (1.0 + 2.0 * (1.0 - MU) / abs(a) ** 3 + 2.0 * MU / abs(b) ** 3)
    c2 = (1.0 - MU) / abs(x + MU) ** 3 + MU / abs(x - 1.0 + MU) ** 3
    lam = np.sqrt((2.0 - c2 + np.sqrt(9.0 * c2 * c2 - 8.0 * c2)) / 2.0)
    k = (lam * lam + 1.0 + 2.0 * c2) / (2.0 * lam)
    return np.array([x - Ax, 0.0, 0.0, 0.0, k * lam * Ax, 0.0])


def planar_perturbed(seed, k):
    """HR.perturbed kept in the plane."""
    s = HR.perturbed(seed, k)
    s[2] = 0.0
    return s


def batch_seeds(base, n, in_plane):
    """The base seed and n - 1 copies off by <= 1e-4 in position and 1e-3 in vy0 (HR.perturbed), [6 x n]."""
    base = np.asarray(base, dtype=float)
    return np.array([base] + [(planar_perturbed if in_plane else HR.perturbed)(base, k) for k in range(1, n)]).T


# ---------------------------------------------------------------------------- the cases of the GPU tests, vetted on the host
Case = collections.namedtuple("Case", "name cls seeds dir0 ds K planar tangent")
_CACHE = {}


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def lyapunov_orbit(which, MU):
    """The planar Lyapunov orbit of x-amplitude 1e-2 about L1 / L2, corrected by HR.correct."""
    def make():
        got = HR.correct(lyapunov_seed_np(which, 1e-2, MU), HR.PLANAR, MU)
        assert got.status == 0
        return got.state
    return _cached(("lyapunov", which, MU), make)


LYAPUNOV_MEMBERS = {1: 8, 2: 16}            # members of the 3-unknown march at ds = 0.01 that reach past the halo bifurcation


def lyapunov_family(which, MU):
    return _cached(("family", which, MU), lambda: march(lyapunov_orbit(which, MU), [0.0, 0.0, 1.0], 0.01, LYAPUNOV_MEMBERS[which], False, MU))


def halo_branch(which, MU):
    """(branch point Member, trials) of the first sign change of det along lyapunov_family."""
    def make():
        fam = lyapunov_family(which, MU)
        return branch_point(fam, family_bifurcations(fam)[0], False, MU)
    return _cached(("branch", which, MU), make)


def switched(which, z, ds, MU):
    """The member one step of ds off the plane from the branch point along (0, z, 0)."""
    def make():
        m = march(halo_branch(which, MU)[0].state, [0.0, z, 0.0], ds, 1, False, MU, dir_is_tangent=True)[0]
        assert m.status == 0
        return m
    return _cached(("switched", which, z, ds, MU), make)


N_BATCH = 17
CLASSES = ("planar", "lyapunov3", "switch", "halo_L2", "halo_L1")


def cases(MU):
    """The marches of tests/test_halo_arclength_gpu.py's comparison with this reference: every case is a batch of N_BATCH seeds, the
    base seed and its perturbed copies."""
    def make():
        out = []
        for w in (1, 2):
            out.append(Case("planar_L%d" % w, "planar", batch_seeds(lyapunov_orbit(w, MU), N_BATCH, True), np.array([0.0, 0.0, 1.0]),
                            0.01, 8, True, False))
        out.append(Case("lyapunov3_L2", "lyapunov3", batch_seeds(lyapunov_orbit(2, MU), N_BATCH, True), np.array([0.0, 0.0, 1.0]), 0.01,
                        16, False, False))
        bp = halo_branch(2, MU)[0].state
        for z in (1.0, -1.0):
            for ds in (1e-3, 1e-2):
                out.append(Case("switch_L2_%s_%g" % ("north" if z > 0 else "south", ds), "switch", batch_seeds(bp, N_BATCH, False),
                                np.array([0.0, z, 0.0]), ds, 1, False, True))
        # L2: from the step off the plane.  L1: from the fourth member of the march of ds = 0.01 from there -- next to the L1 branch
        # point the halo family turns so fast that a first step of 0.02 is refused (halved) from the base seed and from 6 of the 16
        # copies, and copy 11 went to another family; from the fourth member on, 0.02 takes 3 or 4 steps for every copy.
        sw = switched(2, -1.0, 1e-2, MU)
        out.append(Case("halo_L2", "halo_L2", batch_seeds(sw.state, N_BATCH, False), sw.tangent.copy(), 0.02, 24, False, True))
        sw = switched(1, -1.0, 1e-2, MU)
        m3 = march(sw.state, sw.tangent, 0.01, 4, False, MU, dir_is_tangent=True)[3]
        assert m3.status == 0 and m3.halvings == 0
        out.append(Case("halo_L1", "halo_L1", batch_seeds(m3.state, N_BATCH, False), m3.tangent.copy(), 0.02, 24, False, True))
        return {c.name: c for c in out}
    return _cached(("cases", MU), make)


def case_march(case, b, MU, loose=False, **kw):
    """Seed b of a case marched by this reference at the tight or the loose tolerances, computed once and never modified."""
    tl = {"rtol": LOOSE[0], "atol": LOOSE[1]} if loose else {}
    key = ("march", case.name, b, loose, tuple(sorted(kw.items())), MU)
    return _cached(key, lambda: march(case.seeds[:, b], case.dir0, case.ds, case.K, case.planar, MU, dir_is_tangent=case.tangent, **tl, **kw))


def differences(a, b):
    """(state, tangent, period, det relative) differences of two marches' members, the largest over the members."""
    return (max(np.abs(x.state - y.state).max() for x, y in zip(a, b)), max(np.abs(x.tangent - y.tangent).max() for x, y in zip(a, b)),
            max(abs(x.period - y.period) for x, y in zip(a, b)), max(abs(x.det - y.det) / abs(x.det) for x, y in zip(a, b)))


# The step-control cases: per orbit (seed, dir0, ds0), the call's keywords, and the class whose bounds hold for its members.
StepCase = collections.namedtuple("StepCase", "name cls seeds dir0 ds0 K planar tangent kw")
COS_MARGIN = 0.05                           # no tangent product of a step-control case lies this close to its cos_min


def step_cases(MU):
    """halve: the planar L2 family's half period grows with the orbit (1.698 one step of 0.08 from the Ax = 1e-2 orbit, 1.717 at 0.16),
    so with t_max = 1.712 a step of 0.16 finds no crossing (status 2) and is halved once; the next member is refused at 0.08 and
    taken at 0.04.  grow / nogrow: the same family from ds = 0.005 with grow = 1.5 up to ds_max = 0.012, every member fast
    (fast_iter = 3) or none (fast_iter = 0).  dsmin: with cos_min = 0.949 and ds_min = 0.015 the first step of 0.02 from the step
    off the plane at L2 is refused (the tangent turns by 26 degrees there: status 4) and 0.01 is below ds_min, beside a family that
    goes on from the 8th member of the halo march, where the tangent turns by 2 degrees a step."""
    def make():
        sw = switched(2, -1.0, 1e-2, MU)
        h7 = case_march(cases(MU)["halo_L2"], 0, MU)[7]
        lyap = lyapunov_orbit(2, MU)
        f0 = lyapunov_family(2, MU)[0]
        up = np.array([0.0, 0.0, 1.0])
        out = [StepCase("halve", "planar", f0.state[:, None], f0.tangent[:, None], np.array([0.16]), 2, True, True,
                        {"t_max": 1.712, "ds_min": 0.005}),
               StepCase("grow", "planar", lyap[:, None], up[:, None], np.array([0.005]), 6, True, False,
                        {"grow": 1.5, "ds_max": 0.012, "fast_iter": 3, "ds_min": 1e-4}),
               StepCase("nogrow", "planar", lyap[:, None], up[:, None], np.array([0.005]), 6, True, False,
                        {"grow": 1.5, "ds_max": 0.012, "fast_iter": 0, "ds_min": 1e-4}),
               StepCase("dsmin", "halo_L2", np.array([sw.state, h7.state]).T, np.array([sw.tangent, h7.tangent]).T, np.array([0.02, 0.02]), 3,
                        False, True, {"cos_min": 0.949, "ds_min": 0.015, "ds_max": 0.02})]
        return {c.name: c for c in out}
    return _cached(("step_cases", MU), make)


def step_march(case, b, MU, loose=False, **over):
    """(members, trace of every attempt) of orbit b of a step-control case; over: keywords that replace the case's."""
    def make():
        tl = {"rtol": LOOSE[0], "atol": LOOSE[1]} if loose else {}
        trace = []
        kw = dict(case.kw, **over)
        kw.setdefault("ds_min", case.ds0[b] / 1024.0)
        kw.setdefault("ds_max", case.ds0[b])
        got = march(case.seeds[:, b], case.dir0[:, b], case.ds0[b], case.K, case.planar, MU, dir_is_tangent=case.tangent, trace=trace,
                    **kw, **tl)
        return got, trace
    return _cached(("step", case.name, b, loose, tuple(sorted(over.items())), MU), make)


# The bounds the device is held to against this reference, per case class on (states, tangents, periods, det relative): ten times
# this reference's own spread between (1e-13, 1e-14) and LOOSE over the class's cases (the step-control cases of the class
# included), rounded up to a power of ten.  tests/test_halo_arclength_host.py measures the spreads and holds them to a tenth of
# the bound:
#   planar      state 1.4e-14   tangent 6.6e-13   period 3.3e-12   det 5.1e-11
#   lyapunov3   state 3.8e-15   tangent 1.1e-13   period 3.1e-12   det 4.7e-10
#   switch      state 1.1e-12   tangent 3.4e-10   period 6.2e-13   det 2.2e-11
#   halo_L2     state 2.5e-13   tangent 3.4e-12   period 7.2e-13   det 2.1e-11
#   halo_L1     state 1.1e-11   tangent 2.5e-09   period 4.7e-11   det 2.4e-09     (the family turns by 45 degrees in one step at its end)
BOUNDS = {"planar": (1e-12, 1e-11, 1e-10, 1e-9), "lyapunov3": (1e-13, 1e-11, 1e-10, 1e-8), "switch": (1e-10, 1e-8, 1e-11, 1e-9),
          "halo_L2": (1e-11, 1e-10, 1e-11, 1e-9), "halo_L1": (1e-9, 1e-7, 1e-9, 1e-7)}
