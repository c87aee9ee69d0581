"""GPU checks of the targeted periodic-orbit corrector (lto_halo_target_batch) against the independent host reference
(tests/halo_target_reference.py: the same 3 x 3 Newton rule in numpy on scipy's DOP853 at rtol 1e-13 / atol 1e-14).

Bounds.  Device against reference: ten times the reference's own spread between (1e-13, 1e-14) and (1e-11, 1e-12) per quantity and
case class, rounded up to a power of ten (halo_target_reference.BOUNDS; tests/test_halo_target_host.py holds the spread to a tenth):

  class            spread state / period     bound state / period     device state / period (MI355X)
  3-D    Jacobi    1.5e-13 / 4.1e-13         1e-11 / 1e-11            9.6e-15 / 3.9e-14
  3-D    period    8.5e-14 / 2.0e-14         1e-12 / 1e-12            5.6e-15 / 1.3e-14
  planar Jacobi    1.0e-14 / 1.6e-12         1e-12 / 1e-10            9.6e-15 / 3.9e-13
  planar period    2.4e-12 / 1.6e-13         1e-10 / 1e-11            8.5e-14 / 1.7e-13

The marches (planar Jacobi class; 3-D Jacobi class for orbit 1 -> the C of orbit 2): state <= 8.2e-15, period <= 3.1e-13.  RK4 with
2 000 steps per half period against DOP853: 1.2e-11 (bound 1e-9, DESIGN 4.25's).

Properties that need no reference keep tol = 1e-12 itself: |C(state_out) - C*| with C formed in numpy, |period_out - P*|, resid_out."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import halo_reference as HR  # noqa: E402
import halo_target_reference as TR  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-12
WHAT = {"jacobi": TR.JACOBI, "period": TR.PERIOD}
_REF = {}


def _bases(planar):
    """The two converged orbits the cases start from, by the reference: (state, period) x 2, computed once."""
    if ("bases", planar) not in _REF:
        if planar:
            got = [HR.correct(drivers.lyapunov_seed(w, 1e-2, MU)[0], HR.PLANAR, MU) for w in (1, 2)]
        else:
            got = [HR.correct(HR.seed_of(np.asarray(tb[:6], dtype=float)), HR.HOLD_X0, MU) for tb in synth.halo_orbits()]
        assert all(g.status == 0 for g in got)
        _REF[("bases", planar)] = [(g.state, g.period) for g in got]
    return _REF[("bases", planar)]


def _ref_target(seed, q, what, planar):
    """The reference's targeted corrector on one (seed, target), computed once and shared (never modified)."""
    key = (tuple(seed), q, what, planar)
    if key not in _REF:
        _REF[key] = TR.target_correct(seed, q, WHAT[what], planar, MU, tol=TOL)
    return _REF[key]


def _ref_march(seed, targets, what, planar):
    key = ("march", tuple(seed), tuple(targets), what, planar)
    if key not in _REF:
        _REF[key] = TR.march(seed, list(targets), WHAT[what], planar, MU, tol=TOL)
    return _REF[key]


def _cases(planar, what, B):
    cs = TR.cases(planar, WHAT[what], _bases(planar), MU)[:B]
    return np.array([c[0] for c in cs]).T, np.array([c[1] for c in cs])


def _q_of(state, period, what):
    return HR.jacobi(state, MU) if what == "jacobi" else period


@pytest.mark.parametrize("B", [1, 9, 17])
@pytest.mark.parametrize("what", ["jacobi", "period"])
@pytest.mark.parametrize("planar", [False, True])
def test_target_against_the_reference(gpu_ctx, planar, what, B):
    seeds, targets = _cases(planar, what, B)
    if B > 1:
        r = lto.halo_target(seeds, targets[None, :], what=what, planar=planar, tol=TOL, ctx=gpu_ctx)
        assert r.state.shape == (6, 1, B) and r.history.shape == (16, 1, B)
    else:
        r = lto.halo_target(seeds[:, 0], targets[0], what=what, planar=planar, tol=TOL, ctx=gpu_ctx)
        assert r.state.shape == (6,) and r.history.shape == (16,) and isinstance(r.period, float)
    state, hist = np.asarray(r.state).reshape(6, B), np.asarray(r.history).reshape(-1, B)
    period, jac, resid = (np.asarray(v, dtype=float).reshape(B) for v in (r.period, r.jacobi, r.resid))
    its, status = np.asarray(r.iterations).reshape(B), np.asarray(r.status).reshape(B)
    b_state, b_P = TR.BOUNDS[(planar, WHAT[what])]
    worst = [0.0, 0.0, 0.0]
    for b in range(B):
        ref = _ref_target(seeds[:, b], targets[b], what, planar)
        assert ref.status == 0
        e_state, e_P = np.abs(state[:, b] - ref.state).max(), abs(period[b] - ref.period)
        e_q = abs(_q_of(state[:, b], period[b], what) - targets[b])
        worst = [max(worst[0], e_state), max(worst[1], e_P), max(worst[2], e_q)]
        print("%s %s B=%d b=%d: state %.2e, P %.2e, |q - q*| %.2e, resid %.2e, iterations %d (reference %d)" % (
            "planar" if planar else "3-D", what, B, b, e_state, e_P, e_q, resid[b], its[b], ref.iterations))
        assert status[b] == 0
        assert e_state <= b_state and e_P <= b_P
        assert e_q < TOL and resid[b] < TOL
        assert abs(jac[b] - HR.jacobi(state[:, b], MU)) <= 1e-14
        assert HR.same_count(its[b], ref.iterations, ref.history, TOL), (b, its[b], ref.history)
        assert state[1, b] == 0.0 and state[3, b] == 0.0 and state[5, b] == 0.0 and (not planar or state[2, b] == 0.0)
        n = int(its[b]) + 1                                # the history: one residual per flight, NaN past the last
        assert np.all(np.isfinite(hist[:n, b])) and np.all(np.isnan(hist[n:, b])) and hist[n - 1, b] == resid[b]
    print("%s %s B=%d worst: state %.2e (bound %.0e), P %.2e (bound %.0e), |q - q*| %.2e" % (
        "planar" if planar else "3-D", what, B, worst[0], b_state, worst[1], b_P, worst[2]))


def _same_member(rb, k, b, r1):
    """Member (k, b) of a marched batch against a single call's record, bit for bit."""
    return (np.array_equal(rb.state[:, k, b], r1.state, equal_nan=True) and np.array_equal(rb.period[k, b], r1.period, equal_nan=True)
            and np.array_equal(rb.jacobi[k, b], r1.jacobi, equal_nan=True) and np.array_equal(rb.resid[k, b], r1.resid, equal_nan=True)
            and rb.iterations[k, b] == r1.iterations and rb.status[k, b] == r1.status
            and np.array_equal(rb.history[:, k, b], r1.history, equal_nan=True))


def _lyapunov_pair():
    bases = _bases(True)
    return np.array([bases[0][0], bases[1][0]]).T


@pytest.mark.parametrize("K", [3, 4, 8])
def test_march_to_a_common_jacobi_constant(gpu_ctx, K):
    """L1 and L2 Lyapunov orbits side by side, K equal steps of C each down to 3.15."""
    seeds = _lyapunov_pair()
    targets = drivers._step_table(HR.jacobi(seeds, MU), TR.C_COMMON, K)
    rb = lto.halo_target(seeds, targets, what="jacobi", planar=True, tol=TOL, ctx=gpu_ctx)
    b_state, b_P = TR.BOUNDS[(True, TR.JACOBI)]
    for b in range(2):
        ref = _ref_march(seeds[:, b], targets[:, b], "jacobi", True)
        print("K=%d L%d: iterations %s (reference %s)" % (K, b + 1, list(rb.iterations[:, b]), [m.iterations for m in ref]))
        for k in range(K):
            e_state, e_P = np.abs(rb.state[:, k, b] - ref[k].state).max(), abs(rb.period[k, b] - ref[k].period)
            print("    member %d: state %.2e, P %.2e" % (k, e_state, e_P))
            assert rb.status[k, b] == 0 and ref[k].status == 0
            assert e_state <= b_state and e_P <= b_P
            assert abs(HR.jacobi(rb.state[:, k, b], MU) - targets[k, b]) < TOL and rb.resid[k, b] < TOL
            assert HR.same_count(rb.iterations[k, b], ref[k].iterations, ref[k].history, TOL), (k, b, ref[k].history)
            # the member is the single call from the predictor's point, formed here from the call's own outputs
            if k == 0:
                start = seeds[:, b]
            elif k == 1:
                start = rb.state[:, 0, b]
            else:
                start = TR.predictor(rb.state[:, k - 1, b], rb.state[:, k - 2, b], targets[k, b], targets[k - 1, b], targets[k - 2, b])
            assert _same_member(rb, k, b, lto.halo_target(start, targets[k, b], what="jacobi", planar=True, tol=TOL, ctx=gpu_ctx)), (k, b)
    assert abs(rb.period[-1, 0] - 2.844831406797) < 1e-10 and abs(rb.period[-1, 1] - 3.420569721966) < 1e-10


def test_march_of_halo_orbit_1_to_the_jacobi_constant_of_orbit_2(gpu_ctx):
    (s1, _), (s2, P2) = _bases(False)
    targets = drivers._step_table([HR.jacobi(s1, MU)], HR.jacobi(s2, MU), 4)[:, 0]
    r = lto.halo_target(s1, targets, what="jacobi", tol=TOL, ctx=gpu_ctx)
    ref = _ref_march(s1, targets, "jacobi", False)
    b_state, b_P = TR.BOUNDS[(False, TR.JACOBI)]
    for k in range(4):
        e_state, e_P = np.abs(r.state[:, k] - ref[k].state).max(), abs(r.period[k] - ref[k].period)
        print("member %d: state %.2e, P %.2e, iterations %d (reference %d)" % (k, e_state, e_P, r.iterations[k], ref[k].iterations))
        assert r.status[k] == 0 and e_state <= b_state and e_P <= b_P and HR.same_count(r.iterations[k], ref[k].iterations, ref[k].history, TOL)
    # the family is a curve: the member of orbit 2's C is orbit 2
    assert np.abs(r.state[:, -1] - s2).max() <= b_state and abs(r.period[-1] - P2) <= b_P
    drv = drivers.halo_family_by(s1, targets, "jacobi", tol=TOL, ctx=gpu_ctx)
    assert np.array_equal(drv.states, r.state) and np.array_equal(drv.period, r.period) and np.array_equal(drv.status, r.status)


@pytest.mark.parametrize("what", ["jacobi", "period"])
@pytest.mark.parametrize("planar", [False, True])
def test_batch_equals_singles_and_repeats(gpu_ctx, planar, what):
    seeds, targets = _cases(planar, what, 9)
    rb = lto.halo_target(seeds, targets[None, :], what=what, planar=planar, tol=TOL, ctx=gpu_ctx)
    again = lto.halo_target(seeds, targets[None, :], what=what, planar=planar, tol=TOL, ctx=gpu_ctx)
    for f in rb._fields:
        assert np.array_equal(getattr(rb, f), getattr(again, f), equal_nan=True), f
    for b in (0, 7, 8):                                    # both wavefronts of the batch
        assert _same_member(rb, 0, b, lto.halo_target(seeds[:, b], targets[b], what=what, planar=planar, tol=TOL, ctx=gpu_ctx)), b


def _none(r, k, b):
    return (np.all(np.isnan(r.state[:, k, b])) and np.isnan(r.period[k, b]) and np.isnan(r.jacobi[k, b]) and np.isnan(r.resid[k, b]))


def test_statuses_in_a_mixed_batch(gpu_ctx):
    (s1, P1), (s2, P2) = _bases(False)
    C1, C2 = HR.jacobi(s1, MU), HR.jacobi(s2, MU)
    nan_seed, still = s1.copy(), s2.copy()
    nan_seed[0] = np.nan
    still[4] = 0.0
    seeds = np.array([s1, nan_seed, s2, still, s1, HR.perturbed(s1, 3)]).T
    q = np.array([C1 + 1e-4, C1, C2 - 1e-3, C2, np.nan, C1 + 5e-3])
    rb = lto.halo_target(seeds, q[None, :], tol=TOL, ctx=gpu_ctx)
    assert list(rb.status[0]) == [0, 2, 0, 2, 2, 0]
    for b in (1, 3, 4):                                     # a NaN seed, vy0 = 0, a NaN target: no numbers
        assert _none(rb, 0, b) and rb.iterations[0, b] == 0 and np.all(np.isnan(rb.history[:, 0, b]))
    for b in (0, 2, 5):
        assert _same_member(rb, 0, b, lto.halo_target(seeds[:, b], q[b], tol=TOL, ctx=gpu_ctx))

    # a period target <= 0, beside a good one
    rp = lto.halo_target(np.array([s1, s2, s1]).T, np.array([[P1 + 1e-3, 0.0, -1.0]]), what="period", tol=TOL, ctx=gpu_ctx)
    assert list(rp.status[0]) == [0, 2, 2] and _none(rp, 0, 1) and _none(rp, 0, 2)
    assert _same_member(rp, 0, 0, lto.halo_target(s1, P1 + 1e-3, what="period", tol=TOL, ctx=gpu_ctx))

    # planar: z0 != 0 is refused next to a Lyapunov orbit
    lyap = _lyapunov_pair()[:, 0]
    Cl = HR.jacobi(lyap, MU) - 1e-3
    rz = lto.halo_target(np.array([lyap, s1]).T, np.array([[Cl, Cl]]), planar=True, tol=TOL, ctx=gpu_ctx)
    assert list(rz.status[0]) == [0, 2] and _none(rz, 0, 1)
    assert _same_member(rz, 0, 0, lto.halo_target(lyap, Cl, planar=True, tol=TOL, ctx=gpu_ctx))

    # t_max = 1.0 is before either half period (1.454, 1.565): no crossing
    rt = lto.halo_target(np.array([s1, s2]).T, np.array([[C1, C2]]), t_max=1.0, tol=TOL, ctx=gpu_ctx)
    assert list(rt.status[0]) == [2, 2] and _none(rt, 0, 0) and _none(rt, 0, 1)

    # max_steps = 5: the flight runs out of steps
    rs = lto.halo_target(np.array([s1, s2]).T, np.array([[C1, C2]]), integ=lto.integrator(max_steps=5), tol=TOL, ctx=gpu_ctx)
    assert list(rs.status[0]) == [2, 2] and np.all(np.isnan(rs.state))

    # max_iter = 0 evaluates the start: status 1 for a target off the orbit's own value, history[0] = the residual
    r0 = lto.halo_target(np.array([s1, s2]).T, np.array([[C1 + 1e-4, C2 - 1e-3]]), max_iter=0, tol=TOL, ctx=gpu_ctx)
    assert list(r0.status[0]) == [1, 1] and list(r0.iterations[0]) == [0, 0] and r0.history.shape == (1, 1, 2)
    assert np.array_equal(r0.state[:, 0, 0], s1) and np.array_equal(r0.state[:, 0, 1], s2)
    assert np.array_equal(r0.history[0], r0.resid) and abs(r0.resid[0, 0] - 1e-4) < 1e-12 and abs(r0.resid[0, 1] - 1e-3) < 1e-12
    assert abs(r0.period[0, 0] - P1) < 1e-11

    # sing_tol = 0.999: by Hadamard's inequality |det| <= the product of the row norms, and for these starts the ratio is below
    # 0.9 (vetted on the host), so the first step is refused as singular
    r3 = lto.halo_target(np.array([s1, s2]).T, np.array([[C1 + 1e-4, C2 - 1e-3]]), sing_tol=0.999, tol=TOL, ctx=gpu_ctx)
    assert list(r3.status[0]) == [3, 3] and _none(r3, 0, 0) and _none(r3, 0, 1) and list(r3.iterations[0]) == [0, 0]
    assert np.all(np.isfinite(r3.history[0, 0])) and np.all(np.isnan(r3.history[1:, 0]))


def test_a_failed_member_ends_its_family_only(gpu_ctx):
    """A member that cannot be reached (a NaN target in the second place) leaves the rest of its family NaN with status 2; with
    max_steps = 5 every family dies at its first member.  The neighbouring family is untouched, bit for bit."""
    seeds = _lyapunov_pair()
    targets = drivers._step_table(HR.jacobi(seeds, MU), TR.C_COMMON, 4)
    good = lto.halo_target(seeds, targets, planar=True, tol=TOL, ctx=gpu_ctx)
    broken = targets.copy()
    broken[1, 0] = np.nan
    r = lto.halo_target(seeds, broken, planar=True, tol=TOL, ctx=gpu_ctx)
    assert list(r.status[:, 0]) == [0, 2, 2, 2] and list(r.status[:, 1]) == [0, 0, 0, 0]
    assert all(_none(r, k, 0) and np.all(np.isnan(r.history[:, k, 0])) for k in (1, 2, 3))
    for f in r._fields:
        assert np.array_equal(getattr(r, f)[..., 1], getattr(good, f)[..., 1], equal_nan=True), f
        assert np.array_equal(getattr(r, f)[..., 0, 0], getattr(good, f)[..., 0, 0], equal_nan=True), f
    rs = lto.halo_target(seeds, targets, planar=True, integ=lto.integrator(max_steps=5), tol=TOL, ctx=gpu_ctx)
    assert np.all(rs.status == 2) and np.all(np.isnan(rs.state)) and np.all(np.isnan(rs.period))
    assert np.all(rs.iterations == 0) and np.all(np.isnan(rs.history))


def test_rk4_agrees_with_dop853(gpu_ctx):
    """4 000 steps over t_max = 2.9 = two half periods of orbit 1: 2 000 steps per half period, the setting DESIGN 4.25 measured the
    corrector's RK4 form at (4.3e-12 against DOP853, bound 1e-9: RK4's h^4 with the flow's growth over half a revolution)."""
    (s1, P1), _ = _bases(False)
    q = HR.jacobi(s1, MU) + 1e-4
    a = lto.halo_target(s1, q, tol=TOL, ctx=gpu_ctx)
    r = lto.halo_target(s1, q, t_max=2.9, integ=lto.integrator(lto.RK4, steps=4000), tol=TOL, ctx=gpu_ctx)
    e = max(np.abs(a.state - r.state).max(), abs(a.period - r.period))
    print("targeted corrector RK4 x 2000 per half period against DOP853: %.2e" % e)
    assert a.status == 0 and r.status == 0 and e <= 1e-9


def test_refusals_through_the_raw_entry_point(gpu_ctx):
    import ctypes as C
    (s1, _), _ = _bases(False)
    fn, h = gpu_ctx.fn("halo_target_batch"), gpu_ctx.handle
    S = np.asfortranarray(s1.reshape(6, 1))
    Q = np.array([HR.jacobi(s1, MU) + 1e-4])
    state, period, status = np.zeros(6), np.zeros(1), np.zeros(1, dtype=np.int32)
    ptr = lambda arr: arr.ctypes.data_as(C.c_void_p)        # noqa: E731

    def call(n_targets=1, n_batch=1, mu=MU, what=0, tol=1e-12, max_iter=15, t_max=10.0, sing_tol=1e-12, integ=None, seeds=S,
             out=state):
        integ = integ or lto.integrator()
        return fn(h, n_targets, n_batch, mu, 0, what, ptr(seeds) if seeds is not None else None, ptr(Q), tol, max_iter, t_max, sing_tol,
                  C.byref(integ), ptr(out) if out is not None else None, ptr(period), None, None, None, None, ptr(status))

    assert call() == 0 and status[0] == 0
    for kw in ({"n_targets": 0}, {"n_batch": 0}, {"what": 2}, {"what": -1}, {"tol": 0.0}, {"max_iter": -1}, {"t_max": 0.0},
               {"t_max": np.inf}, {"mu": 1.5}, {"sing_tol": 1.0}, {"integ": lto.integrator(lto.RK4, steps=0)},
               {"n_targets": 1 << 20, "n_batch": 1 << 20}, {"n_targets": 1 << 16, "n_batch": 1 << 13},
               {"n_targets": 1 << 14, "n_batch": 1 << 13, "max_iter": 15}, {"n_batch": 1 << 28, "max_iter": 0}):
        assert call(**kw) == -1, kw
    for method in (lto.RKF78_FIXED, lto.RKF78_ADAPTIVE):
        assert call(integ=lto.integrator(method, steps=10)) == -3
    assert call(seeds=None) == -2 and call(out=None) == -2
    assert fn(None, 1, 1, MU, 0, 0, None, None, 1e-12, 15, 10.0, 1e-12, None, None, None, None, None, None, None, None) == -2
    assert call() == 0 and status[0] == 0                  # the context is fine afterwards
    assert gpu_ctx.lib.lto_last_call_ms(gpu_ctx.handle) > 0.0


def test_halo_orbit_at_a_jacobi_constant(gpu_ctx):
    (s1, _), _ = _bases(False)
    q = HR.jacobi(s1, MU) - 1e-3
    o = drivers.halo_orbit_at(s1, jacobi=q, n_samples=50, tol=TOL, ctx=gpu_ctx)
    print("halo_orbit_at: C = %.15f (asked %.15f), closure %.2e, P = %.12f" % (o.jacobi[0], q, o.closure, o.period))
    assert o.status == 0 and abs(o.jacobi[0] - q) < TOL and o.closure <= 1e-10 and o.states.shape == (6, 50)
    p = drivers.halo_orbit_at(s1, period=o.period, n_samples=3, tol=TOL, ctx=gpu_ctx)
    assert p.status == 0 and abs(p.period - o.period) < TOL and np.abs(p.state0 - o.state0).max() <= 1e-10


@pytest.fixture(scope="module")
def matched(gpu_ctx):
    return drivers.matched_orbits(_lyapunov_pair(), TR.C_COMMON, n_steps=8, planar=True, tol=TOL, ctx=gpu_ctx)


def test_matched_orbits_share_the_jacobi_constant(matched):
    a, b = matched
    print("matched: C = %.15f, %.15f; P = %.12f, %.12f" % (a.jacobi[0], b.jacobi[0], a.period, b.period))
    assert a.status == 0 and b.status == 0
    assert abs(a.jacobi[0] - TR.C_COMMON) < TOL and abs(b.jacobi[0] - TR.C_COMMON) < TOL and abs(a.jacobi[0] - b.jacobi[0]) < TOL
    assert abs(a.period - 2.844831406797) < 1e-10 and abs(b.period - 3.420569721966) < 1e-10
    print("closures %.2e, %.2e; nu %s, %s" % (a.closure, b.closure, a.nu, b.nu))


def test_connection_refinement_never_grows(gpu_ctx, matched):
    from lowthrustopt_amd.constants import DU, TU
    a, b = matched
    found = drivers.manifold_connections(a, b, n_phase=32, ctx=gpu_ctx)
    assert found
    levels = drivers.manifold_connection_refine(a, b, found[0], levels=3, n_phase=8, spacing=1.0 / 32.0, ctx=gpu_ctx)
    assert len(levels) == 3
    dist = [found[0].dist] + [c.dist for c in levels]
    print("refinement: %s" % ", ".join("%.3e (%.1f km, %.2f m/s)" % (c.dist, c.dr_km, c.dv_ms) for c in [found[0]] + levels))
    assert all(dist[i + 1] <= dist[i] for i in range(3)) and dist[-1] < dist[0]
    for c in levels:
        dr, dv = np.linalg.norm(c.x1[:3] - c.x2[:3]), np.linalg.norm(c.x1[3:] - c.x2[3:])
        assert abs(c.dr_km - dr * DU) <= 1e-9 * max(1.0, dr * DU) and abs(c.dv_ms - dv * DU / TU * 1e3) <= 1e-9 * max(1.0, dv * DU / TU * 1e3)
        assert abs(c.dist - np.hypot(dr, dv)) <= 1e-12
        assert c.branch1 == found[0].branch1 and c.branch2 == found[0].branch2
