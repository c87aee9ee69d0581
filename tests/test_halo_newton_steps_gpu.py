"""GPU checks of every Newton iteration of the three periodic-orbit correctors (k_halo_correct, k_halo_target, k_halo_arclength;
DESIGN 4.25, 4.27, 4.28) against the one-iteration restatement on the independent references (tests/halo_newton_reference.py).

Mechanism.  All three kernels store the current iterate with status 1 when `it >= max_iter`, so the call with max_iter = k returns the
loop's state after k iterations; each case is called with max_iter = 0 .. K (K: the iteration count of the full call).  Then

  * the prefix property: the call with max_iter = k has the first k + 1 entries of the full call's history bit for bit,
    iterations = min(k, K), status 1 for k < K and the full call's status and state, bit for bit, for k >= K;
  * per iteration, from the device's own iterate u_k: |history[k] - res_k| <= the residual bound (1e-11, what the suite holds a
    device residual to; no family's spread asks for more), and on counted steps |(u_(k+1) - u_k) + d_k|_inf <= the step bound
    |J^-1|_inf x 1e-11 + 10 x the reference's own spread of d_k (halo_newton_reference.replay); a step is counted where that bound
    is at most 1e-4 |d_k|_inf, so a Jacobian wrong by 1e-3 is ten times over it (tests/test_halo_newton_host.py shows that);
  * what is held does not move by a bit, y = vx = vz = 0 exactly, the period output is 2 t_c of the reference's flight from u_k, the
    Jacobi output C(u_k), the arclength outputs (tangent, det, ds, halvings) those of the reference from u_k;
  * the stopping rule and the singular rule, bit-exact from the device's own numbers.

Shapes.  Every family runs as a batch of 9: one full wavefront of 8 groups and one group beside 7 shadow groups in a second.  The
first wavefront holds rough seeds (3 to 8 iterations), a nearly converged one (1 iteration), a NaN seed and one with vy0 = 0, so
that groups that have left the loop sit beside groups still iterating.  Records 0, 3, 7 and 8 are replayed against the reference,
the others are held to their single-orbit calls bit for bit at every k.  B = 1: the RK4 cases, the stopping and singular rules.

Measured on an MI355X (DESIGN 4.25 has the table): 121 counted steps, the largest step error 2.7e-3 of its bound (k_halo_correct, planar),
history within 4.7e-13 of the reference's residual; under RK4 5.6e-2 of the bound and 7.0e-12."""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import halo_reference as HR  # noqa: E402
import halo_target_reference as TR  # noqa: E402
import halo_newton_reference as NR  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import synth  # noqa: E402
from lowthrustopt_amd.constants import MU  # noqa: E402

pytestmark = pytest.mark.gpu

R = collections.namedtuple("R", "state period resid iterations history status jacobi tangent det ds halvings",
                           defaults=(None,) * 5)
_BASE = []


def _base():
    if not _BASE:
        _BASE.extend(HR.seed_of(np.asarray(tb[:6], dtype=float)) for tb in synth.halo_orbits())
    return _BASE


def _call(ctx, kind, kw, seeds, max_iter=NR.MAX_ITER, **over):
    """The kind's entry on seeds [6 x n] (a batch even for n = 1), one member per orbit; every output with the batch axis last."""
    seeds = np.asarray(seeds, dtype=float).reshape(6, -1)
    common = dict(tol=NR.TOL, max_iter=max_iter, ctx=ctx)
    common.update(over)
    if kind == NR.CORRECT:
        r = lto.halo_correct(seeds, kw["mode"], **common)
        return R(r.state, r.period, r.resid, r.iterations, r.history, r.status)
    if kind == NR.TARGET:
        r = lto.halo_target(seeds, np.asarray(kw["targets"], dtype=float).reshape(1, -1), what=kw["what"], planar=kw["planar"], **common)
        return R(r.state[:, 0], r.period[0], r.resid[0], r.iterations[0], r.history[:, 0], r.status[0], r.jacobi[0])
    ds = kw["ds"]
    r = lto.halo_arclength(seeds, 1, ds, kw["dir0"], planar=kw["planar"], dir_is_tangent=kw["dir_is_tangent"], ds_min=ds, ds_max=ds, grow=1.0,
                           **common)
    return R(r.state[:, 0], r.period[0], r.resid[0], r.iterations[0], r.history[:, 0], r.status[0], r.jacobi[0], r.tangent[:, 0], r.det[0],
             r.ds[0], r.halvings[0])


def _cols(kw, cols):
    """The call's keywords for the records `cols` alone."""
    return dict(kw, targets=np.asarray(kw["targets"])[cols]) if "targets" in kw else kw


def _same(ra, a, rb, b):
    """Record a of one result against record b of another, bit for bit in every output (the histories as far as the shorter goes)."""
    n = min(ra.history.shape[0], rb.history.shape[0])
    return (all(np.array_equal(np.asarray(x)[..., a], np.asarray(y)[..., b], equal_nan=True)
                for f, x, y in zip(R._fields, ra, rb) if x is not None and f != "history")
            and np.array_equal(ra.history[:n, a], rb.history[:n, b], equal_nan=True))


def _prefix(full, runs, b):
    """The prefix property of record b: runs[k] is the call with max_iter = k."""
    K, st = int(full.iterations[b]), int(full.status[b])
    for k, r in enumerate(runs):
        assert r.history.shape[0] == k + 1
        assert np.array_equal(r.history[:, b], full.history[:k + 1, b], equal_nan=True), (b, k)
        if st >= 2:                                          # a seed that fails at once: nothing but NaN at every k
            assert r.status[b] == st and r.iterations[b] == 0 and np.all(np.isnan(r.history[:, b])) and np.all(np.isnan(r.state[:, b]))
            continue
        assert r.iterations[b] == min(k, K), (b, k)
        if k < K:
            assert r.status[b] == 1, (b, k)
            assert np.all(np.isfinite(r.history[:, b]))
        else:
            assert r.status[b] == st and _same(r, b, full, b), (b, k)


def _replayed(label, p, runs, b, K, extra=(0.0,) * 5, need=2):
    """Iterations 0 .. K of record b against the reference from the device's own iterates.  Returns (counted steps, the largest
    step error / bound, the largest residual deviation)."""
    U = [runs[k].state[[0, 2, 4], b] for k in range(K + 1)]
    assert np.array_equal(U[0], NR.first_iterate(p)), label                   # the seed, or the predictor's point, bit for bit
    steps = NR.replay(p, U, MU, res_bound=NR.RES_BOUND, d_extra=extra[1])
    counted, worst, worst_res = 0, 0.0, 0.0
    for k in range(K + 1):
        r, s = runs[k], steps[k]
        e_res = abs(runs[K].history[k, b] - s.res)
        worst_res = max(worst_res, e_res)
        line = "%s b=%d k=%d: res %.3e (reference off by %.1e)" % (label, b, k, runs[K].history[k, b], e_res)
        assert np.all(r.state[[1, 3, 5], b] == 0.0), (label, b, k)
        # what is held does not move by a bit
        if p.kind == NR.CORRECT and p.mode != HR.HOLD_Z0:
            assert U[k][0] == U[0][0], (label, b, k)
        if (p.kind == NR.CORRECT and p.mode != HR.HOLD_X0) or p.planar:
            assert U[k][1] == U[0][1], (label, b, k)
        e_P = abs(r.period[b] - s.ref.period)
        assert e_P <= NR.PERIOD_BOUND + extra[2], (label, b, k, e_P)
        if r.jacobi is not None:
            assert abs(r.jacobi[b] - HR.jacobi(r.state[:, b], MU)) <= 1e-14, (label, b, k)
        if p.kind == NR.ARCLENGTH:
            e_t, e_det = np.abs(r.tangent[:, b] - s.ref.t_new).max(), abs(r.det[b] - s.ref.det) / abs(s.ref.det)
            line += ", tangent %.1e det %.1e" % (e_t, e_det)
            assert e_t <= NR.TANGENT_BOUND + extra[3] and e_det <= NR.DET_BOUND + extra[4], (label, b, k, e_t, e_det)
            assert np.sign(r.det[b]) == np.sign(s.ref.det) and r.tangent[:, b] @ s.ref.t_row > 0.0
            assert np.sign(r.det[b]) == np.sign(np.cross(s.ref.J[0], s.ref.J[1]) @ s.ref.t_row)
            if p.orient and k == 0:                          # the seed's tangent points dir0's way
                assert r.tangent[:, b] @ p.t_row > 0.0
            assert r.ds[b] == (0.0 if p.orient else p.ds) and r.halvings[b] == 0
            assert abs(np.linalg.norm(r.tangent[:, b]) - 1.0) <= 1e-15
        if k < K:
            e_d = np.abs((U[k + 1] - U[k]) + s.d).max()
            line += ", |d| %.2e, step off by %.1e (bound %.1e%s)" % (np.abs(s.d).max(), e_d, s.bound, ", counted" if s.counted else "")
            if s.counted:
                counted += 1
                worst = max(worst, e_d / s.bound)
        print(line)
        assert e_res <= NR.RES_BOUND + extra[0], (label, b, k, e_res)
        if k < K and s.counted:
            assert e_d <= s.bound, (label, b, k, e_d, s.bound)
    assert counted >= need, (label, b, counted)
    return counted, worst, worst_res


@pytest.mark.parametrize("name", NR.FAMILIES)
def test_every_iteration_of_a_batch_of_nine(gpu_ctx, name):
    fam = NR.family(name, _base(), MU)
    everyone = list(range(NR.B))
    full = _call(gpu_ctx, fam.kind, fam.kw, fam.seeds)
    assert [int(s) for s in full.status] == [2 if b in (NR.NAN_SEED, NR.STILL) else 0 for b in everyone], list(full.status)
    Kmax = int(full.iterations.max())
    assert Kmax <= 10
    runs = [_call(gpu_ctx, fam.kind, fam.kw, fam.seeds, max_iter=k) for k in range(Kmax + 1)]
    counted, worst, worst_res = 0, 0.0, 0.0
    for b in everyone:
        _prefix(full, runs, b)
        if b in NR.REPLAYED:
            c, w, wr = _replayed(name, fam.problems[b], runs, b, int(full.iterations[b]))
            counted, worst, worst_res = counted + c, max(worst, w), max(worst_res, wr)
        elif full.status[b] == 0:                            # held to its single-orbit call at every k
            for k, r in enumerate(runs):
                assert _same(r, b, _call(gpu_ctx, fam.kind, _cols(fam.kw, [b]), fam.seeds[:, b], max_iter=k), 0), (name, b, k)
    print("FIGURES %s: %d counted steps, the largest step error %.1e of its bound, the largest residual deviation %.1e; iterations %s" % (
        name, counted, worst, worst_res, [int(i) for i in full.iterations]))
    assert counted >= 8
    assert full.iterations[NR.NEAR] == 1 and all(full.iterations[b] >= 3 for b in everyone if b not in (NR.NEAR, NR.NAN_SEED, NR.STILL))


SINGLES = ["correct_x0", "target_jacobi", "arc_step"]       # one family per kernel


def _single(name):
    fam = NR.family(name, _base(), MU)
    return fam, fam.problems[0], fam.seeds[:, 0], _cols(fam.kw, [0])


@pytest.mark.parametrize("name", SINGLES)
def test_every_iteration_under_rk4(gpu_ctx, name):
    """halo_return_rk4 is the flight: RK4_STEPS steps over RK4_T_MAX (2 000 per half period of orbit 1).  The reference stays
    scipy's flight; the residual bound is widened by RK4's own truncation error there, the step bound by its error in d and the
    bounds of period, tangent and det by theirs, all measured on the CPU (halo_newton_reference.RK4_ERR; tests/test_halo_newton_host.py)."""
    fam, p, seed, kw = _single(name)
    over = dict(t_max=NR.RK4_T_MAX, integ=lto.integrator(lto.RK4, steps=NR.RK4_STEPS))
    full = _call(gpu_ctx, fam.kind, kw, seed, **over)
    K = int(full.iterations[0])
    assert full.status[0] == 0 and 3 <= K <= 5
    runs = [_call(gpu_ctx, fam.kind, kw, seed, max_iter=k, **over) for k in range(K + 1)]
    _prefix(full, runs, 0)
    c, w, wr = _replayed(name + " RK4", p, runs, 0, K, extra=NR.RK4_ERR[name], need=1)
    print("FIGURES %s RK4: %d counted steps, the largest step error %.1e of its bound, the largest residual deviation %.1e" % (name, c, w, wr))


def test_every_iteration_of_a_long_predictor(gpu_ctx):
    """B = 1, ds = 0.08 from orbit 1: the predictor is 2.6e-2 off the family and the loop takes 4 to 6 iterations.  r[2] =
    t_row . (u - u_pred) is linear in u, so Newton meets it at the first step and it is rounding noise from k = 1 on, whatever ds
    (tests/test_halo_newton_host.py); that the device forms it from the right predictor shows in history[k] all the same."""
    p, orbit = NR.long_step(_base(), MU)
    kw = {"planar": False, "dir0": p.t_row, "dir_is_tangent": True, "ds": p.ds}
    full = _call(gpu_ctx, NR.ARCLENGTH, kw, orbit)
    K = int(full.iterations[0])
    assert full.status[0] == 0 and 4 <= K <= 6
    runs = [_call(gpu_ctx, NR.ARCLENGTH, kw, orbit, max_iter=k) for k in range(K + 1)]
    _prefix(full, runs, 0)
    c, w, wr = _replayed("arc_long", p, runs, 0, K, need=3)
    print("FIGURES arc_long: %d counted steps, the largest step error %.1e of its bound, the largest residual deviation %.1e" % (c, w, wr))


def test_every_iteration_of_a_marched_member(gpu_ctx):
    """A march of T = 3: member 2 starts from the secant point, which the host forms bit for bit from the call's outputs."""
    seed, targets = NR.target_march(_base(), MU)
    m = lto.halo_target(seed, targets, what="jacobi", tol=NR.TOL, ctx=gpu_ctx)
    assert list(m.status) == [0, 0, 0]
    start = TR.predictor(m.state[:, 1], m.state[:, 0], targets[2], targets[1], targets[0])
    kw = {"targets": targets[2:], "what": "jacobi", "planar": False}
    full = _call(gpu_ctx, NR.TARGET, kw, start)
    K = int(full.iterations[0])
    assert K == m.iterations[2] and K >= 2 and np.array_equal(full.state[:, 0], m.state[:, 2]) and full.period[0] == m.period[2]
    assert np.array_equal(full.history[:, 0], m.history[:, 2], equal_nan=True) and full.jacobi[0] == m.jacobi[2]
    runs = [_call(gpu_ctx, NR.TARGET, kw, start, max_iter=k) for k in range(K + 1)]
    _prefix(full, runs, 0)
    p = NR.Problem(NR.TARGET, NR._u(start), qstar=float(targets[2]), what=TR.JACOBI, planar=False)
    c, w, wr = _replayed("target_march", p, runs, 0, K, need=1)
    print("FIGURES target_march: %d counted steps, the largest step error %.1e of its bound, the largest residual deviation %.1e" % (c, w, wr))


@pytest.mark.parametrize("name", SINGLES)
def test_the_stopping_rule_is_strict(gpu_ctx, name):
    fam, p, seed, kw = _single(name)
    full = _call(gpu_ctx, fam.kind, kw, seed)
    k = 1
    assert full.status[0] == 0 and full.iterations[0] > k
    h = float(full.history[k, 0])
    at = _call(gpu_ctx, fam.kind, kw, seed, tol=h)                              # res < tol is strict: history[k] itself does not stop
    assert at.iterations[0] > k and np.array_equal(at.history[:k + 1, 0], full.history[:k + 1, 0])
    above = _call(gpu_ctx, fam.kind, kw, seed, tol=float(np.nextafter(h, np.inf)))
    stopped = _call(gpu_ctx, fam.kind, kw, seed, max_iter=k)
    assert above.status[0] == 0 and above.iterations[0] == k and stopped.status[0] == 1
    assert np.array_equal(above.state[:, 0], stopped.state[:, 0]) and above.period[0] == stopped.period[0] and above.resid[0] == h
    assert np.array_equal(above.history[:k + 1, 0], full.history[:k + 1, 0]) and np.all(np.isnan(above.history[k + 1:, 0]))


@pytest.mark.parametrize("name", SINGLES + ["correct_planar"])
def test_the_singular_rule(gpu_ctx, name):
    """sing_tol twice the reference's measure |det| / prod |row|_2 at the seed refuses the first step, half of it changes nothing;
    the factor 2 is 1e6 times the measure's spread (tests/test_halo_newton_host.py).  The planar form of k_halo_correct only asks
    |J| > 0: no sing_tol makes it singular."""
    fam, p, seed, kw = _single(name)
    s = NR.one_pass(p, NR.first_iterate(p), MU).sing
    free = _call(gpu_ctx, fam.kind, kw, seed, sing_tol=0.0)
    assert free.status[0] == 0
    if name == "correct_planar":
        assert _same(_call(gpu_ctx, fam.kind, kw, seed, sing_tol=0.999), 0, free, 0)
        return
    assert 2.0 * s < 1.0
    assert _same(_call(gpu_ctx, fam.kind, kw, seed, sing_tol=0.5 * s), 0, free, 0)
    r = _call(gpu_ctx, fam.kind, kw, seed, sing_tol=2.0 * s)
    assert r.status[0] == 3 and r.iterations[0] == 0
    assert r.history[0, 0] == free.history[0, 0] and np.all(np.isnan(r.history[1:, 0]))
    assert np.all(np.isnan(r.state[:, 0])) and np.isnan(r.period[0]) and np.isnan(r.resid[0])
    if r.tangent is not None:
        assert np.all(np.isnan(r.tangent[:, 0])) and np.isnan(r.det[0]) and r.halvings[0] == 0
