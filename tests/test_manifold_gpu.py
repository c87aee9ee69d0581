"""GPU checks of the invariant-manifold calls (lto_halo_manifold_seeds_batch, lto_section_flight_batch, lto_state_match_batch and
the drivers above them) against the independent host reference (tests/manifold_reference.py: mpmath at 50 digits for
the eigen step, scipy DOP853 at rtol 1e-13 / atol 1e-14 for the flights, numpy for the match).  Every bound is a named constant of
tests/test_manifold_host.py, which holds the reference's own spread to a tenth of it.  The shapes are the smallest that can still go
wrong: the 64 vetted starts (two orbits x 8 phases x 4 branches) cut to 1, 63 and 65 arcs, 1 to 17 phases.

Figures measured on an MI355X are in DESIGN 4.26."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import manifold_reference as MR  # noqa: E402
import test_manifold_host as H  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402

pytestmark = pytest.mark.gpu

Y0 = ("y", 0.0)
X1MU = ("x", 1.0 - MU)


@pytest.fixture(scope="module")
def orbits():
    return MR.packaged_orbits(synth.halo_orbits(), MU)


def _batch(orbits, ks):
    return (np.array([orbits[k][0] for k in ks]).T, np.array([orbits[k][1] for k in ks]),
            np.stack([orbits[k][2] for k in ks], axis=2))


def _same(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b) if x is not None)


# ------------------------------------------------------------------------------------------------------------------- 1. eigen step
def _check_eigen(lam, V, M, tag):
    e = MR.eig_pair(M)
    d = (abs(lam[0] - e.lam_u) / abs(e.lam_u), abs(lam[1] - e.lam_s) / abs(e.lam_s),
         np.abs(V[:, 0] - e.v_u).max(), np.abs(V[:, 1] - e.v_s).max())
    print("%s: lambda_u %.15g lambda_s %.15g, lambda_u lambda_s - 1 = %.2e; against 50 digits: %.1e %.1e (relative), vectors %.1e %.1e"
          % (tag, lam[0], lam[1], lam[0] * lam[1] - 1.0, *d))
    assert d[0] <= H.GPU_LAM_U_REL and d[1] <= H.GPU_LAM_S_REL and d[2] <= H.GPU_VEC_U and d[3] <= H.GPU_VEC_S
    for kind in range(2):
        assert abs(np.linalg.norm(V[:, kind]) - 1.0) <= 1e-15 and V[0, kind] > 0.0


@pytest.mark.parametrize("B", [1, 2])
def test_eigen_step_on_the_packaged_orbits(gpu_ctx, orbits, B):
    S, P, M = _batch(orbits, range(B))
    r = lto.manifold_seeds(S if B > 1 else S[:, 0], P if B > 1 else P[0], M if B > 1 else M[:, :, 0], [0.0], eps=1e-3, ctx=gpu_ctx)
    lam, X, V, status = (np.asarray(r.lam).reshape(2, B), np.asarray(r.X).reshape(6, 2, 1, B), np.asarray(r.V).reshape(6, 2, 1, B),
                         np.atleast_1d(r.status))
    for b in range(B):
        assert status[b] == 0
        _check_eigen(lam[:, b], V[:, :, 0, b], M[:, :, b], "orbit %d of %d" % (b + 1, B))
        assert np.array_equal(X[:, 0, 0, b], S[:, b]) and np.array_equal(X[:, 1, 0, b], S[:, b])       # nothing is flown


def test_eigen_step_mixed_batch(gpu_ctx, orbits):
    """A negative lambda_u is accepted; a complex dominant pair, a NaN entry and an M without an expanding direction give status 1
    with NaN outputs; the good orbits beside them stay bitwise what their single calls give."""
    S, P, M = _batch(orbits, [0, 0, 0, 0, 1, 1])
    M = M.copy()
    M[:, :, 1], M[:, :, 2], M[:, :, 3] = H.synthetic_M("negative"), H.synthetic_M("complex"), H.synthetic_M("nan")
    M[:, :, 5] = np.eye(6)
    r = lto.manifold_seeds(S, P, M, [0.0], eps=1e-3, ctx=gpu_ctx)
    print("statuses %s, lambda %s" % (r.status, r.lam.T))
    assert list(r.status) == [0, 0, 1, 1, 0, 1]
    _check_eigen(r.lam[:, 1], r.V[:, :, 0, 1], M[:, :, 1], "synthetic, lambda_u = -30")
    assert abs(r.lam[0, 1] + 30.0) < 1e-11
    for b in (2, 3, 5):
        assert np.all(np.isnan(r.lam[:, b])) and np.all(np.isnan(r.X[..., b])) and np.all(np.isnan(r.V[..., b]))
        assert np.all(np.isnan(r.starts[..., b]))
    for b, k in ((0, 0), (4, 1)):
        one = lto.manifold_seeds(orbits[k][0], orbits[k][1], orbits[k][2], [0.0], eps=1e-3, ctx=gpu_ctx)
        assert _same((r.lam[:, b], r.X[..., b], r.V[..., b], r.starts[..., b]), (one.lam, one.X, one.V, one.starts))
        assert one.status == 0


# ------------------------------------------------------------------------------------------------------------------------- 2. seeds
@pytest.mark.parametrize("n_phase,B", [(1, 1), (3, 1), (9, 1), (1, 2), (3, 2), (9, 2), (17, 2)])
def test_seeds_against_the_reference(gpu_ctx, orbits, n_phase, B):
    S, P, M = _batch(orbits, range(B))
    tau = np.arange(n_phase) / float(n_phase)
    eps = 1e-3
    r = lto.manifold_seeds(S, P, M, tau, eps=eps, ctx=gpu_ctx)
    assert np.all(r.status == 0) and np.array_equal(r.tau, tau)
    worst = [0.0, 0.0]
    for b in range(B):
        lam, X, V = MR.shared_seeds(orbits, b, n_phase, MU)
        eX, eV = np.abs(r.X[..., b] - X).max(), np.abs(r.V[..., b] - V).max()
        worst = [max(worst[0], eX), max(worst[1], eV)]
        assert abs(r.lam[0, b] - lam[0]) <= H.GPU_LAM_U_REL * abs(lam[0]) and abs(r.lam[1, b] - lam[1]) <= H.GPU_LAM_S_REL * abs(lam[1])
        assert eX <= H.GPU_SEED_X and eV <= H.GPU_SEED_V
        assert np.abs(r.starts[..., b] - MR.starts_of(X, V, eps)).max() <= H.GPU_SEED_X + eps * H.GPU_SEED_V
        assert np.array_equal(r.starts[..., b], MR.starts_of(r.X[..., b], r.V[..., b], eps))      # of the call's own outputs, bit for bit
        assert np.abs(np.linalg.norm(r.V[..., b], axis=0) - 1.0).max() <= 1e-15
    print("n_phase %d, B %d: X %.2e, V %.2e against the reference" % (n_phase, B, *worst))


def test_seeds_batch_equals_singles_repeats_and_wraps_tau(gpu_ctx, orbits):
    S, P, M = _batch(orbits, [0, 1])
    tau = np.arange(9) / 9.0
    r = lto.manifold_seeds(S, P, M, tau, eps=1e-3, ctx=gpu_ctx)
    again = lto.manifold_seeds(S, P, M, tau, eps=1e-3, ctx=gpu_ctx)
    assert _same(r, again)
    for b in range(2):
        one = lto.manifold_seeds(S[:, b], P[b], M[:, :, b], tau, eps=1e-3, ctx=gpu_ctx)
        assert _same((r.lam[:, b], r.X[..., b], r.V[..., b], r.starts[..., b]), (one.lam, one.X, one.V, one.starts))
    a = lto.manifold_seeds(S, P, M, [1.25, -0.75, 3.0], eps=1e-3, ctx=gpu_ctx)
    c = lto.manifold_seeds(S, P, M, [0.25, 0.25, 0.0], eps=1e-3, ctx=gpu_ctx)
    assert np.array_equal(a.tau, [0.25, 0.25, 0.0]) and _same((a.lam, a.X, a.V, a.starts), (c.lam, c.X, c.V, c.starts))
    assert np.all(a.status == 0)


def test_seeds_rk4_against_dop853_and_failed_flights(gpu_ctx, orbits):
    S, P, M = _batch(orbits, [0, 1])
    tau = np.arange(3) / 3.0
    r = lto.manifold_seeds(S, P, M, tau, eps=1e-3, ctx=gpu_ctx)
    k = lto.manifold_seeds(S, P, M, tau, eps=1e-3, integ=lto.integrator(lto.RK4, steps=4000), ctx=gpu_ctx)
    eX, eV = np.abs(k.X - r.X).max(), np.abs(k.V - r.V).max()
    print("RK4 x 4000 against DOP853 on the device: X %.2e, V %.2e" % (eX, eV))
    assert np.all(k.status == 0)
    # the two methods' own distance (H.GPU_RK4_*) on top of what DOP853 itself may be off by
    assert eX <= H.GPU_RK4_X + H.GPU_SEED_X and eV <= H.GPU_RK4_V + H.GPU_SEED_V
    assert np.array_equal(k.lam, r.lam) and np.array_equal(k.X[:, :, 0], r.X[:, :, 0])
    # status 2: max_steps used up, and a period that is not > 0, beside an orbit that stays bitwise what it was
    f = lto.manifold_seeds(S, P, M, tau, eps=1e-3, integ=lto.integrator(max_steps=5), ctx=gpu_ctx)
    assert list(f.status) == [2, 2] and np.all(np.isnan(f.X)) and np.all(np.isnan(f.starts)) and np.all(np.isnan(f.lam))
    g = lto.manifold_seeds(S, np.array([P[0], -1.0]), M, tau, eps=1e-3, ctx=gpu_ctx)
    assert list(g.status) == [0, 2] and np.all(np.isnan(g.V[..., 1]))
    assert _same((g.lam[:, 0], g.X[..., 0], g.V[..., 0], g.starts[..., 0]), (r.lam[:, 0], r.X[..., 0], r.V[..., 0], r.starts[..., 0]))


# ----------------------------------------------------------------------------------------------------------------------- 3. flights
def _arcs(orbits, eps, n):
    """The first n of the 64 vetted starts (+ repeats of the first ones past 64) and their signed t_max."""
    Y, sign = MR.vetted_starts(orbits, eps, MU)
    idx = np.arange(n) % 64
    return np.asfortranarray(Y[:, idx]), sign[idx] * H.T_MAX


def _axis(section):
    return {"x": 0, "y": 1}[section[0]]


def _check_flights(r, Y, T, section, n_cross, sec_dir, bt, bx, tag):
    n = Y.shape[1]
    x_end, t_end, count, dC, status = (np.asarray(r.x_end).reshape(6, n), np.atleast_1d(r.t_end), np.atleast_1d(r.count),
                                       np.atleast_1d(r.dC), np.atleast_1d(r.status))
    et = ex = 0.0
    for i in range(n):
        ref = MR.shared_flight(Y[:, i], T[i], _axis(section), section[1], MU, sec_dir, n_cross)
        assert ref.status == 0
        assert status[i] == 0 and count[i] == ref.count == n_cross, (i, status[i], count[i])
        et, ex = max(et, abs(t_end[i] - ref.t_end)), max(ex, np.abs(x_end[:, i] - ref.x_end).max())
        assert np.sign(t_end[i]) == np.sign(T[i])
    print("%s, %d arcs: t %.2e, x %.2e against the reference; |g| at the end <= %.1e; Jacobi drift <= %.1e"
          % (tag, n, et, ex, np.abs(x_end[_axis(section)] - section[1]).max(), dC.max()))
    assert et <= bt and ex <= bx
    assert dC.max() <= H.GPU_DC
    assert np.abs(x_end[_axis(section)] - section[1]).max() <= 1e-13      # located to adjacent doubles in time


@pytest.mark.parametrize("n", [1, 63, 65])
def test_flights_to_the_second_y0_crossing(gpu_ctx, orbits, n):
    Y, T = _arcs(orbits, H.EPS_Y0, n)
    r = lto.section_flight(Y if n > 1 else Y[:, 0], T if n > 1 else T[0], section=Y0, n_cross=2, ctx=gpu_ctx)
    _check_flights(r, Y, T, Y0, 2, 0, H.GPU_Y0_T, H.GPU_Y0_X, "y = 0, second crossing")


@pytest.mark.parametrize("n", [1, 63, 65])
def test_flights_to_x_1_minus_mu_forward_and_backward(gpu_ctx, orbits, n):
    Y, T = _arcs(orbits, H.EPS_X1MU, max(n, 3))
    if n == 1:                                            # the single arc: a backward one (the batches hold both)
        Y, T = np.asfortranarray(Y[:, 2:3]), T[2:3]
    r = lto.section_flight(Y if n > 1 else Y[:, 0], T if n > 1 else T[0], section=X1MU, n_cross=1, ctx=gpu_ctx)
    _check_flights(r, Y, T, X1MU, 1, 0, H.GPU_X1MU_T, H.GPU_X1MU_X, "x = 1 - MU, first crossing")
    assert n == 1 and T[0] < 0.0 or (np.any(T > 0.0) and np.any(T < 0.0))


@pytest.mark.parametrize("sec_dir", [1, -1])
def test_sec_dir_selects_what_the_reference_selects(gpu_ctx, orbits, sec_dir):
    Y, T = _arcs(orbits, H.EPS_Y0, 64)
    r = lto.section_flight(Y, T, section=Y0, sec_dir=sec_dir, n_cross=1, ctx=gpu_ctx)
    _check_flights(r, Y, T, Y0, 1, sec_dir, H.GPU_Y0_T, H.GPU_Y0_X, "y = 0, first crossing of direction %+d" % sec_dir)
    both = lto.section_flight(Y, T, section=Y0, sec_dir=0, n_cross=1, ctx=gpu_ctx)
    first = np.abs(r.t_end) == np.abs(both.t_end)
    print("direction %+d: the first crossing of %d arcs, a later one of %d" % (sec_dir, first.sum(), (~first).sum()))
    assert first.any() and (~first).any() and np.all(np.abs(r.t_end) >= np.abs(both.t_end))
    vy = r.x_end[4] * np.sign(T)                          # dy/ds along the flight: the sense the flight crosses in
    assert np.all(np.sign(vy) == sec_dir)


def test_batch_equals_singles_and_repeats(gpu_ctx, orbits):
    Y, T = _arcs(orbits, H.EPS_Y0, 65)
    r = lto.section_flight(Y, T, section=Y0, n_cross=2, n_samples=5, ctx=gpu_ctx)
    assert _same(r, lto.section_flight(Y, T, section=Y0, n_cross=2, n_samples=5, ctx=gpu_ctx))
    for b in (0, 3, 63, 64):
        one = lto.section_flight(Y[:, b], T[b], section=Y0, n_cross=2, n_samples=5, ctx=gpu_ctx)
        assert _same((r.x_end[:, b], r.t_end[b], r.count[b], r.dC[b], r.X[:, :, b], r.status[b]), one)
    assert _same((r.x_end[:, 64], r.t_end[64]), (r.x_end[:, 0], r.t_end[0]))


def test_no_section_and_the_next_crossing(gpu_ctx, orbits):
    Y, T = _arcs(orbits, H.EPS_Y0, 64)
    ref = [MR.shared_flight(Y[:, i], T[i], 1, 0.0, MU, 0, 2) for i in range(64)]
    tc = np.array([f.t_end for f in ref])
    # n_cross = 0 flown to the reference's crossing time reproduces its state
    r = lto.section_flight(Y, tc, n_cross=0, ctx=gpu_ctx)
    e = max(np.abs(r.x_end[:, i] - ref[i].x_end).max() for i in range(64))
    print("n_cross = 0 to the reference's crossing time: x %.2e" % e)
    assert np.all(r.status == 0) and np.all(r.count == 0) and np.array_equal(r.t_end, tc) and e <= H.GPU_Y0_X
    # a flight started from a returned crossing state finds the NEXT crossing
    a = lto.section_flight(Y, T, section=Y0, n_cross=1, ctx=gpu_ctx)
    b = lto.section_flight(a.x_end, T - a.t_end, section=Y0, n_cross=1, ctx=gpu_ctx)
    assert np.all(a.status == 0) and np.all(b.status == 0) and np.all(b.count == 1)
    e_t = np.abs(a.t_end + b.t_end - tc).max()
    e_x = max(np.abs(b.x_end[:, i] - ref[i].x_end).max() for i in range(64))
    print("second call from the first crossing: |dt| >= %.3f, t %.2e, x %.2e against the reference's second crossing"
          % (np.abs(b.t_end).min(), e_t, e_x))
    assert np.abs(b.t_end).min() > 0.1 and e_t <= H.GPU_Y0_T and e_x <= H.GPU_Y0_X


@pytest.mark.parametrize("n_samples", [2, 5])
def test_samples_against_the_references_stops(gpu_ctx, orbits, n_samples):
    Y, T = _arcs(orbits, H.EPS_Y0, 64)
    pick = np.arange(0, 64, 5)
    Y, T = np.asfortranarray(Y[:, pick]), T[pick]
    tc = np.array([MR.shared_flight(Y[:, i], T[i], 1, 0.0, MU, 0, 2).t_end for i in range(len(pick))])
    r = lto.section_flight(Y, tc, n_cross=0, n_samples=n_samples, ctx=gpu_ctx)
    e = max(np.abs(r.X[:, :, i] - MR.flight_samples(Y[:, i], tc[i], n_samples, MU)).max() for i in range(len(pick)))
    print("%d samples, %d arcs: %.2e against the reference's stops" % (n_samples, len(pick), e))
    assert np.all(r.status == 0) and e <= H.GPU_SAMPLES
    assert np.array_equal(r.X[:, 0], Y) and np.array_equal(r.X[:, -1], r.x_end)
    # with a section the arc ends between two samples: NaN past its end, and the count carries across the sample intervals
    s = lto.section_flight(Y, 1.25 * tc, section=Y0, n_cross=2, n_samples=n_samples, ctx=gpu_ctx)
    assert np.all(s.status == 0) and np.all(s.count == 2)
    assert np.abs(s.t_end - tc).max() <= H.GPU_Y0_T
    for i in range(len(pick)):
        tk = np.arange(n_samples) * abs(1.25 * tc[i]) / (n_samples - 1)
        past = tk > abs(s.t_end[i])
        assert past.any() and np.all(np.isnan(s.X[:, past, i])) and np.all(np.isfinite(s.X[:, ~past, i]))


def test_statuses_in_a_mixed_batch(gpu_ctx, orbits):
    Y, T = _arcs(orbits, H.EPS_Y0, 64)
    base = lto.section_flight(Y, T, section=X1MU, n_cross=1, ctx=gpu_ctx)
    assert np.all(base.status == 0)
    # t_max = +-0.5 comes first (status 1, the state there), a NaN start (status 2), beside unchanged arcs
    Ym, Tm = Y.copy(), T.copy()
    short, bad = [1, 6, 40], [3, 41]
    Tm[short] = 0.5 * np.sign(T[short])
    Ym[2, bad[0]], Ym[4, bad[1]] = np.nan, np.inf
    r = lto.section_flight(Ym, Tm, section=X1MU, n_cross=1, n_samples=2, ctx=gpu_ctx)
    want = np.zeros(64, dtype=int)
    want[short], want[bad] = 1, 2
    assert np.array_equal(r.status, want)
    for i in short:
        ref = MR.flight(Y[:, i], Tm[i], 0, 1.0 - MU, MU, 0, 0)
        e = np.abs(r.x_end[:, i] - ref.x_end).max()
        print("arc %d stopped at t_max = %+.1f: x %.2e against the reference" % (i, Tm[i], e))
        assert e <= H.GPU_SHORT_X and r.t_end[i] == Tm[i] and r.count[i] == 0
    for i in bad:
        assert np.all(np.isnan(r.x_end[:, i])) and np.isnan(r.t_end[i]) and np.isnan(r.dC[i]) and np.all(np.isnan(r.X[:, :, i]))
    keep = want == 0
    assert _same((r.x_end[:, keep], r.t_end[keep], r.count[keep], r.dC[keep]),
                 (base.x_end[:, keep], base.t_end[keep], base.count[keep], base.dC[keep]))
    # max_steps = 5: no arc gets anywhere
    m = lto.section_flight(Y[:, :3], T[:3], section=X1MU, n_cross=1, integ=lto.integrator(max_steps=5), ctx=gpu_ctx)
    assert np.all(m.status == 2) and np.all(np.isnan(m.x_end)) and np.all(np.isnan(m.t_end))
    # r_min[1] = 0.05: status 3 exactly on the arcs whose reference scan passes within 0.05 of the Moon
    ref = [MR.shared_flight(Y[:, i], T[i], 0, 1.0 - MU, MU, 0, 1) for i in range(64)]
    near = np.array([f.closest[1] < 0.05 for f in ref])
    q = lto.section_flight(Y, T, section=X1MU, n_cross=1, r_min=(0.0, 0.05), ctx=gpu_ctx)
    print("r_min = 0.05: status 3 on %d arcs, the reference's scan on %d" % ((q.status == 3).sum(), near.sum()))
    assert near.any() and (~near).any()
    assert np.array_equal(q.status == 3, near) and np.all(q.status[~near] == 0)
    d_moon = np.sqrt((q.x_end[0] + MU - 1.0) ** 2 + q.x_end[1] ** 2 + q.x_end[2] ** 2)
    assert np.all(d_moon[near] < 0.05) and np.all(np.abs(q.t_end[near]) < np.abs(base.t_end[near]))
    assert _same((q.x_end[:, ~near], q.t_end[~near], q.count[~near]), (base.x_end[:, ~near], base.t_end[~near], base.count[~near]))
    # the Earth's r_min alone changes nothing here
    q1 = lto.section_flight(Y, T, section=X1MU, n_cross=1, r_min=(0.05, 0.0), ctx=gpu_ctx)
    assert _same((q1.x_end, q1.t_end, q1.status), (base.x_end, base.t_end, base.status))


def test_an_arc_that_starts_on_the_section_has_not_crossed_it(gpu_ctx, orbits):
    s0 = orbits[0][0]                                      # y = 0 exactly, vy > 0
    r = lto.section_flight(s0, orbits[0][1], section=Y0, n_cross=1, ctx=gpu_ctx)
    print("from y = 0 exactly: the first crossing at t = %.12f, half a period is %.12f" % (r.t_end, 0.5 * orbits[0][1]))
    assert r.status == 0 and r.count == 1 and abs(r.t_end - 0.5 * orbits[0][1]) < 1e-9


def test_rk4_flights(gpu_ctx, orbits):
    Y, T = _arcs(orbits, H.EPS_Y0, 8)
    d = lto.section_flight(Y, 0.4 * T, section=Y0, n_cross=2, ctx=gpu_ctx)
    k = lto.section_flight(Y, 0.4 * T, section=Y0, n_cross=2, integ=lto.integrator(lto.RK4, steps=4000), ctx=gpu_ctx)
    e_t, e_x = np.abs(k.t_end - d.t_end).max(), np.abs(k.x_end - d.x_end).max()
    print("RK4 x 4000 over 4.8 TU against DOP853 on the device: t %.2e, x %.2e" % (e_t, e_x))
    assert np.all(k.status == 0) and np.all(k.count == 2)
    # what is checked is the crossing search of the fixed-step path, not RK4's truncation: the section is met to adjacent doubles,
    # and the two integrators see the same crossing
    assert np.abs(k.x_end[1]).max() <= 1e-13 and e_t <= 1e-6 and e_x <= 1e-6


# ------------------------------------------------------------------------------------------------------------------------- 4. match
def _random_sets(nA, nB, w):
    """Random states whose best and second-best distances differ by > 1e-9 relative (re-drawn otherwise)."""
    for seed in range(100):
        rng = np.random.RandomState(100 * nA + nB + seed)
        A, Bs = rng.uniform(-1.0, 1.0, (6, nA)), rng.uniform(-1.0, 1.0, (6, nB))
        if MR.second_best_gap(A, Bs, w) > 1e-9:
            return np.asfortranarray(A), np.asfortranarray(Bs)
    raise AssertionError("no well-separated draw")


@pytest.mark.parametrize("nA,nB", [(1, 1), (3, 257), (65, 64)])
@pytest.mark.parametrize("w", [1.0, 0.3])
def test_match_against_numpy(gpu_ctx, nA, nB, w):
    A, Bs = _random_sets(nA, nB, w)
    idx, d, dr, dv = MR.match(A, Bs, w)
    r = lto.state_match(A, Bs, w=w, ctx=gpu_ctx)
    assert np.array_equal(r.index, idx)
    assert np.array_equal(r.dist, d) and np.array_equal(r.dr, dr) and np.array_equal(r.dv, dv)      # the header's order: bit for bit
    one = lto.state_match(A[:, 0], Bs, w=w, ctx=gpu_ctx)
    assert one == (r.index[0], r.dist[0], r.dr[0], r.dv[0])


def test_match_ties_and_nan(gpu_ctx):
    A, Bs = _random_sets(65, 300, 1.0)
    Bs = Bs.copy()
    idx, _, _, _ = MR.match(A, Bs, 1.0)
    Bs[:, 290] = Bs[:, idx[0]]                             # a duplicate of row 0's winner at a higher index, one at a lower
    lo = 0 if idx[0] > 0 else None
    if lo is not None:
        Bs[:, lo] = Bs[:, idx[0]]
    Bs[:, 7] = np.nan                                      # a NaN column never wins
    Bs[3, 260] = np.nan
    want, d, dr, dv = MR.match(A, Bs, 1.0)
    r = lto.state_match(A, Bs, ctx=gpu_ctx)
    assert np.array_equal(r.index, want) and np.array_equal(r.dist, d)
    assert r.index[0] == (lo if lo is not None else idx[0]) and not np.any(np.isin(r.index, [7, 260]))
    An = A.copy()
    An[1, 5] = np.nan                                      # a row of A with a NaN: every distance NaN
    r = lto.state_match(An, Bs, ctx=gpu_ctx)
    assert r.index[5] == -1 and np.isnan(r.dist[5]) and np.isnan(r.dr[5]) and np.isnan(r.dv[5])
    keep = np.arange(65) != 5
    assert np.array_equal(r.index[keep], want[keep]) and np.array_equal(r.dist[keep], d[keep])
    r = lto.state_match(A, Bs * np.nan, ctx=gpu_ctx)       # an all-NaN Bs
    assert np.all(r.index == -1) and np.all(np.isnan(r.dist))
    z = lto.state_match(A, Bs, w=0.0, ctx=gpu_ctx)         # w = 0: positions alone
    assert np.array_equal(z.index, MR.match(A, Bs, 0.0)[0]) and np.array_equal(z.dist, z.dr)


# ----------------------------------------------------------------------------------------------------------------------- 5. drivers
def test_halo_manifold_driver(gpu_ctx, orbits):
    a = drivers.halo_manifold(orbits[0], 8, eps=1e-3, section=Y0, n_cross=2, t_max=H.T_MAX, ctx=gpu_ctx)
    assert a.x_end.shape == (6, 32) and np.all(a.status == 0) and np.all(a.count == 2)
    assert list(a.branch[:4]) == ["u+", "u-", "s+", "s-"] and np.array_equal(a.tau, np.repeat(np.arange(8) / 8.0, 4))
    assert np.all(a.t_end[0::4] > 0.0) and np.all(a.t_end[1::4] > 0.0) and np.all(a.t_end[2::4] < 0.0) and np.all(a.t_end[3::4] < 0.0)
    Y, sign = MR.vetted_starts(orbits, 1e-3, MU)
    assert np.abs(a.start - Y[:, :32]).max() <= H.GPU_SEED_X + 1e-3 * H.GPU_SEED_V
    s = drivers.halo_manifold(orbits[0], 8, eps=1e-3, branches="s-u+", section=Y0, n_cross=2, ctx=gpu_ctx)
    assert s.x_end.shape == (6, 16) and np.array_equal(s.x_end[:, 0::2], a.x_end[:, 3::4]) and np.array_equal(s.x_end[:, 1::2], a.x_end[:, 0::4])
    halo = drivers.halo_orbit(orbits[0][0], "x0", ctx=gpu_ctx)          # the record halo_orbit returns is taken as it is
    h = drivers.halo_manifold(halo, 8, eps=1e-3, section=Y0, n_cross=2, ctx=gpu_ctx)
    assert np.all(h.status == 0) and np.abs(h.t_end - a.t_end).max() < 1e-6


def test_manifold_connections_and_guess(gpu_ctx, orbits):
    k = 10
    con = drivers.manifold_connections(orbits[0], orbits[1], section=Y0, n_phase=8, eps=1e-3, n_cross=2, w=1.0, k=k, ctx=gpu_ctx)
    assert len(con) == k
    dist = [c.dist for c in con]
    assert dist == sorted(dist)
    for c in con:
        dr, dv = np.linalg.norm(c.x1[:3] - c.x2[:3]), np.linalg.norm(c.x1[3:] - c.x2[3:])
        assert abs(c.dr_km - dr * DU) <= 1e-9 * DU and abs(c.dv_ms - dv * DU / TU * 1e3) <= 1e-9 * DU / TU * 1e3
        assert abs(c.dist - np.hypot(dr, dv)) <= 1e-12 and c.t1 > 0.0 and c.t2 < 0.0
        assert c.branch1 in ("u+", "u-") and c.branch2 in ("s+", "s-") and abs(c.x1[1]) <= 1e-13 and abs(c.x2[1]) <= 1e-13
    print("best pair: dr %.1f km, dv %.2f m/s, phases %.3f -> %.3f, %s -> %s, flight times %.3f and %.3f TU"
          % (con[0].dr_km, con[0].dv_ms, con[0].tau1, con[0].tau2, con[0].branch1, con[0].branch2, con[0].t1, con[0].t2))
    # the nearest partner of every departure arc, recomputed by numpy from the two tubes
    a = drivers.halo_manifold(orbits[0], 8, eps=1e-3, branches="u+u-", section=Y0, n_cross=2, ctx=gpu_ctx)
    b = drivers.halo_manifold(orbits[1], 8, eps=1e-3, branches="s+s-", section=Y0, n_cross=2, ctx=gpu_ctx)
    _, d, _, _ = MR.match(a.x_end, b.x_end, 1.0)
    assert np.allclose(sorted(d)[:k], dist, rtol=0.0, atol=1e-15)
    n_nodes = 30
    X, t, tau1, tau2 = drivers.manifold_guess(con[0], n_nodes, ctx=gpu_ctx)
    assert X.shape == (6, n_nodes) and t.shape == (n_nodes,) and np.all(np.isfinite(X)) and np.all(np.diff(t) > 0.0)
    assert t[0] == 0.0 and abs(t[-1] - (con[0].t1 - con[0].t2)) <= 1e-12 and (tau1, tau2) == (con[0].tau1, con[0].tau2)
    # the end nodes lie eps from the two orbits' points at the phases (the orbits re-tabled by the reference)
    for node, k_orb, tau in ((X[:, 0], 0, tau1), (X[:, -1], 1, tau2)):
        _, Xr, _ = MR.shared_seeds(orbits, k_orb, 8, MU)
        j = int(round(tau * 8))
        gap = np.linalg.norm(node - Xr[:, 0 if k_orb == 0 else 1, j])
        print("end node on orbit %d at tau = %.3f: %.6e from the orbit (eps = 1e-3)" % (k_orb + 1, tau, gap))
        assert abs(gap - 1e-3) <= 1e-3 * 1e-6
