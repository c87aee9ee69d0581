"""GPU checks of the periodic-orbit generator (lto_halo_correct_batch, lto_halo_table_batch) against the independent
host reference (tests/halo_reference.py: scipy DOP853 on the 42-component system at rtol 1e-13).  The bounds are the issue's:
corrected unknowns and period 1e-11 (about 70 x the reference's own 1.4e-13 spread), the project's flow bar 1e-10 for the device's
orbit re-flown by scipy, table states 1e-10, M 1e-9 max |M|, nu 1e-7, closure 1e-10, Jacobi drift 1e-11, 1e-7 against the packaged
tables (which are good to 8 digits); tests/test_halo_host.py holds the reference's own spread to a tenth of each.

Figures measured on an MI355X are in DESIGN 4.25."""
import os
import sys

import numpy as np
import pytest
from scipy.integrate import solve_ivp

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import halo_reference as HR  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU, day  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = {"z0": HR.HOLD_Z0, "x0": HR.HOLD_X0, "planar": HR.PLANAR}


@pytest.fixture(scope="module")
def packaged():
    return [np.asarray(tb[:6], dtype=float) for tb in synth.halo_orbits()]


def _halo_seeds(packaged, mode="x0"):
    """17 seeds: the two packaged ones and perturbed copies (<= 1e-4 in position, <= 1e-3 in vy0), vetted on the host."""
    return HR.gpu_seeds([HR.seed_of(p) for p in packaged], mode)


def _planar_seeds():
    """Lyapunov seeds at L1 and L2 with the vetted amplitudes HR.PLANAR_AX, repeated to 17."""
    six = [drivers.lyapunov_seed(w, ax, MU)[0] for ax in HR.PLANAR_AX for w in (1, 2)]
    return np.array([six[k % 6] for k in range(17)]).T


_REF = {}


def _ref_correct(seed, mode):
    """The reference's corrector on one seed, computed once and shared (never modified)."""
    key = (mode, tuple(seed))
    if key not in _REF:
        _REF[key] = HR.correct(seed, MODES[mode], MU)
    return _REF[key]


def _ref_table(state, period, n):
    key = ("table", n, tuple(state), period)
    if key not in _REF:
        _REF[key] = HR.table(state, period, n, MU)
    return _REF[key]


def _reflown(state, period):
    """The state at P / 2 of the device's orbit by scipy."""
    s = solve_ivp(HR.rhs42(MU), (0.0, 0.5 * period), HR.start42(state), method="DOP853", rtol=HR.RTOL, atol=HR.ATOL)
    return s.y[:6, -1]


@pytest.mark.parametrize("B", [1, 9, 17])
@pytest.mark.parametrize("mode", ["z0", "x0", "planar"])
def test_corrector_against_the_reference(gpu_ctx, packaged, mode, B):
    seeds = (_planar_seeds() if mode == "planar" else _halo_seeds(packaged, mode))[:, :B]
    r = lto.halo_correct(seeds if B > 1 else seeds[:, 0], mode, ctx=gpu_ctx)
    state = np.asarray(r.state).reshape(6, B)
    period, its, status = np.atleast_1d(r.period), np.atleast_1d(r.iterations), np.atleast_1d(r.status)
    hist = np.asarray(r.history).reshape(-1, B)
    worst = [0.0, 0.0, 0.0]
    for b in range(B):
        ref = _ref_correct(seeds[:, b], mode)
        assert ref.status == 0
        e_state, e_P = np.abs(state[:, b] - ref.state).max(), abs(period[b] - ref.period)
        back = _reflown(state[:, b], period[b])
        flow = max(abs(back[1]), abs(back[3]), abs(back[5]))
        worst = [max(worst[0], e_state), max(worst[1], e_P), max(worst[2], flow)]
        print("%s B=%d b=%d: state %.2e, P %.2e, iterations %d (reference %d), re-flown |y|,|vx|,|vz| %.2e" % (
            mode, B, b, e_state, e_P, its[b], ref.iterations, flow))
        assert status[b] == 0
        assert e_state <= 1e-11 and e_P <= 1e-11
        assert HR.same_count(its[b], ref.iterations, ref.history, 1e-12), (b, its[b], ref.history)
        assert flow <= 1e-10
        assert state[1, b] == 0.0 and state[3, b] == 0.0 and state[5, b] == 0.0
        n = int(its[b]) + 1                                # the history: one residual per flight, NaN past the last
        assert np.all(np.isfinite(hist[:n, b])) and np.all(np.isnan(hist[n:, b])) and hist[n - 1, b] < 1e-12
    print("%s B=%d worst: state %.2e, P %.2e, re-flown %.2e" % (mode, B, *worst))


@pytest.mark.parametrize("mode", ["z0", "x0", "planar"])
def test_corrector_batch_equals_singles_and_repeats(gpu_ctx, packaged, mode):
    seeds = (_planar_seeds() if mode == "planar" else _halo_seeds(packaged, mode))[:, :9]
    rb = lto.halo_correct(seeds, mode, ctx=gpu_ctx)
    again = lto.halo_correct(seeds, mode, ctx=gpu_ctx)
    for f in rb._fields:
        assert np.array_equal(getattr(rb, f), getattr(again, f), equal_nan=True), f
    for b in (0, 7, 8):                                    # both wavefronts of the batch
        r1 = lto.halo_correct(seeds[:, b], mode, ctx=gpu_ctx)
        assert np.array_equal(rb.state[:, b], r1.state) and rb.period[b] == r1.period and rb.resid[b] == r1.resid
        assert rb.iterations[b] == r1.iterations and np.array_equal(rb.history[:, b], r1.history, equal_nan=True)


def _orbits(packaged, B):
    """(state0 [6 x B], P [B]) of the reference's corrected orbits (hold x0) from the first B seeds."""
    refs = [_ref_correct(s, "x0") for s in _halo_seeds(packaged)[:, :B].T]
    return np.array([r.state for r in refs]).T, np.array([r.period for r in refs])


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("n", [2, 3, 100])
def test_table_against_the_reference(gpu_ctx, packaged, n, B):
    state0, P = _orbits(packaged, B)
    r = lto.halo_table(state0 if B > 1 else state0[:, 0], P if B > 1 else P[0], n, ctx=gpu_ctx)
    X = np.asarray(r.X).reshape(6, n, B)
    M = np.asarray(r.M).reshape(6, 6, B)
    closure, status = np.atleast_1d(r.closure), np.atleast_1d(r.status)
    jac, nu = np.asarray(r.jacobi).reshape(2, B), np.asarray(r.nu).reshape(2, B)
    assert np.array_equal(r.times, np.arange(n) / (n - 1.0))              # i / (n - 1): LinRange(0, 1, n) to the last bit or the one before
    assert np.abs(r.times - np.linspace(0.0, 1.0, n)).max() <= 2.3e-16
    for b in range(B):
        assert status[b] == 0
        assert np.array_equal(X[:, 0, b], state0[:, b])
        assert closure[b] == np.abs(X[:, -1, b] - X[:, 0, b]).max()          # the last column is the integrated state
        print("n=%d B=%d b=%d: closure %.2e, C = %.9f, drift %.2e, nu %s" % (n, B, b, closure[b], jac[0, b], jac[1, b], nu[:, b]))
        assert closure[b] <= 1e-10
        assert abs(jac[0, b] - HR.jacobi(state0[:, b], MU)) <= 1e-13 and jac[1, b] <= 1e-11
        if n == 100 and b >= 2:                            # the reference's 100-sample table: the two packaged orbits
            continue
        Xr, Mr = _ref_table(state0[:, b], P[b], n)
        e_X, e_M = np.abs(X[:, :, b] - Xr).max(), np.abs(M[:, :, b] - Mr).max() / np.abs(Mr).max()
        e_nu = np.abs(nu[:, b] - HR.nu_from_traces(Mr)).max()
        print("    states %.2e, M rel %.2e, nu %.2e" % (e_X, e_M, e_nu))
        assert e_X <= 1e-10 and e_M <= 1e-9 and e_nu <= 1e-7
        assert np.abs(nu[:, b] - HR.nu_from_eigenvalues(M[:, :, b])).max() <= 1e-7
        if n == 100:
            e_pack = np.abs(X[:, :, b] - packaged[b]).max()
            print("    against the packaged table %.2e" % e_pack)
            assert e_pack <= 1e-7


def test_table_batch_equals_singles_and_repeats(gpu_ctx, packaged):
    state0, P = _orbits(packaged, 9)
    rb = lto.halo_table(state0, P, 7, ctx=gpu_ctx)
    again = lto.halo_table(state0, P, 7, ctx=gpu_ctx)
    for f in rb._fields:
        assert np.array_equal(getattr(rb, f), getattr(again, f), equal_nan=True), f
    for b in (1, 8):
        r1 = lto.halo_table(state0[:, b], P[b], 7, ctx=gpu_ctx)
        assert np.array_equal(rb.X[:, :, b], r1.X) and np.array_equal(rb.M[:, :, b], r1.M)
        assert rb.closure[b] == r1.closure and np.array_equal(rb.jacobi[:, b], r1.jacobi) and np.array_equal(rb.nu[:, b], r1.nu)


def _same_as_single(rb, b, r1):
    return (np.array_equal(rb.state[:, b], r1.state, equal_nan=True) and rb.period[b] == r1.period and rb.resid[b] == r1.resid
            and rb.iterations[b] == r1.iterations and rb.status[b] == r1.status
            and np.array_equal(rb.history[:, b], r1.history, equal_nan=True))


def test_statuses_in_a_mixed_batch(gpu_ctx, packaged):
    s1, s2 = (HR.seed_of(p) for p in packaged)
    nan_seed, still = s1.copy(), s2.copy()
    nan_seed[0] = np.nan
    still[4] = 0.0
    seeds = np.array([s1, nan_seed, s2, still, HR.perturbed(s1, 3)]).T
    rb = lto.halo_correct(seeds, "x0", ctx=gpu_ctx)
    assert list(rb.status) == [0, 2, 0, 2, 0]
    for b in (1, 3):                                        # no numbers from an unusable seed
        assert np.all(np.isnan(rb.state[:, b])) and np.isnan(rb.period[b]) and np.isnan(rb.resid[b])
        assert rb.iterations[b] == 0 and np.all(np.isnan(rb.history[:, b]))
    for b in (0, 2, 4):
        assert _same_as_single(rb, b, lto.halo_correct(seeds[:, b], "x0", ctx=gpu_ctx))

    # planar mode: z0 != 0 is refused next to a Lyapunov seed
    lyap = drivers.lyapunov_seed(2, 1e-3, MU)[0]
    rp = lto.halo_correct(np.array([lyap, s1]).T, "planar", ctx=gpu_ctx)
    assert list(rp.status) == [0, 2] and np.all(np.isnan(rp.state[:, 1]))
    assert _same_as_single(rp, 0, lto.halo_correct(lyap, "planar", ctx=gpu_ctx))

    # t_max between the two half periods (1.454 and 1.565): orbit 2 finds no crossing
    rt = lto.halo_correct(np.array([s1, s2]).T, "x0", t_max=1.5, ctx=gpu_ctx)
    assert list(rt.status) == [0, 2] and np.isnan(rt.period[1])
    assert _same_as_single(rt, 0, lto.halo_correct(s1, "x0", t_max=1.5, ctx=gpu_ctx))

    # max_iter = 0 evaluates the seed: status 1 for a rough one, 0 for one that already meets the tolerance
    good = rb.state[:, 0]
    r0 = lto.halo_correct(np.array([s2, good]).T, "x0", max_iter=0, ctx=gpu_ctx)
    assert list(r0.status) == [1, 0] and list(r0.iterations) == [0, 0] and r0.history.shape == (1, 2)
    assert np.array_equal(r0.state[:, 0], s2) and abs(r0.resid[0] - _ref_correct(s2, "x0").history[0]) < 1e-11
    assert r0.history[0, 0] == r0.resid[0] and r0.resid[1] < 1e-12
    assert _same_as_single(r0, 1, lto.halo_correct(good, "x0", max_iter=0, ctx=gpu_ctx))

    # steps used up: status 2 (the corrector) and 2 (the table), nothing but NaN
    rs = lto.halo_correct(np.array([s1, s2]).T, "x0", integ=lto.integrator(max_steps=5), ctx=gpu_ctx)
    assert list(rs.status) == [2, 2] and np.all(np.isnan(rs.state))
    tb = lto.halo_table(np.array([good, good]).T, np.array([rb.period[0], -1.0]), 3, ctx=gpu_ctx)
    assert list(tb.status) == [0, 2] and np.all(np.isnan(tb.X[:, 1:, 1])) and np.all(np.isnan(tb.nu[:, 1]))


def test_rk4_agrees_with_dop853(gpu_ctx, packaged):
    s1 = HR.seed_of(packaged[0])
    a = lto.halo_correct(s1, "x0", ctx=gpu_ctx)
    # 4 000 steps over t_max = 2.9 = two half periods: 2 000 steps per half period
    r = lto.halo_correct(s1, "x0", t_max=2.9, integ=lto.integrator(lto.RK4, steps=4000), ctx=gpu_ctx)
    e = max(np.abs(a.state - r.state).max(), abs(a.period - r.period))
    print("corrector RK4 x 2000 per half period against DOP853: %.2e" % e)
    assert r.status == 0 and e <= 1e-9
    ta = lto.halo_table(a.state, a.period, 3, ctx=gpu_ctx)
    tr = lto.halo_table(a.state, a.period, 3, integ=lto.integrator(lto.RK4, steps=2000), ctx=gpu_ctx)
    e_X, e_M = np.abs(ta.X - tr.X).max(), np.abs(ta.M - tr.M).max() / np.abs(ta.M).max()
    print("table RK4 x 2000 per half period against DOP853: states %.2e, M rel %.2e" % (e_X, e_M))
    assert tr.status == 0 and e_X <= 1e-9 and e_M <= 1e-9


def test_refusals(gpu_ctx, packaged):
    s1 = HR.seed_of(packaged[0])
    for method in (lto.RKF78_FIXED, lto.RKF78_ADAPTIVE):
        integ = lto.integrator(method, steps=10)
        with pytest.raises(lto.LtoError) as ei:
            lto.halo_correct(s1, "x0", integ=integ, ctx=gpu_ctx)
        assert ei.value.code == -3
        with pytest.raises(lto.LtoError) as ei:
            lto.halo_table(s1, 2.9, 5, integ=integ, ctx=gpu_ctx)
        assert ei.value.code == -3
    for kw in ({"tol": 0.0}, {"t_max": 0.0}, {"t_max": np.inf}, {"MU": 1.5}, {"sing_tol": 1.0}, {"integ": lto.integrator(lto.RK4, steps=0)}):
        with pytest.raises(lto.LtoError) as ei:
            lto.halo_correct(s1, "x0", ctx=gpu_ctx, **kw)
        assert ei.value.code == -1, kw
    fn, h = gpu_ctx.fn("halo_correct_batch"), gpu_ctx.handle
    assert fn(h, 0, MU, 0, None, 1e-12, 15, 10.0, 1e-12, None, None, None, None, None, None, None) == -1
    assert fn(h, 1, MU, 0, None, 1e-12, 15, 10.0, 1e-12, None, None, None, None, None, None, None) == -2
    ft = gpu_ctx.fn("halo_table_batch")
    assert ft(h, 1, 1, MU, None, None, None, None, None, None, None, None, None, None) == -1
    assert ft(h, 2, 1, MU, None, None, None, None, None, None, None, None, None, None) == -2
    assert lto.halo_correct(s1, "x0", ctx=gpu_ctx).status == 0        # the context is fine afterwards
    assert gpu_ctx.lib.lto_last_call_ms(gpu_ctx.handle) > 0.0


@pytest.fixture(scope="module")
def march(gpu_ctx, packaged):
    first = lto.halo_correct(HR.seed_of(packaged[0]), "x0", ctx=gpu_ctx)
    values = np.linspace(packaged[0][0, 0], packaged[1][0, 0], 9)[1:]
    return first, values, drivers.halo_family(first.state, values, hold="x0", ctx=gpu_ctx)


def test_family_march_reaches_orbit_2(gpu_ctx, packaged, march):
    first, values, fam = march
    print("march: iterations %s, periods %s" % (list(fam.iterations), fam.period))
    assert np.all(fam.status == 0) and np.array_equal(fam.states[0], values)
    assert np.abs(fam.states[:, -1] - HR.seed_of(packaged[1])).max() <= 1e-7
    # two families side by side: the same march twice in one call per member
    two = drivers.halo_family(np.array([first.state, first.state]).T, values, hold="x0", ctx=gpu_ctx)
    assert np.array_equal(two.states[:, :, 0], fam.states) and np.array_equal(two.states[:, :, 1], fam.states)


def test_family_fill(gpu_ctx, march):
    first, values, fam = march
    members = np.column_stack([first.state, fam.states])
    fill = drivers.halo_family_fill(members, 3, ctx=gpu_ctx)
    assert fill.state.shape == (6, 24) and np.all(fill.status == 0)
    assert np.all(np.diff(fill.state[0]) > 0.0) and np.all(fill.iterations <= 4)


def test_direct_transfer_between_generated_orbits(gpu_ctx, packaged):
    """The direct demo transfer (30 nodes, 20 days, flagEnd = false) between tables from halo_orbit and between the packaged ones."""
    times = np.linspace(0.0, 1.0, 100)
    gen = [drivers.halo_orbit(HR.seed_of(p), "x0", n_samples=100, ctx=gpu_ctx) for p in packaged]
    assert all(g.status == 0 for g in gen)

    def solve(t0s, X0s, tfs, Xfs):
        n, tof = 30, 10.0 * day / TU
        X, t, tau1, tau2 = drivers.stacked_guess(n, tof, tof, 0.75, t0s, X0s, tfs, Xfs, MU, ctx=gpu_ctx)
        drivers.multiShoot_CRTBP_direct(X, np.zeros((3, n)), tau1, tau2, t, np.zeros(3), np.zeros(3), MU, DU, TU, n, 10, 1000.0, 2000.0,
                                        t0s, X0s, tfs, Xfs, False, False, 0.0, False, 100, verbose=False)
        last = drivers.multiShoot_CRTBP_direct.last
        return last["status"], last["iterations"]

    st_gen, it_gen = solve(gen[0].times, gen[0].states, gen[1].times, gen[1].states)
    st_pack, it_pack = solve(times, packaged[0], times, packaged[1])
    print("direct demo transfer: generated tables status %d after %d iterations, packaged tables status %d after %d" % (
        st_gen, it_gen, st_pack, it_pack))
    assert st_gen == st_pack == 0
