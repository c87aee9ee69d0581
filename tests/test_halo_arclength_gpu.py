"""GPU checks of the pseudo-arclength continuation (lto_halo_arclength_batch) against the independent host reference
(tests/halo_arclength_reference.py: the same rule in numpy on scipy's DOP853 at rtol 1e-13 / atol 1e-14).

Bounds.  Device against reference, per case class on (states, tangents, periods, det relative): ten times the reference's own spread
between (1e-13, 1e-14) and (1e-11, 1e-12) over the class's cases, rounded up to a power of ten (halo_arclength_reference.BOUNDS, with
the spreads; tests/test_halo_arclength_host.py holds the spread to a tenth and vets every input as far from a decision's edge).  Only
states, tangents, det, periods, iteration counts, ds_out and halvings are compared with the reference.  The step sizes and halving
counts must be the reference's exactly, and so must an iteration count unless a residual of the reference's run lies within
[tol / 10, 10 tol] (halo_reference.same_count): there it may differ by one.

  class        spread state / tangent / period / det        bound                          device (MI355X, worst of B = 1, 9, 17)
  planar       1.4e-14 / 6.6e-13 / 3.3e-12 / 5.1e-11        1e-12 / 1e-11 / 1e-10 / 1e-9   6.7e-16 / 8.7e-15 / 4.6e-13 / 1.6e-12
  lyapunov3    3.8e-15 / 1.1e-13 / 3.1e-12 / 4.7e-10        1e-13 / 1e-11 / 1e-10 / 1e-8   6.7e-16 / 6.7e-15 / 4.6e-13 / 6.5e-11
  switch       1.1e-12 / 3.4e-10 / 6.2e-13 / 2.2e-11        1e-10 / 1e-8 / 1e-11 / 1e-9    1.6e-14 / 1.9e-10 / 1.4e-13 / 8.9e-12
  halo_L2      2.5e-13 / 3.4e-12 / 7.2e-13 / 2.1e-11        1e-11 / 1e-10 / 1e-11 / 1e-9   1.1e-14 / 2.8e-12 / 1.4e-13 / 4.3e-12
  halo_L1      1.1e-11 / 2.5e-09 / 4.7e-11 / 2.4e-09        1e-9 / 1e-7 / 1e-9 / 1e-7      2.0e-13 / 3.6e-11 / 9.8e-13 / 3.0e-11

RK4 with 2 000 steps per half period against DOP853 on the planar L2 march: 2.4e-12 (bound 1e-9, DESIGN 4.25's).  The driver chain
from MU alone: branch point C and P 2.8e-14 / 7.8e-14 from the reference driver's, the 25 members within 9.7e-13.

Properties that need no reference: an orbit of a batch equals its single call bit for bit, repeated calls are identical, and member
k equals the one-member call from member k - 1's state and tangent by member k's ds_out."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import halo_reference as HR  # noqa: E402
import halo_arclength_reference as AR  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-12
CASE_NAMES = ["planar_L1", "planar_L2", "lyapunov3_L2", "switch_L2_north_0.001", "switch_L2_north_0.01", "switch_L2_south_0.001",
              "switch_L2_south_0.01", "halo_L2", "halo_L1"]
FIELDS = lto.HaloArclength._fields
_REF = {}


def _call(gpu_ctx, case, B, **kw):
    seeds = case.seeds[:, :B] if B > 1 else case.seeds[:, 0]
    return lto.halo_arclength(seeds, case.K, case.ds, case.dir0, planar=case.planar, dir_is_tangent=case.tangent, tol=TOL, ctx=gpu_ctx, **kw)


def _against(r, b, ref, bound, label):
    """Orbit b of a device result [.. x K x B] against the reference's members; returns the largest differences."""
    worst = np.zeros(4)
    for k, m in enumerate(ref):
        assert m.status == 0 and r.status[k, b] == 0, (label, k, b, r.status[k, b])
        e = np.array([np.abs(r.state[:, k, b] - m.state).max(), np.abs(r.tangent[:, k, b] - m.tangent).max(), abs(r.period[k, b] - m.period),
                      abs(r.det[k, b] - m.det) / abs(m.det)])
        worst = np.maximum(worst, e)
        assert np.all(e <= np.array(bound)), (label, k, b, e, bound)
        assert HR.same_count(r.iterations[k, b], m.iterations, m.history, TOL), (label, k, b, r.iterations[k, b], m.iterations, m.history)
        assert r.ds[k, b] == m.ds and r.halvings[k, b] == m.halvings, (label, k, b, r.ds[k, b], m.ds, r.halvings[k, b], m.halvings)
        assert r.resid[k, b] < TOL and abs(r.jacobi[k, b] - HR.jacobi(r.state[:, k, b], MU)) <= 1e-14
        assert r.state[1, k, b] == 0.0 and r.state[3, k, b] == 0.0 and r.state[5, k, b] == 0.0
        assert abs(np.linalg.norm(r.tangent[:, k, b]) - 1.0) <= 1e-15
        n = int(r.iterations[k, b]) + 1                    # the history: one residual per flight of the accepted attempt, NaN past it
        assert np.all(np.isfinite(r.history[:n, k, b])) and np.all(np.isnan(r.history[n:, k, b])) and r.history[n - 1, k, b] == r.resid[k, b]
    return worst


@pytest.mark.parametrize("B", [1, 9, 17])
@pytest.mark.parametrize("name", CASE_NAMES)
def test_march_against_the_reference(gpu_ctx, name, B):
    case = AR.cases(MU)[name]
    r = _call(gpu_ctx, case, B)
    if B == 1:
        assert r.state.shape == (6, case.K) and r.tangent.shape == (3, case.K) and r.history.shape == (16, case.K) and r.det.shape == (case.K,)
        r = lto.HaloArclength(*[np.asarray(v)[..., None] for v in r])
    assert r.state.shape == (6, case.K, B) and r.history.shape == (16, case.K, B) and r.halvings.shape == (case.K, B)
    bound = AR.BOUNDS[case.cls]
    worst = np.zeros(4)
    for b in range(B):
        ref = AR.case_march(case, b, MU)
        worst = np.maximum(worst, _against(r, b, ref, bound, name))
        # det changes sign between the same members as the reference's
        assert drivers._sign_changes(r.det[:, b]) == AR.family_bifurcations(ref), (name, b)
        if case.planar or name.startswith("lyapunov3"):
            assert np.all(r.state[2, :, b] == 0.0) and np.all(r.tangent[1, :, b] == 0.0)
        if case.tangent and name.startswith("switch"):      # the step off the plane moves z0 by ds exactly
            assert abs(r.state[2, 0, b] - (case.seeds[2, b] + case.ds * case.dir0[1])) <= 1e-15
    print("%s B=%d worst: state %.2e tangent %.2e period %.2e det %.2e (bounds %s)" % ((name, B) + tuple(worst) + (bound,)))
    if name == "lyapunov3_L2":
        assert drivers._sign_changes(r.det[:, 0]) == [13]
    if name == "halo_L2":
        fam = drivers.HaloFamily(r.state[:, :, 0], r.period[:, 0], r.resid[:, 0], r.iterations[:, 0], r.status[:, 0], r.tangent[:, :, 0],
                                 r.det[:, 0], r.ds[:, 0])
        assert drivers.family_folds(fam) == {"x0": AR.family_folds(AR.case_march(case, 0, MU), 0), "z0": [12], "vy0": AR.family_folds(
            AR.case_march(case, 0, MU), 2)}


def _step_call(gpu_ctx, case, b=None, **over):
    kw = dict(case.kw, **over)
    sl = slice(None) if b is None else b
    seeds, dirs, ds0 = case.seeds[:, sl], case.dir0[:, sl], case.ds0[sl]
    if b is None and case.seeds.shape[1] == 1:
        seeds, dirs, ds0 = seeds[:, 0], dirs[:, 0], ds0[0]
    return lto.halo_arclength(seeds, case.K, ds0, dirs, planar=case.planar, dir_is_tangent=case.tangent, tol=TOL, ctx=gpu_ctx, **kw)


def _batched(r):
    return r if r.status.ndim == 2 else lto.HaloArclength(*[np.asarray(v)[..., None] for v in r])


@pytest.mark.parametrize("name", ["halve", "grow", "nogrow"])
def test_step_control_against_the_reference(gpu_ctx, name):
    case = AR.step_cases(MU)[name]
    r = _batched(_step_call(gpu_ctx, case))
    ref, _ = AR.step_march(case, 0, MU)
    print("%s: ds_out %s halvings %s iterations %s (reference %s %s %s)" % (
        name, list(r.ds[:, 0]), list(r.halvings[:, 0]), list(r.iterations[:, 0]), [m.ds for m in ref], [m.halvings for m in ref],
        [m.iterations for m in ref]))
    worst = _against(r, 0, ref, AR.BOUNDS[case.cls], name)
    print("%s worst: state %.2e tangent %.2e period %.2e det %.2e" % ((name,) + tuple(worst)))
    if name == "halve":
        assert list(r.halvings[:, 0]) == [1, 1] and list(r.ds[:, 0]) == [0.08, 0.04]
    elif name == "grow":
        assert list(r.ds[:, 0]) == [0.0, 0.005, 0.005 * 1.5, 0.005 * 1.5 * 1.5, 0.012, 0.012]
    else:
        assert list(r.ds[:, 0]) == [0.0] + [0.005] * 5


def _none(r, k, b):
    return (np.all(np.isnan(r.state[:, k, b])) and np.all(np.isnan(r.tangent[:, k, b])) and np.isnan(r.det[k, b]) and np.isnan(r.period[k, b])
            and np.isnan(r.jacobi[k, b]) and np.isnan(r.resid[k, b]))


def _same(ra, ka, ba, rb, kb, bb, skip=()):
    """Member (ka, ba) of one batched result against member (kb, bb) of another, bit for bit."""
    return all(np.array_equal(getattr(ra, f)[..., ka, ba], getattr(rb, f)[..., kb, bb], equal_nan=True) for f in FIELDS if f not in skip)


def test_ds_min_ends_one_family_beside_an_unchanged_neighbour(gpu_ctx):
    case = AR.step_cases(MU)["dsmin"]
    r = _step_call(gpu_ctx, case)
    refs = [AR.step_march(case, b, MU)[0] for b in range(2)]
    assert list(r.status[:, 0]) == [4, 2, 2] == [m.status for m in refs[0]] and list(r.halvings[:, 0]) == [0, 0, 0]
    assert r.ds[0, 0] == 0.02 and np.all(np.isnan(r.ds[1:, 0])) and all(_none(r, k, 0) for k in range(3))
    assert np.all(np.isnan(r.history[:, 1:, 0])) and np.all(r.iterations[1:, 0] == 0)
    # the attempt that was refused did converge: its history is kept
    n = int(r.iterations[0, 0]) + 1
    assert HR.same_count(n - 1, refs[0][0].iterations, refs[0][0].history, TOL)
    assert np.all(np.isfinite(r.history[:n, 0, 0])) and r.history[n - 1, 0, 0] < TOL
    _against(r, 1, refs[1], AR.BOUNDS[case.cls], "dsmin neighbour")
    single = _batched(_step_call(gpu_ctx, case, b=1))
    assert all(_same(r, k, 1, single, k, 0) for k in range(3))


@pytest.mark.parametrize("name", ["planar_L2", "halo_L2"])
def test_batch_equals_singles_and_repeats(gpu_ctx, name):
    case = AR.cases(MU)[name]._replace(K=6)
    rb = _call(gpu_ctx, case, 9)
    again = _call(gpu_ctx, case, 9)
    for f in FIELDS:
        assert np.array_equal(getattr(rb, f), getattr(again, f), equal_nan=True), f
    assert np.all(rb.status == 0)
    for b in (0, 7, 8):                                    # both wavefronts of the batch
        one = _batched(lto.halo_arclength(case.seeds[:, b], case.K, case.ds, case.dir0, planar=case.planar, dir_is_tangent=case.tangent,
                                          tol=TOL, ctx=gpu_ctx))
        assert all(_same(rb, k, b, one, k, 0) for k in range(case.K)), b


def _chained(gpu_ctx, r, b, planar, kw, first=None):
    """Every member k >= 1 of orbit b (and member 0 from `first` = (seed, dir0) where the march started from a tangent) against the
    one-member call from member k - 1's state and tangent by member k's ds_out with grow = 1; `halvings` is the march's own."""
    K = r.status.shape[0]
    for k in range(K):
        if k == 0 and first is None:
            continue
        seed, t = first if k == 0 else (r.state[:, k - 1, b], r.tangent[:, k - 1, b])
        ds = float(r.ds[k, b])
        one = _batched(lto.halo_arclength(seed, 1, ds, t, planar=planar, dir_is_tangent=True, tol=TOL, ctx=gpu_ctx,
                                          **dict(kw, grow=1.0, ds_min=ds, ds_max=ds)))
        assert _same(r, k, b, one, 0, 0, skip=("halvings",)), (k, b)
        assert one.halvings[0, 0] == 0


@pytest.mark.parametrize("name", ["halo_L2", "lyapunov3_L2"])
def test_every_member_equals_its_chained_call(gpu_ctx, name):
    case = AR.cases(MU)[name]
    r = _call(gpu_ctx, case, 2)
    assert np.all(r.status == 0)
    for b in range(2):
        _chained(gpu_ctx, r, b, case.planar, {}, first=(case.seeds[:, b], case.dir0) if case.tangent else None)


@pytest.mark.parametrize("name", ["halve", "grow"])
def test_halved_and_grown_members_equal_their_chained_calls(gpu_ctx, name):
    case = AR.step_cases(MU)[name]
    r = _batched(_step_call(gpu_ctx, case))
    assert np.all(r.status == 0)
    kw = {k: v for k, v in case.kw.items() if k in ("t_max", "cos_min")}
    _chained(gpu_ctx, r, 0, case.planar, kw, first=(case.seeds[:, 0], case.dir0[:, 0]) if case.tangent else None)


def test_statuses_beside_unchanged_good_orbits(gpu_ctx):
    halo = AR.cases(MU)["halo_L2"]
    good, t_good = halo.seeds[:, 0], halo.dir0
    kw = dict(dir_is_tangent=True, tol=TOL, ctx=gpu_ctx)
    want = lto.halo_arclength(np.array([good, good]).T, 3, 0.02, t_good, **kw)
    assert np.all(want.status == 0)

    def check(r, bad, statuses, good_cols, ref=want):
        for b, st in zip(bad, statuses):
            assert list(r.status[:, b]) == st, (b, list(r.status[:, b]))
            assert all(_none(r, k, b) for k in range(r.status.shape[0]) if st[k] >= 2)
        for b in good_cols:
            assert all(_same(r, k, b, ref, k, 0) for k in range(r.status.shape[0])), b

    nan_seed, still = good.copy(), good.copy()
    nan_seed[0] = np.nan
    still[4] = 0.0
    # a NaN seed, vy0 = 0
    r = lto.halo_arclength(np.array([good, nan_seed, still, good]).T, 3, 0.02, t_good, **kw)
    check(r, (1, 2), ([2, 2, 2], [2, 2, 2]), (0, 3))
    assert np.all(r.iterations[:, 1:3] == 0) and np.all(np.isnan(r.history[:, :, 1:3])) and np.all(np.isnan(r.ds[:, 1:3]))
    # a zero dir0, a NaN dir0
    dirs = np.array([t_good, np.zeros(3), [np.nan, 0.0, 1.0], t_good]).T
    r = lto.halo_arclength(np.array([good] * 4).T, 3, 0.02, dirs, **kw)
    check(r, (1, 2), ([2, 2, 2], [2, 2, 2]), (0, 3))

    # planar: z0 != 0 is refused next to a Lyapunov orbit; and a dir0 perpendicular to the seed's tangent when the seed is corrected
    lyap = AR.lyapunov_orbit(2, MU)
    up = np.array([0.0, 0.0, 1.0])
    pkw = dict(planar=True, tol=TOL, ctx=gpu_ctx)
    pwant = _batched(lto.halo_arclength(lyap, 3, 0.01, up, **pkw))
    assert np.all(pwant.status == 0)
    r = lto.halo_arclength(np.array([lyap, good, lyap]).T, 3, 0.01, up, **pkw)
    check(r, (1,), ([2, 2, 2],), (0, 2), ref=pwant)
    r = lto.halo_arclength(np.array([lyap, lyap, lyap]).T, 3, 0.01, np.array([up, [0.0, 1.0, 0.0], up]).T, **pkw)
    check(r, (1,), ([2, 2, 2],), (0, 2), ref=pwant)
    assert np.all(np.isnan(r.history[:, :, 1])) and np.all(r.iterations[:, 1] == 0)      # the flight was made; nothing of it is kept

    # max_iter = 0: the start is evaluated.  A seed on the family (status 0) beside one off it (status 1, its numbers kept, march over)
    south = np.array([0.0, -1.0, 0.0])
    on = lto.halo_arclength(good, 1, 0.02, south, tol=TOL, ctx=gpu_ctx).state[:, 0]       # the device's own point of the family
    off = HR.perturbed(good, 3)
    r0 = lto.halo_arclength(np.array([on, off]).T, 2, 0.02, south, max_iter=0, tol=TOL, ctx=gpu_ctx)
    assert list(r0.status[:, 0]) == [0, 1] and list(r0.status[:, 1]) == [1, 2] and r0.history.shape == (1, 2, 2)
    assert np.array_equal(r0.state[:, 0, 0], on) and np.array_equal(r0.state[:, 0, 1], off) and np.all(r0.iterations == 0)
    assert np.array_equal(r0.history[0], r0.resid, equal_nan=True) and r0.resid[0, 1] > 1e-6 and np.isfinite(r0.det[0, 1]) and _none(r0, 1, 1)
    assert r0.halvings[1, 0] == 10 and r0.ds[1, 0] == 0.02 / 1024.0 and r0.ds[0, 0] == 0.0 and r0.ds[0, 1] == 0.0
    assert abs(np.linalg.norm(r0.tangent[:, 0, 1]) - 1.0) <= 1e-15

    # t_max = 1.0 is before the half period (1.7): no crossing
    rt = lto.halo_arclength(np.array([good, good]).T, 2, 0.02, t_good, t_max=1.0, ds_min=0.02, **kw)
    assert np.all(rt.status == 2) and all(_none(rt, k, b) for k in range(2) for b in range(2))
    # max_steps = 5: the flight runs out of steps
    rs = lto.halo_arclength(np.array([good, good]).T, 2, 0.02, t_good, integ=lto.integrator(max_steps=5), ds_min=0.02, **kw)
    assert np.all(rs.status == 2) and np.all(np.isnan(rs.state)) and np.all(rs.iterations == 0)
    # sing_tol = 0.999: by Hadamard's inequality |det| <= the product of the row norms, and here the ratio is below 0.9 (vetted on
    # the host), so the first step is refused as singular
    r3 = lto.halo_arclength(np.array([good, good]).T, 2, 0.02, t_good, sing_tol=0.999, ds_min=0.02, **kw)
    assert list(r3.status[:, 0]) == [3, 2] and _none(r3, 0, 0) and list(r3.iterations[:, 0]) == [0, 0]
    assert np.isfinite(r3.history[0, 0, 0]) and np.all(np.isnan(r3.history[1:, 0, 0]))
    # cos_min = 0.9999: the first step up the halo branch turns the tangent by 26 degrees (status 4), a step of 1e-3 along the planar
    # family in the 3-unknown form by less than 0.1 degree
    f0 = AR.lyapunov_family(2, MU)[0]
    seeds, dirs = np.array([good, f0.state]).T, np.array([t_good, f0.tangent]).T
    r4 = lto.halo_arclength(seeds, 2, np.array([0.02, 1e-3]), dirs, cos_min=0.9999, ds_min=0.015, ds_max=0.02, **kw)
    assert list(r4.status[:, 0]) == [4, 2] and list(r4.status[:, 1]) == [0, 0] and _none(r4, 0, 0)
    assert list(r4.halvings[:, 0]) == [0, 0] and r4.ds[0, 0] == 0.02
    alone = _batched(lto.halo_arclength(f0.state, 2, 1e-3, f0.tangent, cos_min=0.9999, ds_min=0.015, ds_max=0.02, **kw))
    assert all(_same(r4, k, 1, alone, k, 0) for k in range(2))


def test_refusals_through_the_raw_entry_point(gpu_ctx):
    import ctypes as C
    halo = AR.cases(MU)["halo_L2"]
    fn, h = gpu_ctx.fn("halo_arclength_batch"), gpu_ctx.handle
    S = np.asfortranarray(halo.seeds[:, :1])
    D = np.asfortranarray(halo.dir0.reshape(3, 1))
    state, status = np.zeros(6), np.zeros(1, dtype=np.int32)
    ptr = lambda arr: arr.ctypes.data_as(C.c_void_p) if arr is not None else None        # noqa: E731

    def call(n_members=1, n_batch=1, mu=MU, ds0=0.02, ds_min=1e-3, ds_max=0.02, grow=1.0, fast_iter=3, cos_min=0.0, tol=1e-12, max_iter=15,
             t_max=10.0, sing_tol=1e-12, integ=None, seeds=S, dirs=D, out=state, st=status, no_ds=False):
        integ = integ or lto.integrator()
        s0 = np.array([ds0])
        return fn(h, n_members, n_batch, mu, 0, 1, ptr(seeds), ptr(dirs), None if no_ds else ptr(s0), ds_min, ds_max, grow, fast_iter, cos_min,
                  tol, max_iter, t_max, sing_tol, C.byref(integ), ptr(out), None, None, None, None, None, None, None, None, None, ptr(st))

    assert call() == 0 and status[0] == 0                  # every output but state_out and status may be NULL
    for kw in ({"n_members": 0}, {"n_batch": 0}, {"tol": 0.0}, {"max_iter": -1}, {"t_max": 0.0}, {"t_max": np.inf}, {"mu": 1.5},
               {"sing_tol": 1.0}, {"integ": lto.integrator(lto.RK4, steps=0)}, {"ds0": 0.0}, {"ds0": -0.01}, {"ds0": np.nan},
               {"ds0": np.inf}, {"ds_min": 0.0}, {"ds_min": 0.03}, {"ds_max": np.inf}, {"ds_min": np.nan}, {"grow": 0.99}, {"grow": np.nan},
               {"fast_iter": -1}, {"cos_min": 1.0}, {"cos_min": -0.01}, {"cos_min": np.nan},
               {"n_members": 1 << 20, "n_batch": 1 << 20}, {"n_members": 1 << 16, "n_batch": 1 << 13},
               {"n_members": 1 << 14, "n_batch": 1 << 13, "max_iter": 15}, {"n_batch": 1 << 28, "max_iter": 0}):
        assert call(**kw) == -1, kw
    for method in (lto.RKF78_FIXED, lto.RKF78_ADAPTIVE):
        assert call(integ=lto.integrator(method, steps=10)) == -3
    assert call(seeds=None) == -2 and call(dirs=None) == -2 and call(no_ds=True) == -2 and call(out=None) == -2 and call(st=None) == -2
    assert fn(None, 1, 1, MU, 0, 1, None, None, None, 1e-3, 0.02, 1.0, 3, 0.0, 1e-12, 15, 10.0, 1e-12, None, None, None, None, None, None,
              None, None, None, None, None, None) == -2
    assert call() == 0 and status[0] == 0                  # the context is fine afterwards
    assert gpu_ctx.lib.lto_last_call_ms(gpu_ctx.handle) > 0.0


def test_rk4_agrees_with_dop853(gpu_ctx):
    """8 members of the planar L2 family, 4 000 steps over t_max = 3.4 = two half periods: 2 000 steps per half period, the setting
    DESIGN 4.25 measured the corrector's RK4 form at (bound 1e-9: RK4's h^4 with the flow's growth over half a revolution)."""
    case = AR.cases(MU)["planar_L2"]
    a = _call(gpu_ctx, case, 1)
    r = _call(gpu_ctx, case, 1, t_max=3.4, integ=lto.integrator(lto.RK4, steps=4000))
    e = max(np.abs(a.state - r.state).max(), np.abs(a.period - r.period).max(), np.abs(a.tangent - r.tangent).max())
    print("arclength march RK4 x 2000 per half period against DOP853: %.2e" % e)
    assert np.all(a.status == 0) and np.all(r.status == 0) and e <= 1e-9 and np.array_equal(a.ds, r.ds)


@pytest.fixture(scope="module")
def branch(gpu_ctx):
    return drivers.halo_from_lyapunov(2, 24, 0.02, north=False, n_samples=20, tol=TOL, ctx=gpu_ctx)


def test_halo_from_lyapunov_against_the_reference_driver(branch):
    if "driver" not in _REF:
        _REF["driver"] = AR.halo_from_lyapunov(2, 24, 0.02, MU, north=False)
    bp, members = _REF["driver"]
    b_lyap, b_halo = AR.BOUNDS["lyapunov3"], AR.BOUNDS["halo_L2"]
    got = branch.branch_point
    print("branch point: C %.12f P %.12f (reference off by %.2e, %.2e), |det| %.2e after %d trials" % (
        got.jacobi, got.period, abs(got.jacobi - bp.jacobi), abs(got.period - bp.period), abs(got.det), len(got.trials)))
    assert got.status == 0 and len(got.trials) <= 8 and abs(got.det) < 1e-9 * abs(branch.lyapunov.det[12])
    assert abs(got.jacobi - bp.jacobi) <= b_lyap[2] and abs(got.period - bp.period) <= b_lyap[2]
    assert abs(got.jacobi - 3.152118903) < 1e-8 and abs(got.period - 3.415530893) < 1e-8
    assert drivers.family_bifurcations(branch.lyapunov) == [13]
    fam = branch.family
    assert fam.states.shape == (6, 25) and np.all(fam.status == 0) and len(members) == 25
    e = [max(np.abs(fam.states[:, k] - m.state).max(), np.abs(fam.tangent[:, k] - m.tangent).max()) for k, m in enumerate(members)]
    eP = [abs(fam.period[k] - m.period) for k, m in enumerate(members)]
    print("members: state / tangent %.2e, period %.2e" % (max(e), max(eP)))
    assert max(e) <= b_halo[1] and max(np.abs(fam.states[:, k] - m.state).max() for k, m in enumerate(members)) <= b_halo[0]
    assert max(eP) <= b_halo[2]
    assert drivers.family_folds(fam)["z0"] == AR.family_folds(members, 1) == [13]
    tb = branch.table
    print("closures of the 25 tables: at most %.2e" % tb.closure.max())
    assert tb.X.shape == (6, 20, 25) and np.all(tb.status == 0) and np.all(np.isfinite(tb.closure))


def test_the_branch_passes_through_the_packaged_orbits(gpu_ctx, branch):
    fam = branch.family
    for tb in synth.halo_orbits():
        packaged = HR.seed_of(np.asarray(tb[:6], dtype=float))
        k = int(np.argmin(np.abs(fam.states[0] - packaged[0])))
        start = fam.states[:, k].copy()
        start[0] = packaged[0]
        got = lto.halo_correct(start, "x0", tol=TOL, ctx=gpu_ctx)
        own = lto.halo_correct(packaged, "x0", tol=TOL, ctx=gpu_ctx)
        d = np.abs(got.state - own.state).max()
        print("member %d re-corrected at the packaged x0: %.2e from halo_correct(packaged seed), %.2e from the packaged seed" % (
            k, d, np.abs(got.state - packaged).max()))
        # DESIGN 4.25's bound of the 3-D corrector against its reference, for two device results that are each within it
        assert got.status == 0 and own.status == 0 and d <= 1e-11 and abs(got.period - own.period) <= 1e-11
        assert np.abs(got.state - packaged).max() < 1e-7
