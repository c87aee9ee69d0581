"""GPU checks of the direct method's mesh refinement on the device (lto_direct_refine_batch).

The reference is the host loop drivers.meshRefine_direct on this library's own sweeps (HipDirectOps): batched=False, the literal
one-node-per-pass loop, at every size, wherever the node limit does not cut a pass short.  Where it does (the `all_once` and `clipped`
shapes and the capped trajectory of the batch) the rule of the call -- the first segments in index order are split -- is the host
loop's batched=True, while batched=False would split the largest first; those cases alone compare with batched=True, which the driver
documents (and tests/test_drivers.py checks) to give the literal loop's mesh whenever the limit is not reached.

Comparisons are bitwise for n, t, U and the kept columns of X, and 1e-14 relative for inserted states.  Every fixture is first
shown to be decisive on the host loop alone (RecordingOps): no estimate within 1e-6 relative of a tolerance it is compared with,
and at every removal step the two smallest estimates differ by more than 1e-6 relative or are bitwise equal."""
import numpy as np
import pytest

import lowthrustopt_amd as lto
from lowthrustopt_amd import drivers, synth
from lowthrustopt_amd.constants import MU, DU, TU

pytestmark = pytest.mark.gpu
ISP = 2000.0


class RecordingOps:
    """HipDirectOps that keeps every estimate vector the host loop decided on."""

    def __init__(self, ctx):
        self.ops = drivers.HipDirectOps(MU, DU, TU, ISP, ctx=ctx)
        self.seen = []

    def defect(self, X, U, t, nsteps):
        d, e = self.ops.defect(X, U, t, nsteps)
        self.seen.append(np.array(e))
        return d, e

    def midpoints(self, X, U, t):
        return self.ops.midpoints(X, U, t)


def assert_decisive(seen, tol_min, tol_max):
    for e in seen:
        for tol in (tol_min, tol_max):
            if np.isfinite(tol) and tol > 0.0:
                assert np.all(np.abs(e - tol) > 1e-6 * tol), "fixture: an estimate sits on a tolerance"
        if len(e) > 1 and e.min() < tol_min:
            a, b = np.sort(e)[:2]
            assert a == b or (b - a) > 1e-6 * b, "fixture: the two smallest estimates are too close to call"


def host_loop(ctx, X, U, t, nsteps, tol_min, tol_max, max_nodes, batched=False):
    ops = RecordingOps(ctx)
    r = drivers.meshRefine_direct(X, U, t, X.shape[0], X.shape[1], nsteps, ISP, MU, DU, TU, tol_min=tol_min, tol_max=tol_max,
                                  max_nodes=max_nodes, batched=batched, ops=ops, verbose=False)
    assert_decisive(ops.seen, tol_min, tol_max)
    return r


def device(ctx, X, U, t, nsteps, tol_min, tol_max, max_nodes):
    return lto.direct_refine(X, U, t, nsteps, MU, DU, TU, ISP, tol_min, tol_max, max_nodes, ctx=ctx)


def assert_same_mesh(r, ref, X_in, t_in):
    Xh, Uh, th, nh = ref
    assert r.n == nh and r.X.shape == Xh.shape and r.t.shape == (nh,)
    assert np.array_equal(r.t, th)
    assert np.array_equal(r.U, Uh)
    kept = np.isin(r.t, t_in)                       # times are unique: a kept node carries an input time
    assert np.array_equal(r.X[:, kept], Xh[:, kept])
    assert np.array_equal(r.X[:, kept], X_in[:, np.isin(t_in, r.t)])      # bit copies of the input
    new = ~kept
    if new.any():
        assert np.all(np.abs(r.X[:, new] - Xh[:, new]) <= 1e-14 * np.abs(Xh[:, new]))


def assert_after_the_call(ctx, r, nsteps, tol_min, tol_max):
    """An independent sweep of the output reproduces errors_out bitwise, and the status' inequalities hold."""
    _, e = lto.direct_defectCalc(r.X, r.U, r.t, nsteps, MU, DU, TU, ISP, ctx=ctx)
    assert np.array_equal(e, r.errors)
    assert r.status in (0, 1)
    if r.passes == 0:                               # (halves inserted later may well lie below tol_min: the removal is over by then)
        assert e.min() >= tol_min or r.n == 2
    if r.status == 0:
        assert e.max() <= tol_max
    else:
        assert e.max() > tol_max


def mesh_problem(nstate):
    X, U, T = synth.direct_problem(12, seed=3, nstate=nstate, dt_seg=0.4)
    return X[:, :, 0], U[:, :, 0], T[:, 0]


@pytest.mark.parametrize("nstate", [6, 7])
def test_equals_the_host_loop(gpu_ctx, nstate):
    X, U, t = mesh_problem(nstate)
    tol_min, tol_max = 1e-16, 1e-13
    ref = host_loop(gpu_ctx, X, U, t, 10, tol_min, tol_max, 1 << 10)
    r = device(gpu_ctx, X, U, t, 10, tol_min, tol_max, 1 << 10)
    print("nstate %d: %d -> %d nodes, removed %d, %d passes, status %d" % (nstate, 12, r.n, r.n_removed, r.passes, r.status))
    assert r.n_removed > 0 and r.passes > 0          # both phases fire (tests/test_drivers.py:183-186)
    assert_same_mesh(r, ref, X, t)
    assert r.status == 0
    assert_after_the_call(gpu_ctx, r, 10, tol_min, tol_max)


# ------------------------------------------------------------------------------------------------ the tie rule
STATE_A = np.array([0.85, 0.02, 0.05, 0.01, 0.18, -0.02])
STATE_B = np.array([0.87, -0.03, 0.04, -0.02, 0.16, 0.03])
STATE_C = np.array([1.0 - MU + 0.06, 0.0, 0.0, 0.0, 0.3, 0.0])      # close to the smaller primary: a much larger estimate


def pattern(states, dt=0.125):
    X = np.asfortranarray(np.stack(states, axis=1))
    U = np.asfortranarray(np.repeat(np.array([[0.01], [-0.02], [0.015]]), X.shape[1], axis=1))
    return X, U, dt * np.arange(X.shape[1])


def test_first_of_equal_minima_goes(gpu_ctx):
    A, B = STATE_A, STATE_B
    _, e = lto.direct_defectCalc(*pattern([A, B, A, B, A]), 10, MU, DU, TU, ISP, ctx=gpu_ctx)
    if e[0] > e[1]:
        A, B = B, A                                   # the pair whose (A, B) segments are the smaller ones
    X, U, t = pattern([A, B, A, B, A])
    _, e = lto.direct_defectCalc(X, U, t, 10, MU, DU, TU, ISP, ctx=gpu_ctx)
    print("estimates", e)
    assert e[0] == e[2] and e[1] == e[3]              # autonomous dynamics: equal segments, bitwise equal estimates
    assert e[1] - e[0] > 1e-3 * e[1]
    tol_min = 0.5 * (e[0] + e[1])
    # arg-min 0 (first of the two equal minima) -> k == 0 becomes 1: node 1 goes, whatever follows
    ref = host_loop(gpu_ctx, X, U, t, 10, tol_min, np.inf, 5)
    r = device(gpu_ctx, X, U, t, 10, tol_min, np.inf, 5)
    assert_same_mesh(r, ref, X, t)
    assert r.n_removed >= 1 and t[1] not in r.t and r.t[0] == t[0] and r.t[-1] == t[-1]
    assert_after_the_call(gpu_ctx, r, 10, tol_min, np.inf)
    # equal minima away from the first segment: C, A, B, A, B, A -> segments 1 and 3 tie, node 1 goes first (not node 3)
    X, U, t = pattern([STATE_C, A, B, A, B, A])
    _, e = lto.direct_defectCalc(X, U, t, 10, MU, DU, TU, ISP, ctx=gpu_ctx)
    assert e[1] == e[3] and e[1] < e[0] and e[1] < e[2] and e[2] == e[4]
    tol_min = 0.5 * (e[1] + min(e[0], e[2]))
    ref = host_loop(gpu_ctx, X, U, t, 10, tol_min, np.inf, 6)
    r = device(gpu_ctx, X, U, t, 10, tol_min, np.inf, 6)
    assert_same_mesh(r, ref, X, t)
    assert r.n_removed >= 1 and t[1] not in r.t
    # every estimate below tol_min: the removal stops at two nodes, the first and the last
    r = device(gpu_ctx, X, U, t, 10, np.inf, np.inf, 6)
    assert r.n == 2 and r.n_removed == 4 and r.status == 0 and r.passes == 0
    assert np.array_equal(r.t, t[[0, -1]]) and np.array_equal(r.X, X[:, [0, -1]]) and np.array_equal(r.U, U[:, [0, -1]])
    ref = host_loop(gpu_ctx, X, U, t, 10, np.inf, np.inf, 6)
    assert_same_mesh(r, ref, X, t)


# ------------------------------------------------------------------------------------------------ shapes
def decisive_between(es, k):
    """A value between the sorted estimates es[k-1] and es[k'] for the first k' >= k with a clear gap below it."""
    for j in range(k, len(es)):
        if es[j] - es[j - 1] > 1e-3 * es[j]:
            return 0.5 * (es[j - 1] + es[j])
    raise AssertionError("fixture: no clear gap between the sorted estimates")


_shape_cache = {}


def shape_problem(ctx, m):
    """n = m + 1 nodes on a grid whose segments alternate between 0.4 and 0.05 TU, and its estimates at nsteps = 2 (computed once)."""
    if m not in _shape_cache:
        n = m + 1
        X, U, _ = synth.direct_problem(n, seed=11, dt_seg=0.4)
        t = np.concatenate(([0.0], np.cumsum(np.where(np.arange(m) % 2 == 0, 0.4, 0.05))))
        X, U = X[:, :, 0], U[:, :, 0]
        _, e = lto.direct_defectCalc(X, U, t, 2, MU, DU, TU, ISP, ctx=ctx)
        for a in (X, U, t, e):
            a.setflags(write=False)
        _shape_cache[m] = (X, U, t, e)
    return _shape_cache[m]


SHAPES = [(m, what) for m in (1, 2, 3, 63, 64, 65, 255, 256, 257, 1025)
          for what in ("nothing", "all_once", "clipped", "alternating", "remove")
          if m >= 2 or what not in ("alternating", "remove")]     # one segment: no pattern to alternate, no node to remove


@pytest.mark.parametrize("m,what", SHAPES)
def test_shapes(gpu_ctx, m, what):
    """Sizes around the 64-entry scan tile, the 256-thread workgroup and the 1 024-node limit of the removal's LDS form (1 026 nodes
    take the global-scratch form); decision patterns chosen from the sorted estimates of the input."""
    X, U, t, e = shape_problem(gpu_ctx, m)
    n = m + 1
    es = np.sort(e)
    tol_min, batched = 0.0, False
    if what == "nothing":
        tol_max, M = 2.0 * es[-1], n + 7
    elif what == "all_once":                          # every segment split once, then the limit
        tol_max, M, batched = 0.5 * es[0], 2 * n - 1, True
    elif what == "clipped":                           # the limit falls in the middle of the first pass
        tol_max, M, batched = 0.5 * es[0], n + (m + 1) // 2, True
    elif what == "alternating":                       # the long segments (even ones) are split, the short ones are not
        lo, hi = e[1::2].max(), e[0::2].min()
        assert hi - lo > 1e-3 * hi, "fixture: long and short segments do not separate"
        tol_max, M = 0.5 * (lo + hi), 4 * n
    else:                                             # a handful of removals, each followed by the merged segment's estimate
        tol_min, tol_max, M = decisive_between(es, min(4, m - 1)), np.inf, n
    ref = host_loop(gpu_ctx, X, U, t, 2, tol_min, tol_max, M, batched=batched)
    r = device(gpu_ctx, X, U, t, 2, tol_min, tol_max, M)
    print("m = %d %s: n %d -> %d, removed %d, passes %d, status %d" % (m, what, n, r.n, r.n_removed, r.passes, r.status))
    assert_same_mesh(r, ref, X, t)
    assert_after_the_call(gpu_ctx, r, 2, tol_min, tol_max)
    if what == "nothing":
        assert r.n == n and r.passes == 0 and r.n_removed == 0 and r.status == 0
    elif what == "all_once":
        assert r.n == 2 * n - 1 and r.passes == 1 and np.array_equal(r.t[0::2], t)
    elif what == "clipped":
        k = (m + 1) // 2
        assert r.n == M and r.passes == 1 and (r.status == 1 or k == m)     # segments k .. m-1 stay above tol_max
        assert np.array_equal(r.t[0:2 * k:2], t[:k]) and np.array_equal(r.t[2 * k:], t[k:])   # the first k segments, no others
    elif what == "alternating":
        assert r.passes >= 1 and r.status == 0 and np.all(np.isin(t, r.t))
        assert all(np.count_nonzero((r.t > t[i]) & (r.t < t[i + 1])) == 0 for i in range(1, m, 2))
    else:
        assert r.n_removed >= 1 and r.passes == 0


# ------------------------------------------------------------------------------------------------ batch
STATE_P = synth.direct_problem(12, seed=3, dt_seg=0.4)[0][:, 0, 0].copy()       # on the departure halo: a middling estimate
STATE_Q = np.array([0.5 - MU, np.sqrt(3.0) / 2.0, 0.0, 0.0, 0.0, 0.0])          # L4, at rest: next to none
STATE_L = STATE_C                                                               # a large one


def batch_problem():
    """Five 12-node trajectories on one grid with five outcomes under tol_min = 3e-18, tol_max = 1e-11, max_nodes = 18."""
    P, Q, L = STATE_P, STATE_Q, STATE_L
    rows = [[P] * 12,                                                 # nothing to do
            [P] * 3 + [Q, Q] + [P] * 7,                               # the (Q, Q) segment's left node is removed
            [P] * 6 + [L] + [P] * 5,                                  # the two segments at L are split
            [P] * 2 + [Q, Q] + [P] * 4 + [L] + [P] * 3,               # both
            [P, L, P, P, L, P, P, L, P, P, L, P]]                     # eight segments to split, room for six
    X = np.asfortranarray(np.stack([np.stack(r, axis=1) for r in rows], axis=2))
    U = np.zeros((3, 12, 5), order="F")
    U[:] = np.array([0.01, -0.02, 0.015])[:, None, None]
    return X, U, 0.4 * np.arange(12)


def same_result(a, b):
    return (a.n, a.n_removed, a.passes, a.status) == (b.n, b.n_removed, b.passes, b.status) and \
        all(x.tobytes() == y.tobytes() for x, y in ((a.X, b.X), (a.U, b.U), (a.t, b.t), (a.errors, b.errors)))


def test_batch_of_different_outcomes(gpu_ctx):
    X, U, t = batch_problem()
    tol_min, tol_max, M = 3e-18, 1e-11, 18
    singles = [device(gpu_ctx, X[:, :, b], U[:, :, b], t, 10, tol_min, tol_max, M) for b in range(5)]
    for b, s in enumerate(singles):
        print("trajectory %d: n %d, removed %d, passes %d, status %d" % (b, s.n, s.n_removed, s.passes, s.status))
        ref = host_loop(gpu_ctx, X[:, :, b], U[:, :, b], t, 10, tol_min, tol_max, M, batched=(b == 4))
        assert_same_mesh(s, ref, X[:, :, b], t)
        assert_after_the_call(gpu_ctx, s, 10, tol_min, tol_max)
    outcome = [(s.n_removed > 0, s.passes > 0, s.status) for s in singles]
    assert outcome == [(False, False, 0), (True, False, 0), (False, True, 0), (True, True, 0), (False, True, 1)]
    assert singles[4].n == M
    for grids in (t, np.asfortranarray(np.repeat(t[:, None], 5, axis=1))):
        got = device(gpu_ctx, X, U, grids, 10, tol_min, tol_max, M)
        assert all(same_result(g, s) for g, s in zip(got, singles))
    # the raw outputs: NaN from n_out[b] on
    import ctypes as C
    from lowthrustopt_amd.hotpath import _ptr
    Xo = np.zeros((6, M, 5), order="F"); Uo = np.zeros((3, M, 5), order="F"); to = np.zeros((M, 5), order="F")
    eo = np.zeros((M - 1, 5), order="F"); n_out = np.zeros(5, dtype=np.int32)
    prm = lto.LtoDirectParams(MU, DU, TU, ISP)
    gpu_ctx.check(gpu_ctx.lib.lto_direct_refine_batch(gpu_ctx.handle, 6, 12, 5, _ptr(X), _ptr(U), _ptr(t), 1, 10, C.byref(prm), tol_min,
                                                      tol_max, M, _ptr(Xo), _ptr(Uo), _ptr(to), _ptr(n_out), None, None, None, _ptr(eo)))
    for b, s in enumerate(singles):
        k = int(n_out[b])
        assert k == s.n and Xo[:, :k, b].tobytes(order="F") == s.X.tobytes(order="F")
        assert np.isnan(Xo[:, k:, b]).all() and np.isnan(Uo[:, k:, b]).all() and np.isnan(to[k:, b]).all() and np.isnan(eo[k - 1:, b]).all()
        assert not np.isnan(to[:k, b]).any() and not np.isnan(eo[:k - 1, b]).any()


def test_nan_trajectory_is_left_alone(gpu_ctx):
    Xb, Ub, Tb = synth.direct_problem(12, n_batch=3, seed=5, dt_seg=0.4)
    t = Tb[:, 0].copy()
    Xb[1, 5, 1] = np.nan
    tol_min, tol_max = 1e-16, 1e-13
    got = device(gpu_ctx, Xb, Ub, t, 10, tol_min, tol_max, 64)
    bad = got[1]
    assert bad.status == 2 and bad.n == 12 and bad.n_removed == 0 and bad.passes == 0
    assert bad.X.tobytes(order="F") == np.asfortranarray(Xb[:, :, 1]).tobytes(order="F")
    assert np.array_equal(bad.U, Ub[:, :, 1]) and np.array_equal(bad.t, t)
    for b in (0, 2):
        alone = device(gpu_ctx, Xb[:, :, b], Ub[:, :, b], t, 10, tol_min, tol_max, 64)
        assert same_result(got[b], alone)
        assert alone.status in (0, 1) and (alone.n_removed > 0 or alone.passes > 0)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(gpu_ctx):
    import ctypes as C
    from lowthrustopt_amd.hotpath import _ptr
    X, U, t = mesh_problem(6)
    M = 16
    Xo = np.zeros((6, M), order="F"); Uo = np.zeros((3, M), order="F"); to = np.zeros(M); n_out = np.zeros(1, dtype=np.int32)
    prm = lto.LtoDirectParams(MU, DU, TU, ISP)
    fn = gpu_ctx.lib.lto_direct_refine_batch
    EINVAL, ENULL = lto._lib.LTO_EINVAL, lto._lib.LTO_ENULL

    def call(nstate=6, n=12, B=1, X=X, U=U, t=t, ntg=1, nsteps=10, prm=C.byref(prm), tmin=1e-16, tmax=1e-13, M=M, Xo=Xo, to=to,
             n_out=n_out):
        return fn(gpu_ctx.handle, nstate, n, B, _ptr(X), _ptr(U), _ptr(t), ntg, nsteps, prm, tmin, tmax, M, _ptr(Xo), _ptr(Uo), _ptr(to),
                  _ptr(n_out), None, None, None, None)

    assert call() == 0                                # the optional outputs may all be NULL
    for bad in (dict(nstate=5), dict(nstate=8), dict(n=1), dict(B=0), dict(nsteps=1), dict(M=11), dict(ntg=2), dict(ntg=0),
                dict(tmin=np.nan), dict(tmax=np.nan)):
        assert call(**bad) == EINVAL, bad
    for bad in (dict(X=None), dict(U=None), dict(t=None), dict(prm=None), dict(Xo=None), dict(to=None), dict(n_out=None)):
        assert call(**bad) == ENULL, bad
    assert gpu_ctx.lib.lto_direct_refine(None, 6, 12, _ptr(X), _ptr(U), _ptr(t), 10, C.byref(prm), 1e-16, 1e-13, M, _ptr(Xo), None,
                                         _ptr(to), _ptr(n_out), None, None, None, None) == ENULL


# ------------------------------------------------------------------------------------------------ driver and demo
def test_driver_device_path(gpu_ctx):
    X, U, t = mesh_problem(6)
    kw = dict(tol_min=1e-16, tol_max=1e-13, max_nodes=256, verbose=False)
    host = drivers.meshRefine_direct(X, U, t, 6, 12, 10, ISP, MU, DU, TU, batched=False, **kw)
    dev = drivers.meshRefine_direct(X, U, t, 6, 12, 10, ISP, MU, DU, TU, device=True, **kw)
    assert isinstance(dev, tuple) and len(dev) == 4 and isinstance(dev[3], int) and dev[3] == host[3]
    Xd, Ud, td, nd = dev
    assert Xd.shape == (6, nd) and Ud.shape == (3, nd) and td.shape == (nd,) and Xd.flags.f_contiguous and Ud.flags.f_contiguous
    assert np.array_equal(td, host[2]) and np.array_equal(Ud, host[1])
    assert np.all(np.abs(Xd - host[0]) <= 1e-14 * np.abs(host[0]))
    # an injected back end keeps the host loop, whatever `device` says
    ops = RecordingOps(gpu_ctx)
    drivers.meshRefine_direct(X, U, t, 6, 12, 10, ISP, MU, DU, TU, device=True, ops=ops, **kw)
    assert len(ops.seen) > 1


def test_demo_refine_resolves(gpu_ctx, capsys):
    import importlib.util
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "halo_direct_demo.py")
    spec = importlib.util.spec_from_file_location("halo_direct_demo", path)
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    out = demo.refine_and_resolve(ctx=gpu_ctx, verbose=False)
    print(out)
    assert out["n_before"] == 30
    assert out["status"] == 0 and out["max_defect"] <= 1e-6
