"""GPU checks of the direct method's resampling onto one node count (lto_direct_resample_batch), step by step against
the host restatement (tests/resample_reference.py):

  estimates   errors_before / errors_after == lto_direct_defect on the compacted input / on the output, bit for bit;
  grid        t_out against new_grid on the weights made from errors_before (16 ulp of t_end, as tests/test_remesh_gpu.py holds
              k_remesh_grid), end points bit copies;
  nodes       X_out against the CPU oracle's flow at the device's own new times, 1e-14 relative element by element (the bar of
              tests/test_direct_refine_gpu.py for inserted states) wherever an element is at least NEAR_ZERO = 1/4 of the largest
              magnitude S of its component along the trajectory; controls 1e-15 relative.  The halo's y, z and velocity
              components cross zero, and a step of the flow ends in x + h sum(b_i k_i), rounded at the size the component has
              on that arc, up to S: two correct flows of nsteps - 1 <= 9 steps may differ by about an ulp of S a step, 10 ulp of
              S in all, whatever |x| is.  1e-14 is 45 ulp of the element, so the element-wise bar is well-posed down to
              |x| = S / 4 (11 ulp of S).  Below that a separate check holds the difference to the same absolute room,
              1e-14 S / 4.  The element-wise figure over ALL elements is printed beside them; it is not asserted
              (DESIGN 4.17 records it);
  passes      passes = 2 == two calls of passes = 1, bit for bit, so the above covers every pass.
Then the bitwise cases, the statuses, the refusals, and the demo's three starts through drivers.multiStart_direct."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import direct_helpers as DH  # noqa: E402
import resample_reference as RS  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers, synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402
from lowthrustopt_amd.hotpath import _ptr  # noqa: E402

pytestmark = pytest.mark.gpu
ISP = 2000.0
PRM = (MU, DU, TU, ISP)
ULP16 = 16 * np.finfo(np.float64).eps
NEAR_ZERO = 0.25         # fraction of a component's largest magnitude below which an element counts as near a zero crossing


def resample(ctx, X, U, t, n_new, **kw):
    kw.setdefault("nsteps", 10)
    return lto.direct_resample(X, U, t, MU=MU, DU=DU, TU=TU, Isp=ISP, n_new=n_new, ctx=ctx, **kw)


def same(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


_problems = {}


def problem(nstate, n_cap, B, ragged):
    """B trajectories of n_cap columns on grids whose segments alternate between 0.4 and 0.1 TU (computed once); ragged: every
    odd trajectory keeps two nodes, and everything behind a trajectory's nodes is NaN."""
    key = (nstate, n_cap, B, ragged)
    if key not in _problems:
        X, U, _ = synth.direct_problem(n_cap, n_batch=max(B, 2), seed=21, nstate=nstate, dt_seg=0.4)
        X, U = np.asfortranarray(X[:, :, :B]), np.asfortranarray(U[:, :, :B])
        t1 = np.concatenate(([0.0], np.cumsum(np.where(np.arange(n_cap - 1) % 2 == 0, 0.4, 0.1))))
        t = np.asfortranarray(np.repeat(t1[:, None], B, axis=1) * (1.0 + 0.01 * np.arange(B))[None, :])
        n_in = None
        if ragged:
            n_in = np.where(np.arange(B) % 2 == 1, 2, n_cap).astype(np.int32)
            for b in range(B):
                X[:, n_in[b]:, b], U[:, n_in[b]:, b], t[n_in[b]:, b] = np.nan, np.nan, np.nan
        for a in (X, U, t):
            a.setflags(write=False)
        _problems[key] = (X, U, t, n_in)
    return _problems[key]


def check_against_the_restatement(ctx, oracle, X, U, t, n, r_X, r_U, r_t, e_before, e_after, n_new, nsteps, w_floor, tag):
    """One trajectory of a passes = 1 call: its valid input (X, U, t)[:n] and everything the call returned for it."""
    Xv, Uv, tv = np.asfortranarray(X[:, :n]), np.asfortranarray(U[:, :n]), np.ascontiguousarray(t[:n])
    _, e = lto.direct_defectCalc(Xv, Uv, tv, nsteps, *PRM[:3], ISP, ctx=ctx)
    assert e_before[:n - 1].tobytes() == e.tobytes() and np.isnan(e_before[n - 1:]).all()
    want_t = RS.grid(tv, RS.weights_from_estimates(e, w_floor), n_new)
    err_t = np.abs(r_t - want_t).max()
    assert r_t[0] == tv[0] and r_t[-1] == tv[-1] and np.all(np.diff(r_t) > 0)
    Xw, Uw = RS.nodes(oracle, Xv, Uv, tv, r_t, nsteps, PRM)
    d, mag = np.abs(r_X - Xw), np.abs(Xw)
    S = np.broadcast_to(mag.max(axis=1, keepdims=True), mag.shape)       # per component over the trajectory, see the module's docstring
    sized = mag >= NEAR_ZERO * S
    err_u = (np.abs(r_U - Uw) / np.maximum(np.abs(Uw), 1e-300)).max()
    with np.errstate(divide="ignore", invalid="ignore"):
        every = np.where(d > 0, d / mag, 0.0)
    k = np.unravel_index(np.argmax(every), every.shape)
    print("%s n %d -> %d: grid %.2e (%.1f ulp of t_end); states, element by element: %.2e where |x| >= S/4 (%d of %d elements), "
          "%.2e over all of them (there |x| = %.2e S); largest |difference| %.2f ulp of S, %.2f ulp of S where |x| < S/4; "
          "controls %.2e relative" % (tag, n, n_new, err_t, err_t / (np.finfo(float).eps * abs(tv[-1])), every[sized].max(),
                                      sized.sum(), sized.size, every.max(), mag[k] / S[k], (d / S).max() / np.finfo(float).eps,
                                      (d[~sized] / S[~sized]).max() / np.finfo(float).eps if (~sized).any() else 0.0, err_u))
    assert err_t <= ULP16 * abs(tv[-1])
    assert np.all(d[sized] <= 1e-14 * mag[sized])                        # the issue's bar, element by element
    assert np.all(d[~sized] <= 1e-14 * NEAR_ZERO * S[~sized])            # near a zero crossing: the same absolute room
    assert np.all(np.abs(r_U - Uw) <= 1e-15 * np.abs(Uw))
    _, e2 = lto.direct_defectCalc(np.asfortranarray(r_X), np.asfortranarray(r_U), r_t, nsteps, *PRM[:3], ISP, ctx=ctx)
    assert e_after.tobytes() == e2.tobytes()


# nstate, n_cap, n_new, n_batch, ragged, nsteps: every value the kernels branch on, both sides of the 64-lane block of the node
# kernel (64, 65, 129) and of the 32-segment block of the estimates (n_cap 30, 65), one- and two-node inputs and outputs
SHAPES = [(6, 2, 2, 1, False, 10), (6, 2, 17, 3, False, 2), (7, 3, 3, 1, False, 10), (6, 3, 4, 3, True, 10),
          (7, 5, 64, 3, True, 2), (6, 5, 65, 1, False, 10), (6, 30, 17, 70, True, 10), (7, 30, 129, 3, True, 10),
          (6, 65, 64, 3, True, 10), (7, 65, 65, 70, False, 2), (6, 65, 2, 3, True, 10), (7, 30, 30, 1, False, 10)]


@pytest.mark.parametrize("nstate,n_cap,n_new,B,ragged,nsteps", SHAPES)
def test_shapes(gpu_ctx, oracle, nstate, n_cap, n_new, B, ragged, nsteps):
    X, U, t, n_in = problem(nstate, n_cap, B, ragged)        # n_in None: the NULL argument
    w_floor = 0.1
    r = resample(gpu_ctx, X, U, t, n_new, n_in=n_in, nsteps=nsteps, w_floor=w_floor)
    assert r.X.shape == (nstate, n_new, B) and r.U.shape == (3, n_new, B) and r.t.shape == (n_new, B)
    assert np.all(r.status == 0) and np.isfinite(r.X).all() and np.isfinite(r.U).all()
    again = resample(gpu_ctx, X, U, t, n_new, n_in=n_in, nsteps=nsteps, w_floor=w_floor)
    assert same(r, again)                                     # two calls agree bit for bit
    for b in sorted({0, 1 % B, B - 1}):
        n = n_cap if n_in is None else int(n_in[b])
        check_against_the_restatement(gpu_ctx, oracle, X[:, :, b], U[:, :, b], t[:, b], n, r.X[:, :, b], r.U[:, :, b], r.t[:, b],
                                      r.errors_before[:, b], r.errors_after[:, b], n_new, nsteps, w_floor,
                                      "nstate %d B %d b %d nsteps %d" % (nstate, B, b, nsteps))
        one = resample(gpu_ctx, X[:, :n, b], U[:, :n, b], t[:n, b], n_new, nsteps=nsteps, w_floor=w_floor)   # the one-trajectory entry
        assert same((one.X, one.U, one.t, one.errors_after), (r.X[:, :, b], r.U[:, :, b], r.t[:, b], r.errors_after[:, b]))
        assert one.errors_before.tobytes() == r.errors_before[:n - 1, b].tobytes() and one.status == 0
    # two passes == the first pass' output resampled once more
    two = resample(gpu_ctx, X, U, t, n_new, n_in=n_in, nsteps=nsteps, w_floor=w_floor, passes=2)
    chained = resample(gpu_ctx, r.X, r.U, r.t, n_new, nsteps=nsteps, w_floor=w_floor)
    assert same((two.X, two.U, two.t, two.errors_after, two.status), (chained.X, chained.U, chained.t, chained.errors_after, chained.status))
    assert two.errors_before.tobytes() == r.errors_before.tobytes()
    assert chained.errors_before.tobytes() == r.errors_after.tobytes()


@pytest.mark.parametrize("nstate", [6, 7])
def test_uniform_weights_copy_the_mesh(gpu_ctx, nstate):
    """Uniform caller weights with n_new = n_in on any grid: bit copies of X, U and t."""
    X, U, t, n_in = problem(nstate, 30, 3, True)
    w = np.ones((29, 3), order="F")
    r = resample(gpu_ctx, X, U, t, 30, n_in=n_in, weights=w)
    assert np.all(r.status == 0)
    for b in range(3):
        n = int(n_in[b])
        one = resample(gpu_ctx, X[:, :n, b], U[:, :n, b], t[:n, b], n, weights=np.ones(n - 1))
        assert one.status == 0 and same((one.X, one.U, one.t), (X[:, :n, b], U[:, :n, b], t[:n, b]))
        if n == 30:
            assert same((r.X[:, :, b], r.U[:, :, b], r.t[:, b]), (X[:, :, b], U[:, :, b], t[:, b]))


@pytest.mark.parametrize("nstate,nsteps", [(6, 10), (7, 10), (6, 2)])
def test_odd_nodes_are_the_sweeps_midpoints(gpu_ctx, nstate, nsteps):
    """Uniform weights on a uniform grid with n_new = 2 n - 1: odd nodes == lto_direct_midpoints at the same nsteps, bit for bit;
    even nodes are bit copies."""
    n = 12
    X, U, T = synth.direct_problem(n, n_batch=2, seed=9, nstate=nstate, dt_seg=0.4)
    t = np.asfortranarray(T * np.array([1.0, 0.37])[None, :])  # 0.4 k and 0.148 k: no dyadic grid
    xm, _, _ = lto.direct_midpoints(X, U, t, nsteps, *PRM[:3], ISP, ctx=gpu_ctx)
    r = resample(gpu_ctx, X, U, t, 2 * n - 1, weights=np.ones((n - 1, 2), order="F"), nsteps=nsteps)
    assert np.all(r.status == 0)
    assert same((r.X[:, 0::2], r.U[:, 0::2], r.t[0::2]), (X, U, t))
    assert r.X[:, 1::2].tobytes() == np.asfortranarray(xm).tobytes()
    assert np.array_equal(r.t[1::2], t[:-1] + (t[1:] - t[:-1]) / 2)


def test_nan_trajectory_is_left_alone(gpu_ctx):
    X, U, t, _ = problem(6, 30, 3, False)
    X = X.copy(order="F")
    X[1, 5, 1] = np.nan
    for passes in (1, 2):
        r = resample(gpu_ctx, X, U, t, 17, passes=passes)
        assert list(r.status) == [0, 2, 0]
        assert np.isnan(r.X[:, :, 1]).all() and np.isnan(r.U[:, :, 1]).all() and np.isnan(r.t[:, 1]).all() and np.isnan(r.errors_after[:, 1]).all()
        for b in (0, 2):
            one = resample(gpu_ctx, X[:, :, b], U[:, :, b], t[:, b], 17, passes=passes)
            assert one.status == 0 and same((one.X, one.U, one.t, one.errors_before, one.errors_after),
                                            (r.X[:, :, b], r.U[:, :, b], r.t[:, b], r.errors_before[:, b], r.errors_after[:, b]))
    # a NaN behind the valid part is never read into a result
    Xr, Ur, tr, n_in = problem(6, 30, 3, True)
    r = resample(gpu_ctx, Xr, Ur, tr, 17, n_in=n_in)
    assert np.all(r.status == 0) and np.isfinite(r.X).all() and np.isfinite(r.errors_after).all()


def test_refusals(gpu_ctx):
    X, U, t, _ = problem(6, 30, 3, False)
    X, U, t = X.copy(order="F"), U.copy(order="F"), t.copy(order="F")
    n_new = 17
    Xo = np.zeros((6, n_new, 3), order="F"); Uo = np.zeros((3, n_new, 3), order="F"); to = np.zeros((n_new, 3), order="F")
    prm = lto.LtoDirectParams(MU, DU, TU, ISP)
    fn = gpu_ctx.lib.lto_direct_resample_batch
    EINVAL, ENULL = lto._lib.LTO_EINVAL, lto._lib.LTO_ENULL
    ones = np.ones((29, 3), order="F")

    def call(nstate=6, cap=30, B=3, X=X, U=U, t=t, n_in=None, nsteps=10, prm=C.byref(prm), n_new=n_new, w=None, w_floor=0.1, passes=1,
             Xo=Xo, Uo=Uo, to=to):
        return fn(gpu_ctx.handle, nstate, cap, B, _ptr(X), _ptr(U), _ptr(t), _ptr(n_in), nsteps, prm, n_new, _ptr(w), w_floor, passes,
                  _ptr(Xo), _ptr(Uo), _ptr(to), None, None, None)

    assert call() == 0                                # the optional outputs may all be NULL
    assert call(w=ones) == 0
    t_nan, t_flat, w_neg, w_inf = t.copy(order="F"), t.copy(order="F"), ones.copy(order="F"), ones.copy(order="F")
    t_nan[4, 1], w_neg[3, 2], w_inf[0, 0] = np.nan, 0.0, np.inf
    t_flat[7, 0] = t_flat[6, 0]
    i32 = lambda *v: np.array(v, dtype=np.int32)    # noqa: E731
    for bad in (dict(nstate=5), dict(nstate=8), dict(cap=1), dict(B=0), dict(n_new=1), dict(passes=0), dict(nsteps=1),
                dict(w_floor=-0.1), dict(w_floor=1.0), dict(w_floor=np.nan), dict(w_floor=np.inf),
                dict(n_in=i32(30, 1, 30)), dict(n_in=i32(30, 31, 30)), dict(t=t_nan), dict(t=t_flat), dict(w=w_neg), dict(w=w_inf),
                dict(w=ones, passes=2), dict(B=65536), dict(cap=262146), dict(n_new=262146), dict(cap=262145, B=65535)):
        assert call(**bad) == EINVAL, bad
    for bad in (dict(X=None), dict(U=None), dict(t=None), dict(prm=None), dict(Xo=None), dict(Uo=None), dict(to=None)):
        assert call(**bad) == ENULL, bad
    # what lies behind a valid part is not looked at: a NaN time and a bad weight there pass
    assert call(n_in=i32(30, 4, 30), t=t_nan, w=None) == 0
    w_pad = ones.copy(order="F")
    w_pad[10, 1] = -1.0
    assert call(n_in=i32(30, 4, 30), w=w_pad) == 0
    assert gpu_ctx.lib.lto_direct_resample(None, 6, 30, _ptr(X), _ptr(U), _ptr(t), 10, C.byref(prm), n_new, None, 0.1, 1, _ptr(Xo),
                                           _ptr(Uo), _ptr(to), None, None, None) == ENULL
    with pytest.raises(ValueError):
        lto.direct_resample(X, U, t, MU=MU, DU=DU, TU=TU, Isp=ISP, n_new=17, n_in=[30, 30], ctx=gpu_ctx)


# ------------------------------------------------------------------------------------------------ the demo's three starts
def test_multi_start_refine_resample_resolve(gpu_ctx):
    """Solve three starts of the demo's 30-node transfer, refine the batch, resample it to 30 nodes each (two passes) and solve again
    with fixed ends: every start reaches status 0 with max defect <= 1e-6, and the largest estimate of a re-solved mesh does not
    exceed that of the solved input mesh.  Without the keyword the driver returns what it returned before."""
    a, b, c, d = DH.tables()
    tof = 10.0 * lto.day / TU
    args = ([0.70, 0.75, 0.80], tof, tof, 30, 10, 1000.0, ISP, a, b, c, d, MU, DU, TU)
    plain = drivers.multiStart_direct(*args, maxIter=100, ctx=gpu_ctx)
    assert "remesh" not in plain and "remesh_starts" not in plain
    m = drivers.multiStart_direct(*args, maxIter=100, ctx=gpu_ctx, remesh_nodes=30, then_indirect=True)
    for key, v in plain.items():
        assert np.asarray(v).tobytes() == np.asarray(m[key]).tobytes(), key
    assert np.all(m["status"] == 0)
    rm = m["remesh"]
    assert np.array_equal(m["remesh_starts"], [0, 1, 2])
    assert rm["X"].shape == (6, 30, 3) and rm["U"].shape == (3, 30, 3) and rm["t"].shape == (30, 3) and rm["errors"].shape == (29, 3)
    _, e_in = lto.direct_defectCalc(m["X"], m["U"], m["t"], 10, MU, DU, TU, ISP, ctx=gpu_ctx)
    for j in range(3):
        print("start %d: %d nodes refined; estimates of the solved mesh max %.3e min %.3e, of the re-solved mesh max %.3e min %.3e; "
              "re-solve status %d after %d iterations, max defect %.2e" % (
                  j, rm["nodes_refined"][j], e_in[:, j].max(), e_in[:, j].min(), rm["errors"][:, j].max(), rm["errors"][:, j].min(),
                  rm["status"][j], rm["iterations"][j], rm["max_defect"][j]))
    assert np.all(rm["resample_status"] == 0)
    assert np.all(rm["status"] == 0) and np.all(rm["max_defect"] <= 1e-6)
    assert np.all(rm["errors"].max(axis=0) <= e_in.max(axis=0))
    assert np.array_equal(rm["t"][[0, -1]], m["t"][[0, -1]])
    ind = m["indirect"]                               # the hand-over starts from the re-solved batch, not from the first solve
    print("indirect from the re-solved starts: status %s, iterations %s" % (ind["status"], ind["iterations"]))
    assert np.array_equal(m["indirect_starts"], [0, 1, 2]) and ind["XC"].shape == (12, 30, 3)
    assert not np.array_equal(rm["X"], m["X"]) and not np.array_equal(rm["t"], m["t"])
    assert np.array_equal(ind["seed"][:6], rm["X"])   # the seed's state rows are bit copies of the states handed over
    handed = drivers.direct_to_indirect(rm["X"], rm["U"], rm["t"], 10, 1000.0, ISP, MU, DU, TU, dV1=rm["dV"][:3], dV2=rm["dV"][3:],
                                        ctx=gpu_ctx)
    assert ind["seed"].tobytes() == handed["seed"].tobytes()      # and its costates come from the re-solved U, t and dV
    # the driver's one-trajectory form, from direct_refine's own result
    ref = lto.direct_refine(m["X"][:, :, 1], m["U"][:, :, 1], m["t"][:, 1], 10, MU, DU, TU, ISP, 1e-19, 1e-16, 120, ctx=gpu_ctx)
    X1, U1, t1, st = drivers.meshEquidistribute_direct(ref, None, None, 6, None, 10, ISP, MU, DU, TU, 30, ctx=gpu_ctx)
    assert st == 0 and X1.shape == (6, 30) and U1.shape == (3, 30) and t1.shape == (30,)
    X2, U2, t2, st2 = drivers.meshEquidistribute_direct(ref.X, ref.U, ref.t, 6, None, 10, ISP, MU, DU, TU, 30, ctx=gpu_ctx)
    assert st2 == 0 and same((X1, U1, t1), (X2, U2, t2))


def test_demo_equidistribute_resolves(gpu_ctx):
    import importlib.util
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "halo_direct_demo.py")
    spec = importlib.util.spec_from_file_location("halo_direct_demo_eq", path)
    demo = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(demo)
    out = demo.equidistribute_and_resolve(30, ctx=gpu_ctx, verbose=False)
    print(out)
    assert out["n_before"] == 30 and out["n_after"] == 30 and out["resample_status"] == 0
    assert out["status"] == 0 and out["max_defect"] <= 1e-6
    assert out["max_error_after"] <= out["max_error_before"]
