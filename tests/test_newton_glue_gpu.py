"""Shape sweep of the public glue entries of the Newton loops -- lto_trial_points_dev, lto_defect_norms_dev,
lto_line_search_pick_dev (both branches: k_take_trial with a defect block, k_pick_alpha without), lto_pack_soa_dev /
lto_unpack_soa_dev and lto_axpy_dev -- against tests/newton_loop_reference.py.  Every output array has room behind its extent
(ld > count) and is filled with a sentinel first, so that a write outside the extent shows; every refusal must leave it untouched."""
import numpy as np
import pytest

import newton_loop_reference as R
import lowthrustopt_amd as lto
from lowthrustopt_amd._lib import LTO_EINVAL, LTO_ENULL

pytestmark = pytest.mark.gpu

SENTINEL = -7.25


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def filled(rows, cols, value=SENTINEL):
    import torch
    return torch.full((rows, cols), value, dtype=torch.float64, device="cuda")


def host(x):
    import torch
    torch.cuda.synchronize()
    return x.cpu().numpy()


def same(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def refused(code, call):
    with pytest.raises(lto.LtoError) as ei:
        call()
    assert ei.value.code == code, (ei.value.code, code, str(ei.value))


# ------------------------------------------------------------------------------------------------ trial points
TRIAL_SHAPES = [(ndim, n, B, na) for ndim in (12, 14) for n in (2, 3, 64, 65) for B in (1, 3) for na in (1, 20)]


def trial_inputs(ndim, n, B, na):
    """(X, delta [ndim x n x B], alphas [na]): the library's step lengths (one of them for na = 1); steps of the nodes' own size, so
    that the product's rounding shows in about a fifth of the sums."""
    rng = np.random.default_rng(1000 * ndim + 10 * n + B + 7 * na)
    X = rng.standard_normal((ndim, n, B))
    delta = 0.5 * rng.standard_normal((ndim, n, B))
    alphas = R.ALPHAS.copy() if na == R.NA else R.ALPHAS[7:7 + na].copy()
    return X, delta, alphas


def fma_sensitive_elements(shapes):
    """Elements of the trial points where the fused result differs from x + a*d rounded twice."""
    count = 0
    for shape in shapes:
        X, delta, alphas = trial_inputs(*shape)
        al = alphas[None, None, :, None]
        count += int(np.sum(R.trial_points(X, delta, alphas) != R.twice_rounded(al, delta[:, :, None, :], X[:, :, None, :])))
    return count


FMA_SHAPES = [s for s in TRIAL_SHAPES if s[1] <= 3]          # the small half of the sweep: cheap to count, enough to tell


def run_trial_points(ctx, X, delta, alphas):
    ndim, n, B = X.shape
    na = len(alphas)
    ld, ldt = n * B + 3, n * B * na + 5
    Xs = np.full((ndim, ld), np.nan); Xs[:, :n * B] = R.to_soa(X)
    ds = np.full((ndim, ld), np.nan); ds[:, :n * B] = R.to_soa(delta)
    Xt = filled(ndim, ldt)
    lto.trial_points(ctx, dev(Xs), dev(ds), ld, ndim, n, B, dev(alphas), Xt, ldt)
    return host(Xt)


@pytest.mark.parametrize("ndim,n,B,na", TRIAL_SHAPES)
def test_trial_points_equal_the_exact_fma(gpu_ctx, ndim, n, B, na):
    X, delta, alphas = trial_inputs(ndim, n, B, na)
    got = run_trial_points(gpu_ctx, X, delta, alphas)
    ref = R.trials_to_soa(R.trial_points(X, delta, alphas))
    assert same(got[:, :n * B * na], ref)
    assert np.all(got[:, n * B * na:] == SENTINEL)


def test_trial_points_inputs_tell_the_fma_from_two_roundings():
    count = fma_sensitive_elements(FMA_SHAPES)
    print("trial points: %d elements of the small shapes differ between the fma and two roundings" % count)
    assert count >= 100


def test_trial_points_past_the_grid_cap_and_nan_in_one_trajectory(gpu_ctx):
    """2 184 000 elements: more than 8 192 workgroups of 256, so the grid-stride loop takes a second trip.  The step lengths are
    powers of two: the product is exact and numpy's a*d + x is the fma."""
    ndim, n, B, na = 14, 300, 26, 20
    assert ndim * n * B * na > 8192 * 256
    rng = np.random.default_rng(5)
    X = rng.standard_normal((ndim, n, B))
    delta = rng.standard_normal((ndim, n, B))
    delta[:, :, 17] = np.nan
    alphas = 2.0 ** -np.arange(na)
    got = run_trial_points(gpu_ctx, X, delta, alphas)
    ref = R.trials_to_soa(alphas[None, None, :, None] * delta[:, :, None, :] + X[:, :, None, :])
    per = na * n
    assert np.all(np.isnan(got[:, 17 * per:18 * per]))
    assert not np.isnan(got[:, :17 * per]).any() and not np.isnan(got[:, 18 * per:B * per]).any()
    assert same(got[:, :B * per], ref)
    assert np.all(got[:, B * per:] == SENTINEL)


def test_trial_points_refusals(gpu_ctx):
    ndim, n, B, na = 12, 5, 2, 20
    X = dev(np.ones((ndim, n * B))); d = dev(np.ones((ndim, n * B))); al = dev(R.ALPHAS)
    Xt = filled(ndim, n * B * na + 2)
    ld, ldt = n * B, n * B * na + 2
    h, fn = gpu_ctx.handle, gpu_ctx.lib.lto_trial_points_dev

    def call(X_=X, d_=d, ld_=ld, ndim_=ndim, n_=n, B_=B, na_=na, al_=al, Xt_=Xt, ldt_=ldt):
        p = lambda v: None if v is None else v.data_ptr()          # noqa: E731
        gpu_ctx.check(fn(h, None, p(X_), p(d_), ld_, ndim_, n_, B_, na_, p(al_), p(Xt_), ldt_))

    for kw in (dict(X_=None), dict(d_=None), dict(al_=None), dict(Xt_=None)):
        refused(LTO_ENULL, lambda: call(**kw))
    for kw in (dict(ndim_=0), dict(n_=0), dict(B_=0), dict(na_=0), dict(ld_=n * B - 1), dict(ldt_=n * B * na - 1)):
        refused(LTO_EINVAL, lambda: call(**kw))
    assert np.all(host(Xt) == SENTINEL)
    call()
    assert np.all(host(Xt)[:, :n * B * na] == 1.0 + np.tile(np.repeat(R.ALPHAS, n), B))


# ------------------------------------------------------------------------------------------------ defect norms
NORM_SHAPES = ([(ndim, 65, B) for ndim in (1, 6, 7, 12, 14, 16, 17, 33) for B in (1, 2, 257)]
               + [(ndim, seg, B) for ndim in (12, 17) for seg in (1, 63, 64, 1023, 1024, 1025, 2049) for B in (1, 2)]
               + [(12, 1, 257), (17, 63, 257), (12, 64, 257), (12, 1, 4100)])


def norm_inputs(ndim, seg, B, seed=0):
    rng = np.random.default_rng(100000 * seed + 1000 * ndim + seg + B)
    return rng.standard_normal((ndim, seg, B)) * 10.0 ** rng.integers(-6, 3, size=(1, 1, B))


def run_norms(ctx, D, want_ss=True, want_mx=True):
    ndim, seg, B = D.shape
    ldd = seg * B + 3
    Ds = np.full((ndim, ldd), np.nan); Ds[:, :seg * B] = R.to_soa(D)      # a read past the extent would surface as NaN
    ss, mx = filled(1, B + 2), filled(1, B + 2)
    lto.defect_norms(ctx, dev(Ds), ldd, ndim, seg, B, ss if want_ss else None, mx if want_mx else None)
    ss, mx = host(ss)[0], host(mx)[0]
    assert np.all(ss[B:] == SENTINEL) and np.all(mx[B:] == SENTINEL)
    return ss[:B], mx[:B]


@pytest.mark.parametrize("ndim,seg,B", NORM_SHAPES)
def test_defect_norms_shapes(gpu_ctx, ndim, seg, B):
    D = norm_inputs(ndim, seg, B)
    ss, mx = run_norms(gpu_ctx, D)
    worst = 0.0
    for b in range(B):
        exact = R.sumsq_exact(D[:, :, b])
        bound = ndim * seg * R.U * exact
        worst = max(worst, abs(ss[b] - exact) / bound)
    print("defect norms %d x %d x %d: largest |sumsq - exact| = %.3f of the bound N 2^-53 sum(v^2)" % (ndim, seg, B, worst))
    assert worst <= 1.0
    assert same(mx, [R.maxabs(D[:, :, b]) for b in range(B)])


@pytest.mark.parametrize("ndim,seg", [(12, 65), (17, 65), (33, 1025)])
def test_defect_norms_nan_stays_in_its_trajectory(gpu_ctx, ndim, seg):
    B = 3
    D = norm_inputs(ndim, seg, B, seed=1)
    ss0, mx0 = run_norms(gpu_ctx, D)
    places = [(0, 0), (ndim - 1, seg - 1)] + ([(16, seg // 2)] if ndim > 16 else [])
    for b in (0, B - 1):
        for row, i in places:
            Dn = D.copy()
            Dn[row, i, b] = np.nan
            ss, mx = run_norms(gpu_ctx, Dn)
            others = [q for q in range(B) if q != b]
            assert np.isnan(mx[b]) and np.array_equal(mx[others], mx0[others]), (b, row, i, mx)
            assert np.array_equal(ss[others], ss0[others]), (b, row, i)


def test_defect_norms_inf_zero_and_null_outputs(gpu_ctx):
    D = norm_inputs(17, 130, 3, seed=2)
    D[16, 129, 2] = -np.inf
    D[0, 0, 0] = np.inf
    ss, mx = run_norms(gpu_ctx, D)
    assert mx[0] == np.inf and mx[2] == np.inf and mx[1] == R.maxabs(D[:, :, 1])
    Z = np.full((14, 70, 2), -0.0)
    ss, mx = run_norms(gpu_ctx, Z)
    assert np.all(ss == 0.0) and np.all(mx == 0.0)
    D = norm_inputs(12, 65, 5, seed=3)
    ss_both, mx_both = run_norms(gpu_ctx, D)
    ss_only, untouched = run_norms(gpu_ctx, D, want_mx=False)
    assert np.array_equal(ss_only, ss_both) and np.all(untouched == SENTINEL)
    untouched, mx_only = run_norms(gpu_ctx, D, want_ss=False)
    assert np.array_equal(mx_only, mx_both) and np.all(untouched == SENTINEL)


# ------------------------------------------------------------------------------------------------ line-search pick
# (NA, B, seg) with 14 rows: 4 100 trajectories pass the 4 096-row cap of k_take_trial's grid, 1 300 segments the 64-workgroup cap in x
PICK_SHAPES = ([(na, B, 37) for na in (1, 2, 20, 64) for B in (1, 5)]
               + [(na, 4100, 1) for na in (1, 2, 20, 64)] + [(2, 4100, 37)]
               + [(20, 5, 1300), (2, 1, 1300), (64, 5, 1), (20, 1, 1)])
PATTERNS = ("min first", "min last", "min in the middle", "tie", "NaN in slot 0", "NaN elsewhere", "all NaN", "inf but one")


def crafted_sums(na, B, rng):
    ss = rng.uniform(1.0, 2.0, size=(B, na))
    for b in range(B):
        kind = PATTERNS[b % len(PATTERNS)]
        if kind == "min first":
            ss[b, 0] = 0.5
        elif kind == "min last":
            ss[b, na - 1] = 0.5
        elif kind == "min in the middle":
            ss[b, na // 2] = 0.5
        elif kind == "tie":
            ss[b, na // 3] = 0.5
            ss[b, na - 1] = 0.5
        elif kind == "NaN in slot 0":
            ss[b, 0] = np.nan
            ss[b, na - 1] = 0.5 if na > 1 else np.nan
        elif kind == "NaN elsewhere":
            k = min(1, na - 1)
            ss[b, k] = np.nan
            if na > 2:
                ss[b, k + 1] = 0.5
        elif kind == "all NaN":
            ss[b, :] = np.nan
        else:
            ss[b, :] = np.inf
            ss[b, na // 2] = 1.5
    return ss


@pytest.mark.parametrize("na,B,seg", PICK_SHAPES)
def test_line_search_pick_both_branches(gpu_ctx, na, B, seg):
    ndim = 14
    rng = np.random.default_rng(100 * na + B + seg)
    ss = crafted_sums(na, B, rng)
    mxt = rng.uniform(0.0, 1.0, size=(B, na))
    mxt[np.isnan(ss)] = np.nan
    alphas = R.ALPHAS if na == R.NA else np.sort(rng.uniform(0.05, 1.0, size=na))
    ldt, ldd = B * na * seg + 3, B * seg + 4
    trial = rng.standard_normal((ndim, ldt))
    best = [R.first_minimiser(ss[b]) for b in range(B)]
    for b in range(min(B, len(PATTERNS))):
        kind = PATTERNS[b]
        if kind in ("min first", "NaN in slot 0", "all NaN"):
            assert best[b] == 0
        elif kind == "tie":
            assert best[b] == na // 3
    step_ref = np.array([alphas[a] for a in best])
    mx_ref = np.array([mxt[b, best[b]] for b in range(B)])
    d_ss, d_mxt, d_al, d_trial = dev(ss.reshape(-1)), dev(mxt.reshape(-1)), dev(alphas), dev(trial)
    # with a defect block: k_take_trial
    step, mx, defect = filled(1, B + 2), filled(1, B + 2), filled(ndim, ldd)
    lto.line_search_pick(gpu_ctx, d_ss, d_mxt, d_al, d_trial, ldt, ndim, seg, B, step, mx, defect, ldd)
    step, mx, defect = host(step)[0], host(mx)[0], host(defect)
    assert np.array_equal(step[:B], step_ref) and np.all(step[B:] == SENTINEL)
    assert same(mx[:B], mx_ref) and np.all(mx[B:] == SENTINEL)
    cols = (np.arange(B)[:, None] * na + np.array(best)[:, None]) * seg + np.arange(seg)[None, :]
    assert np.array_equal(defect[:, :B * seg], trial[:, cols.reshape(-1)])
    assert np.all(defect[:, B * seg:] == SENTINEL)
    # without one: k_pick_alpha; the two branches agree
    step2, mx2 = filled(1, B + 2), filled(1, B + 2)
    lto.line_search_pick(gpu_ctx, d_ss, d_mxt, d_al, None, 0, ndim, seg, B, step2, mx2, None, 0)
    step2, mx2 = host(step2)[0], host(mx2)[0]
    assert np.array_equal(step2, step) and same(mx2, mx)
    # the maxabs pair NULL, in both branches
    step3, defect3 = filled(1, B + 2), filled(ndim, ldd)
    lto.line_search_pick(gpu_ctx, d_ss, None, d_al, d_trial, ldt, ndim, seg, B, step3, None, defect3, ldd)
    assert np.array_equal(host(step3)[0], step) and np.array_equal(host(defect3), defect)
    step4 = filled(1, B + 2)
    lto.line_search_pick(gpu_ctx, d_ss, None, d_al, None, 0, ndim, seg, B, step4, None, None, 0)
    assert np.array_equal(host(step4)[0], step)


def test_line_search_pick_refusals(gpu_ctx):
    na, B, seg, ndim = 20, 3, 7, 12
    ss, mxt, al = dev(np.ones(B * na)), dev(np.ones(B * na)), dev(R.ALPHAS)
    trial = dev(np.ones((ndim, B * na * seg)))
    step, mx, defect = filled(1, B), filled(1, B), filled(ndim, B * seg)
    ldt, ldd = B * na * seg, B * seg
    pick = lambda *a: lto.line_search_pick(gpu_ctx, *a)          # noqa: E731
    refused(LTO_ENULL, lambda: pick(None, mxt, al, trial, ldt, ndim, seg, B, step, mx, defect, ldd))
    refused(LTO_ENULL, lambda: pick(ss, mxt, al, trial, ldt, ndim, seg, B, None, mx, defect, ldd))
    refused(LTO_ENULL, lambda: pick(ss, mxt, al, trial, ldt, ndim, seg, B, step, None, defect, ldd))      # maxabs without maxabs_out
    refused(LTO_ENULL, lambda: pick(ss, None, al, trial, ldt, ndim, seg, B, step, mx, defect, ldd))
    refused(LTO_ENULL, lambda: pick(ss, mxt, al, trial, ldt, ndim, seg, B, step, mx, None, 0))            # trial_defect without defect
    refused(LTO_ENULL, lambda: pick(ss, mxt, al, None, 0, ndim, seg, B, step, mx, defect, ldd))
    refused(LTO_EINVAL, lambda: pick(ss, mxt, al, trial, ldt - 1, ndim, seg, B, step, mx, defect, ldd))
    refused(LTO_EINVAL, lambda: pick(ss, mxt, al, trial, ldt, ndim, seg, B, step, mx, defect, ldd - 1))
    refused(LTO_EINVAL, lambda: pick(ss, mxt, al, trial, ldt, ndim, 0, B, step, mx, defect, ldd))
    refused(LTO_EINVAL, lambda: pick(ss, mxt, al, trial, ldt, ndim, seg, 0, step, mx, defect, ldd))
    refused(LTO_EINVAL, lambda: pick(ss, mxt, al, trial, ldt, 0, seg, B, step, mx, defect, ldd))
    assert np.all(host(step) == SENTINEL) and np.all(host(mx) == SENTINEL) and np.all(host(defect) == SENTINEL)


# ------------------------------------------------------------------------------------------------ pack / unpack
# one pair per regime of tile_nodes: 256 nodes per tile, halved down to 32 for a small count, 224 and 56 (ndim 32: not a
# power of two), 32 / 31 / 15 nodes where the 64 KiB tile allows no more, a short last tile, one node, none
PACK_SHAPES = [(1, 0), (1, 1), (1, 31), (1, 16385), (1, 131073), (13, 33), (13, 16383), (13, 131073), (31, 33), (31, 131073),
               (32, 1), (32, 16385), (32, 131073), (255, 0), (255, 1), (255, 16383), (256, 31), (256, 16385), (512, 33), (512, 16383)]


@pytest.mark.parametrize("ndim,count", PACK_SHAPES)
def test_pack_unpack_shapes(gpu_ctx, ndim, count):
    import torch
    g = torch.Generator(device="cuda"); g.manual_seed(ndim + count)
    # node-contiguous == Julia [ndim x count]; the addresses are passed as such: an empty tensor has none, and the entry refuses NULL
    a_buf = torch.randn(max(count, 1), ndim, dtype=torch.float64, device="cuda", generator=g)
    a = a_buf[:count]
    ld = count + 5
    soa = filled(ndim, ld)
    lto.pack_soa(gpu_ctx, a_buf.data_ptr(), ndim, count, soa, ld)
    torch.cuda.synchronize()
    assert torch.equal(soa[:, :count], a.t()) and bool((soa[:, count:] == SENTINEL).all())
    back = filled(1, count * ndim + 7)
    lto.unpack_soa(gpu_ctx, soa, ld, ndim, count, back)
    torch.cuda.synchronize()
    assert torch.equal(back[0, :count * ndim].reshape(count, ndim), a) and bool((back[0, count * ndim:] == SENTINEL).all())


def test_pack_unpack_refuse_more_than_512_rows(gpu_ctx):
    a = dev(np.ones((5, 513)))
    soa = filled(513, 9)
    with pytest.raises(lto.LtoError):
        lto.pack_soa(gpu_ctx, a, 513, 5, soa, 9)
    back = filled(1, 5 * 513)
    with pytest.raises(lto.LtoError):
        lto.unpack_soa(gpu_ctx, soa, 9, 513, 5, back)
    refused(LTO_EINVAL, lambda: lto.pack_soa(gpu_ctx, a, 12, 5, soa, 4))          # ld < count
    refused(LTO_EINVAL, lambda: lto.unpack_soa(gpu_ctx, soa, 4, 12, 5, back))
    assert np.all(host(soa) == SENTINEL) and np.all(host(back) == SENTINEL)


# ------------------------------------------------------------------------------------------------ axpy
@pytest.mark.parametrize("count", [0, 1, 255, 257, 70001])
@pytest.mark.parametrize("alpha", [0.0, 1.0, -0.5, 0.1])
def test_axpy_equals_the_exact_fma(gpu_ctx, alpha, count):
    rng = np.random.default_rng(count + 3)
    x, d = rng.standard_normal(count), rng.standard_normal(count)
    y = filled(1, count + 6)
    dx, dd = (dev(x), dev(d)) if count else (y, y)           # (an empty tensor has no address: the entry would refuse NULL)
    gpu_ctx.check(gpu_ctx.lib.lto_axpy_dev(gpu_ctx.handle, None, dx.data_ptr(), dd.data_ptr(), alpha, y.data_ptr(), count))
    y = host(y)[0]
    assert np.array_equal(y[:count], R.fma_exact(alpha, d, x)) and np.all(y[count:] == SENTINEL)


def test_axpy_with_a_zero_step_is_still_the_fma(gpu_ctx):
    """lto_axpy_dev is launch_axpy: y = fma(alpha, d, x) for every element, whatever alpha is.  A NaN in d with alpha = 0 therefore
    gives NaN (0 x NaN); keeping a frozen trajectory's values over a NaN step is k_axpy_traj's rule, inside the loop
    (tests/test_newton_loop_steps_gpu.py), not this entry's."""
    x = np.arange(1.0, 9.0)
    d = np.ones(8); d[3] = np.nan; d[5] = np.inf
    y = filled(1, 10)
    dx, dd = dev(x), dev(d)
    gpu_ctx.check(gpu_ctx.lib.lto_axpy_dev(gpu_ctx.handle, None, dx.data_ptr(), dd.data_ptr(), 0.0, y.data_ptr(), 8))
    y = host(y)[0]
    keep = [0, 1, 2, 4, 6, 7]
    assert np.isnan(y[3]) and np.isnan(y[5]) and np.array_equal(y[keep], x[keep]) and np.all(y[8:] == SENTINEL)
    out = filled(1, 8)
    refused(LTO_ENULL, lambda: gpu_ctx.check(gpu_ctx.lib.lto_axpy_dev(gpu_ctx.handle, None, None, dd.data_ptr(), 1.0, out.data_ptr(), 8)))
    assert np.all(host(out) == SENTINEL)
