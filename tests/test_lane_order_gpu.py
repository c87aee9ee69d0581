"""The lane order of the adaptive sweeps and their step statistics, read back from the device and checked against
tests/lane_order_reference.py: lto_segment_order_dev (the launches of lto_indirect_plan_rebalance, on step counts of the test's
choosing), lto_indirect_plan_copy_order (the order a plan holds) and lto_step_stats_dev (k_step_stats).  Every device output is
prefilled with -1 and has room behind its extent: a position never written and a write outside the extent both show.  Outcomes are
exact integers; nothing is asserted about the place of equal keys or the rank of tied windows -- what the device chose there is
decoded by the checker.  The tests named *_entry_* never run a sweep."""
import ctypes

import numpy as np
import pytest

import lane_order_reference as R
import lowthrustopt_amd as lto
from lowthrustopt_amd import synth
from lowthrustopt_amd._lib import LTO_EINVAL, LTO_ENULL

pytestmark = pytest.mark.gpu

PAD = 37
MU, DU, TU = lto.MU, lto.DU, lto.TU


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


def blank(n):
    import torch
    return torch.full((n,), -1, dtype=torch.int32, device="cuda")


def host(x):
    import torch
    torch.cuda.synchronize()
    return x.cpu().numpy()


def refused(code, call):
    with pytest.raises(lto.LtoError) as ei:
        call()
    assert ei.value.code == code, (ei.value.code, code, str(ei.value))


def device_order(ctx, kind, acc, rej, weave=0, out=None):
    """The order the device builds for these step counts; the room behind it must come back untouched."""
    S = len(acc)
    out = blank(S + PAD) if out is None else out
    lto.segment_order(ctx, kind, dev(acc), dev(rej), out, S, weave=weave)
    got = host(out)
    assert np.all(got[S:] == -1), "write behind the order's extent: positions %s" % (S + np.flatnonzero(got[S:] != -1)[:8])
    return got[:S].astype(np.int64)


# ------------------------------------------------------------------------------------------------ global order
@pytest.mark.parametrize("pattern", R.GLOBAL_PATTERNS)
@pytest.mark.parametrize("S", R.GLOBAL_SIZES)
def test_entry_global_order(gpu_ctx, S, pattern):
    acc, rej = R.step_counts(pattern, S)
    keys = R.keys_of(acc, rej)
    order = device_order(gpu_ctx, 1, acc, rej)
    R.check_global(order, keys)
    if np.unique(keys).size == S:                      # no ties: one valid order
        assert np.array_equal(order, R.model_global(keys))
    if pattern == "distinct":
        assert (np.unique(keys).size == S) == (S <= 1024)
    if pattern in ("heavy-first", "heavy-last") and S > 1:
        assert order[0] == (0 if pattern == "heavy-first" else S - 1)


def test_entry_global_order_ignores_weave_and_repeats(gpu_ctx):
    """kind 1 takes any valid weave and ignores it; the same call again, and again behind a windowed order of another size that
    left the shared workspace full, passes again."""
    acc, rej = R.step_counts("distinct", 1023)
    keys = R.keys_of(acc, rej)
    ref = R.model_global(keys)
    for weave in (0, 7, 255, 0):
        assert np.array_equal(device_order(gpu_ctx, 1, acc, rej, weave), ref)
        a2, r2 = R.step_counts("clamped", 8193)
        R.check_windowed(device_order(gpu_ctx, 2, a2, r2), R.keys_of(a2, r2))


# ------------------------------------------------------------------------------------------------ windowed order
@pytest.mark.parametrize("pattern", R.WINDOWED_PATTERNS)
@pytest.mark.parametrize("S,weave", R.WINDOWED_CASES)
def test_entry_windowed_order(gpu_ctx, S, weave, pattern):
    acc, rej = R.step_counts(pattern, S)
    keys = R.keys_of(acc, rej)
    L = R.Layout(S, weave)
    order = device_order(gpu_ctx, 2, acc, rej, weave)
    ranks = R.check_windowed(order, keys, weave)
    assert sorted(ranks.tolist()) == list(range(L.nwin))
    if L.has_short:
        assert ranks[L.nwin - 1] == L.nwin - 1                # the short window ranks last whatever it holds
    if R.keys_distinct_in_windows(keys):                   # given the ranks the device chose, every position is determined
        assert np.array_equal(order, R.build_windowed(keys, weave, ranks))
        if R.window_keys_distinct(keys):                   # and so are the ranks
            assert np.array_equal(order, R.model_windowed(keys, weave))
    if pattern == "window-distinct":
        assert R.keys_distinct_in_windows(keys)
        assert R.window_keys_distinct(keys) == (L.nfull <= R.BINS + 1 - min(L.W, S))      # (more windows than bins left: ties)


@pytest.mark.parametrize("S,weave", [(145, 0), (900, 0), (8193, 0), (33000, 3), (140000, 0)])
def test_entry_windowed_order_twice(gpu_ctx, S, weave):
    """The same call twice, into the same output and with the workspace the first call left, passes again; so does another
    input in between."""
    import torch
    acc, rej = R.step_counts("ten-keys", S)
    keys = R.keys_of(acc, rej)
    out = blank(S + PAD)
    first = device_order(gpu_ctx, 2, acc, rej, weave, out)
    R.check_windowed(first, keys, weave)
    a2, r2 = R.step_counts("window-distinct", S)
    R.check_windowed(device_order(gpu_ctx, 2, a2, r2, weave), R.keys_of(a2, r2), weave)
    out.fill_(-1)
    torch.cuda.synchronize()
    R.check_windowed(device_order(gpu_ctx, 2, acc, rej, weave, out), keys, weave)


# ------------------------------------------------------------------------------------------------ through a plan
def small_plan(ctx, ndim, integ):
    import torch
    n, B = 65, 3
    XC, T = synth.indirect_problem(n, n_batch=B, seed=41, dt_range=(0.02, 0.5))
    if ndim == 14:
        X = np.zeros((14, n, B), order="F")
        X[:6] = XC[:6]; X[6] = 1000.0; X[7:13] = XC[6:]; X[13] = 0.2
        slot = 2000.0
    else:
        X, slot = XC, 1000.0
    prms = [lto.make_params(MU, DU, TU, 0.05, slot, 1.0, 1.0 if b != 1 else 2.0, 10.0 ** -b) for b in range(B)]
    plan = lto.IndirectPlan(ctx, n, B, prms, integ, ndim=ndim)
    Xd = torch.from_numpy(synth.to_soa_nodes(X)).cuda()
    td = torch.from_numpy(np.ascontiguousarray(T.T.reshape(-1))).cuda()
    return plan, Xd, td, n, B


@pytest.mark.parametrize("ndim", [12, 14])
def test_plan_order_read_back(gpu_ctx, ndim):
    """What lto_indirect_plan_rebalance leaves in the plan: the windowed order after defect sweeps, the global one once an STM
    sweep has run, for the plan's own step counts.  Every order is read back and checked before it is dropped again
    (reset_order): no sweep of this test runs on an order."""
    import torch
    plan, Xd, td, n, B = small_plan(gpu_ctx, ndim, lto.integrator())
    S = (n - 1) * B
    untouched = np.full(S + PAD, -1, dtype=np.int32)

    def read():
        out = np.full(S + PAD, -1, dtype=np.int32)
        kind, got = plan.copy_order(out=out)
        assert got is out and np.all(out[S:] == -1)
        return kind, out[:S].astype(np.int64), out

    kind, _, out = read()
    assert kind == 0 and np.array_equal(out, untouched)                  # never rebalanced
    d = torch.zeros(ndim, S, dtype=torch.float64, device="cuda")
    plan.defect(Xd, n * B, td, B, d, S)
    acc, rej = plan.step_counts()
    assert (acc + rej).max() > (acc + rej).min() > 0                     # the step counts really differ across segments
    plan.rebalance()
    kind, order, _ = read()
    assert kind == 2
    R.check_windowed(order, R.keys_of(acc, rej), 0)
    assert plan.copy_order()[0] == 2 and np.array_equal(plan.copy_order()[1], order)
    plan.reset_order()
    kind, _, out = read()
    assert kind == 0 and np.array_equal(out, untouched)
    assert plan.copy_order() == (0, None)
    Phi = torch.zeros(ndim * ndim, S, dtype=torch.float64, device="cuda")
    plan.jacobian(Xd, n * B, td, B, Phi, S, d, S)
    acc, rej = plan.step_counts()
    assert (acc + rej).max() > (acc + rej).min() > 0
    plan.rebalance()
    kind, order, _ = read()
    assert kind == 1
    R.check_global(order, R.keys_of(acc, rej))
    plan.reset_order()
    assert read()[0] == 0
    plan.close()


def test_plan_order_of_a_fixed_step_plan_and_refusals(gpu_ctx):
    plan, Xd, td, n, B = small_plan(gpu_ctx, 12, lto.integrator(lto.RK4, steps=4))
    S = (n - 1) * B
    out = np.full(S, -1, dtype=np.int32)
    assert plan.copy_order(out=out)[0] == 0 and np.all(out == -1)
    fn, kind = gpu_ctx.lib.lto_indirect_plan_copy_order, ctypes.c_int(-9)
    assert fn(None, None, out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(kind)) == LTO_ENULL
    refused(LTO_ENULL, lambda: gpu_ctx.check(fn(plan.handle, None, out.ctypes.data_as(ctypes.c_void_p), None)))
    assert fn(plan.handle, None, None, ctypes.byref(kind)) == 0 and kind.value == 0      # natural order: no array needed
    for wrong in (np.full(S - 1, -1, dtype=np.int32), np.full(S, -1, dtype=np.int64), np.full(2 * S, -1, dtype=np.int32)[::2]):
        refused(LTO_EINVAL, lambda: plan.copy_order(out=wrong))
    plan.close()
    # a plan that holds an order refuses a NULL array and leaves kind_out alone
    import torch
    plan, Xd, td, n, B = small_plan(gpu_ctx, 12, lto.integrator())
    d = torch.zeros(12, S, dtype=torch.float64, device="cuda")
    plan.defect(Xd, n * B, td, B, d, S)
    plan.rebalance()
    kind = ctypes.c_int(-9)
    refused(LTO_ENULL, lambda: gpu_ctx.check(fn(plan.handle, None, None, ctypes.byref(kind))))
    assert kind.value == -9
    assert plan.copy_order(out=out)[0] == 2
    R.check_windowed(out, R.keys_of(*plan.step_counts()), 0)
    plan.reset_order()
    plan.close()


# ------------------------------------------------------------------------------------------------ step statistics
# one workgroup per 4 096 segments up to 64: 262 144 segments are the last size with one trip per thread, 262 145 the first with two
STATS_SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 262144, 262145]


def stats_inputs(S, where, seed=0):
    rng = np.random.default_rng([seed, S])
    acc = rng.integers(0, 400, S).astype(np.int32)
    rej = rng.integers(0, 40, S).astype(np.int32)
    if where != "anywhere":
        acc[0 if where == "first" else S - 1] = 977
    return acc, rej


@pytest.mark.parametrize("where", ["anywhere", "first", "last"])
@pytest.mark.parametrize("S", STATS_SIZES)
def test_entry_step_stats(gpu_ctx, S, where):
    acc, rej = stats_inputs(S, where)
    ref = R.step_stats(acc, rej)
    if where != "anywhere":
        assert ref[1] == 977 + int(rej[0 if where == "first" else S - 1])
    got = lto.step_stats(gpu_ctx, dev(acc), dev(rej), S)
    assert got.tolist() == ref


def test_entry_step_stats_sum_past_2_to_31_zeros_and_calls_in_a_row(gpu_ctx):
    S = 262145
    big = np.full(S, 10000, dtype=np.int32)
    zero = np.zeros(S, dtype=np.int32)
    ref = R.step_stats(big, zero)
    assert ref[0] > 2 ** 31
    assert lto.step_stats(gpu_ctx, dev(big), dev(zero), S).tolist() == ref
    assert lto.step_stats(gpu_ctx, dev(zero), dev(zero), S).tolist() == [0, 0, S]
    assert lto.step_stats(gpu_ctx, dev(zero), dev(zero), 1).tolist() == [0, 0, 1]
    # calls in a row on one context, different inputs and sizes: each is right on its own (the last workgroup's reset)
    for S2, where, seed in ((4097, "first", 1), (65, "last", 2), (262145, "anywhere", 3), (4096, "anywhere", 4), (262145, "last", 5)):
        acc, rej = stats_inputs(S2, where, seed)
        assert lto.step_stats(gpu_ctx, dev(acc), dev(rej), S2).tolist() == R.step_stats(acc, rej), (S2, where)


# ------------------------------------------------------------------------------------------------ refusals
def test_entry_refusals_leave_outputs_untouched(gpu_ctx):
    S = 300
    acc, rej = R.step_counts("ten-keys", S)
    a, r, out = dev(acc), dev(rej), blank(S + PAD)
    h, fn = gpu_ctx.handle, gpu_ctx.lib.lto_segment_order_dev

    def order(kind=2, weave=0, n=S, a_=a, r_=r, out_=out, h_=h):
        p = lambda v: None if v is None else v.data_ptr()          # noqa: E731
        return fn(h_, kind, weave, n, p(a_), p(r_), p(out_), None)

    assert order(h_=None) == LTO_ENULL
    for kw in (dict(a_=None), dict(r_=None), dict(out_=None)):
        refused(LTO_ENULL, lambda: gpu_ctx.check(order(**kw)))
    for kw in (dict(kind=0), dict(kind=3), dict(kind=-1), dict(weave=-1), dict(weave=256), dict(kind=1, weave=256), dict(n=0), dict(n=-5)):
        refused(LTO_EINVAL, lambda: gpu_ctx.check(order(**kw)))
    assert np.all(host(out) == -1)
    gpu_ctx.check(order())
    R.check_windowed(host(out)[:S], R.keys_of(acc, rej))

    fn = gpu_ctx.lib.lto_step_stats_dev
    res = np.full(3, -1, dtype=np.int64)

    def stats(n=S, a_=a, r_=r, res_=res, h_=h):
        p = lambda v: None if v is None else v.data_ptr()          # noqa: E731
        return fn(h_, n, p(a_), p(r_), None if res_ is None else res_.ctypes.data_as(ctypes.c_void_p), None)

    assert stats(h_=None) == LTO_ENULL
    for kw in (dict(a_=None), dict(r_=None), dict(res_=None)):
        refused(LTO_ENULL, lambda: gpu_ctx.check(stats(**kw)))
    for kw in (dict(n=0), dict(n=-1)):
        refused(LTO_EINVAL, lambda: gpu_ctx.check(stats(**kw)))
    assert res.tolist() == [-1, -1, -1]
    for wrong in (np.zeros(2, dtype=np.int64), np.zeros(3, dtype=np.int32), np.zeros(6, dtype=np.int64)[::2]):
        refused(LTO_EINVAL, lambda: lto.step_stats(gpu_ctx, a, r, S, out=wrong))
    gpu_ctx.check(stats())
    assert res.tolist() == R.step_stats(acc, rej)
