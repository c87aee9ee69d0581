"""The device Newton solve (launch_bvp_solve, kernels_bvp.hip) across its launch sequences, in all four variants <12,12>, <12,6>,
<14,14> and <14,7>, against the refined sparse host reference of bvp_reference.py.

The segment counts S per trajectory are read against bvp_solve_impl: a problem of at most 16 segments is one tail launch; above
that every k_bvp_chunk launch reduces 16 rows (four levels) to one, and one k_bvp_backchunk launch per chunk launch runs back down.
  1, 2, 15, 16         tail only (k_bvp_rows0 / k_bvp_rhs0, k_bvp_tail)
  17, 33               one chunk launch whose last workgroup carries a single row up four levels (S = 16k + 1)
  31, 32, 255, 256     one chunk launch (256: the largest)
  257, 271             two: k_bvp_chunk<*, false> / k_bvp_chunk_rhs<*, false> and k_bvp_backchunk at level0 = 4
  4095, 4096           two, 256 rows into the tail
  4097                 three: level0 = 0, 4, 8 (4097 -> 257 -> 17 -> 2 rows), each with a carried row
Each case: the factor solve into a NaN-poisoned delta and the re-solve (Phi = None, the SOC step) of an unrelated right-hand side,
both against the reference; a second factorisation is bitwise equal to the first; where a chunk launch starts, padded leading
dimensions give bitwise the same solution, never read the input padding and never write the output padding.  Batches of
different systems equal their single solves bitwise, and the sweep's own STMs are checked at 257 and 4097 segments."""
import numpy as np
import pytest

import lowthrustopt_amd as lto
from lowthrustopt_amd import drivers, synth
from lowthrustopt_amd.constants import MU, DU, TU

import bvp_reference as R

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 15, 16, 17, 31, 32, 33, 255, 256, 257, 271, 4095, 4096, 4097]
PADDED = (17, 257, 4097)           # a chunk launch starts: first, second, third
BATCHES = [(17, 3), (257, 4), (4097, 2)]
TOL = 1e-11                        # synthetic systems: forward error / max(1, |x_ref|_inf)
SENTINEL = -7.25e300


def _prm(nd):
    return lto.make_params(MU, DU, TU, 0.05, 2000.0 if nd == 14 else 1000.0, 1.0, 1.0, 1.0)


def _plan(ctx, nd, n, B):
    return lto.IndirectPlan(ctx, n, B, _prm(nd), lto.integrator(lto.RKF78_FIXED, steps=4), ndim=nd)


def _system(family, nd, S, seed, adj):
    """Phi [nd, nd, S], the defect of the factor solve and an unrelated defect for the re-solve (same distribution)."""
    Phi, d = R.GENERATORS[family](nd, S, seed, adj)
    rng = np.random.default_rng(seed + 100003)
    d2 = rng.integers(-3, 4, size=d.shape).astype(np.float64) if family == "permutation" else rng.standard_normal(d.shape)
    return Phi, d, d2


def _phi_to_device(Phis, ldp):
    """List of per-trajectory Phi [nd, nd, S] -> SoA device array [nd*nd][ldp], row pc*nd + r, segment b*S + i; NaN padding."""
    import torch
    nd, _, S = Phis[0].shape
    P = np.full((nd * nd, ldp), np.nan)
    P[:, :len(Phis) * S] = np.stack(Phis, axis=3).transpose(1, 0, 3, 2).reshape(nd * nd, -1)
    return torch.from_numpy(P).cuda()


def _defect_to_device(ds, ldd):
    """List of per-trajectory defects [nd, S] -> SoA device array [nd][ldd], segment b*S + i; NaN padding."""
    import torch
    nd, S = ds[0].shape
    D = np.full((nd, ldd), np.nan)
    D[:, :len(ds) * S] = np.stack(ds, axis=2).transpose(0, 2, 1).reshape(nd, -1)
    return torch.from_numpy(D).cuda()


def _delta(nd, n, B, ldx):
    import torch
    x = np.full((nd, ldx), SENTINEL)
    x[:, :B * n] = np.nan
    return torch.from_numpy(x).cuda()


def _solve(plan, Phis, ds, d2s, adj, pad=False):
    """Factor solve of (Phis, ds) and re-solve of d2s; returns the two [nd, ldx] host arrays."""
    import torch
    nd, _, S = Phis[0].shape
    B, n = len(Phis), S + 1
    ldp, ldd, ldx = (B * S + 5, B * S + 3, B * n + 7) if pad else (B * S, B * S, B * n)
    Phi, d, d2 = _phi_to_device(Phis, ldp), _defect_to_device(ds, ldd), _defect_to_device(d2s, ldd)
    x1, x2 = _delta(nd, n, B, ldx), _delta(nd, n, B, ldx)
    plan.newton_solve(Phi, ldp, d, ldd, x1, ldx, adjoints_only=adj)
    plan.newton_solve(None, 0, d2, ldd, x2, ldx, adjoints_only=adj)
    torch.cuda.synchronize()
    out = []
    for x in (x1, x2):
        x = x.cpu().numpy()
        assert np.all(x[:, B * n:] == SENTINEL), "output padding written"
        out.append(x[:, :B * n].reshape(nd, B, n).transpose(0, 2, 1))          # [nd, n, B]
    return out


def _check(x, ref, dd, adj, nd, tol, what):
    """Finite, pinned entries exactly 0 (adjoints-only: every state row too), forward error against the reference.
    Returns the relative forward error."""
    assert np.all(np.isfinite(x)), what
    free = R.free_mask(nd, x.shape[1], adj)
    assert np.all(x[~free] == 0.0), what
    xr, err = ref.solve(dd)
    scale = max(1.0, np.abs(xr).max())
    assert err < 0.01 * tol * scale, (what, "reference", err)
    e = np.abs(x - xr).max() / scale
    assert e <= tol, (what, e)
    return e


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("nd,adj", R.VARIANTS, ids=[R.variant_name(*v) for v in R.VARIANTS])
def test_synthetic_shape_sweep(gpu_ctx, nd, adj, S):
    plan = _plan(gpu_ctx, nd, S + 1, 1)
    try:
        for k, family in enumerate(sorted(R.GENERATORS)):
            Phi, d, d2 = _system(family, nd, S, 1000 * S + 10 * nd + 2 * adj + k, adj)
            ref = R.BvpReference(Phi, adj)
            x1, x2 = _solve(plan, [Phi], [d], [d2], adj)
            e1 = _check(x1[:, :, 0], ref, d, adj, nd, TOL, (family, "factor"))
            e2 = _check(x2[:, :, 0], ref, d2, adj, nd, TOL, (family, "re-solve"))
            print("\nbvp-shapes %s S=%d %s: factor %.2e re-solve %.2e" % (R.variant_name(nd, adj), S, family, e1, e2))
            # a second factorisation (and re-solve) of the same input: bitwise the same
            y1, y2 = _solve(plan, [Phi], [d], [d2], adj)
            assert np.array_equal(x1, y1) and np.array_equal(x2, y2), family
            if S in PADDED:            # NaN input padding never read, output padding never written, bitwise the same solution
                p1, p2 = _solve(plan, [Phi], [d], [d2], adj, pad=True)
                assert np.array_equal(x1, p1) and np.array_equal(x2, p2), family
    finally:
        plan.close()


@pytest.mark.parametrize("S,B", BATCHES)
@pytest.mark.parametrize("nd,adj", R.VARIANTS, ids=[R.variant_name(*v) for v in R.VARIANTS])
def test_batch_of_different_systems(gpu_ctx, nd, adj, S, B):
    """One system per trajectory, the two families alternating: trajectory b of the batch == the same system solved alone, bitwise
    (nothing reduces across trajectories), and == the reference."""
    fams = sorted(R.GENERATORS)
    systems = [_system(fams[b % 2], nd, S, 77 + 13 * b + nd + adj, adj) for b in range(B)]
    plan = _plan(gpu_ctx, nd, S + 1, B)
    try:
        x1, x2 = _solve(plan, [s[0] for s in systems], [s[1] for s in systems], [s[2] for s in systems], adj)
    finally:
        plan.close()
    single = _plan(gpu_ctx, nd, S + 1, 1)
    try:
        for b, (Phi, d, d2) in enumerate(systems):
            y1, y2 = _solve(single, [Phi], [d], [d2], adj)
            assert np.array_equal(x1[:, :, b], y1[:, :, 0]) and np.array_equal(x2[:, :, b], y2[:, :, 0]), b
            ref = R.BvpReference(Phi, adj)
            _check(x1[:, :, b], ref, d, adj, nd, TOL, (b, "factor"))
            _check(x2[:, :, b], ref, d2, adj, nd, TOL, (b, "re-solve"))
    finally:
        single.close()


def _sweep(ctx, nd, n, seed):
    """The device sweep's STMs and defect of one trajectory (RKF7(8) fixed step): 12-dim synth.indirect_problem, 14-dim lifted
    to the variable-mass system as test_indirect_mass_gpu.guess14 does.  Returns Phi [nd, nd, S], defect [nd, S] (host)."""
    import torch
    XC, T = synth.indirect_problem(n, n_batch=1, seed=seed, dt_range=(0.05, 0.2))
    if nd == 14:
        XC = drivers.lift_to_mass(XC, 1000.0)
        XC[6] -= 0.01 * np.arange(n)[:, None]
        XC[13] = 0.2
        XC[13, -1] = 0.0
    S = n - 1
    plan = lto.IndirectPlan(ctx, n, 1, _prm(nd), lto.integrator(lto.RKF78_FIXED, steps=4 if n > 1000 else 6), ndim=nd)
    try:
        X = torch.from_numpy(synth.to_soa_nodes(XC)).cuda()
        t = torch.from_numpy(np.ascontiguousarray(T.T)).cuda()
        Phi = torch.zeros(nd * nd, S, dtype=torch.float64, device="cuda")
        d = torch.zeros(nd, S, dtype=torch.float64, device="cuda")
        plan.jacobian(X, n, t, 1, Phi, S, d, S)
        torch.cuda.synchronize()
    finally:
        plan.close()
    return np.asfortranarray(Phi.cpu().numpy().reshape(nd, nd, S).transpose(1, 0, 2)), d.cpu().numpy()


def _backward_ok(ref, x, d, what):
    """Long-double backward error: |J x - b| (square) or |J^T (J x - b)| (least squares) against 1e-9 * scale."""
    b = -d.reshape(-1, order="F")
    jmax = np.abs(ref.J).max()
    scale = jmax * np.abs(x).max() + np.abs(b).max()
    if ref.adjoints_only:
        scale *= jmax
    be = ref.backward_error(x, d)
    assert be < 1e-9 * scale, (what, be, scale)


@pytest.mark.parametrize("nd,S,check_forward", [(12, 257, True), (14, 257, True), (14, 4097, False)])
def test_sweep_stms(gpu_ctx, nd, S, check_forward):
    """The device sweep's STMs (conditioning of the real problem): at 257 segments forward error against the reference at 1e-7
    and backward error; at 4 097 segments (650 TU, conditioning unknown) the backward error only, as the 12-dim 4 096 test."""
    Phi, d = _sweep(gpu_ctx, nd, S + 1, 45)
    d2 = 0.5 * d + 0.01
    for adj in (False, True):
        ref = R.BvpReference(Phi, adj)
        plan = _plan(gpu_ctx, nd, S + 1, 1)
        try:
            x1, x2 = _solve(plan, [Phi], [d], [d2], adj)
        finally:
            plan.close()
        for x, dd, what in ((x1[:, :, 0], d, "factor"), (x2[:, :, 0], d2, "re-solve")):
            assert np.all(np.isfinite(x)), what
            assert np.all(x[~R.free_mask(nd, S + 1, adj)] == 0.0), what
            _backward_ok(ref, x, dd, (adj, what))
            if check_forward:
                xr, _ = ref.solve(dd)
                assert np.abs(x - xr).max() < 1e-7 * max(1.0, np.abs(xr).max()), (adj, what)
