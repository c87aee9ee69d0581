"""The device QP step of the direct method (kernels_direct_qp.hip) across the levels of its reduction, in all six variants (frozen,
free ends, free tf; nstate 6 and 7), against the refined sparse host reference of qp_reference.py.

Segment counts S per trajectory, read against direct_qp_impl:
  1                             one carried level-0 row, no back substitution
  2 .. 9                        the first carried rows at levels 0, 1 and 2, and the clamped right node of k_qp_back
  13, 21, 43, 85                carried rows at alternating levels (binary 1101, 10101, ...)
  15 .. 17, 31 .. 33, 63 .. 65  either side of powers of two
  254 .. 257                    n = 255 .. 258: around one QP_FIN block and around the 256-wide grid of k_qp_gmax
  511 .. 513                    n = 512 .. 514: two blocks to three
Frozen step (lto_direct_qp_step_dev) on the three synthetic families of qp_reference.synthetic, ns in {6, 7}, impulses on and off:
finite, status 0, dV == 0 exactly without impulses, forward error of dX, dU, dV and the cost, the linearised defects and the pins
as test_direct_solve_gpu._check_step asserts them, and a second call bitwise the same.  At S in {17, 257, 513} padded leading
dimensions: NaN input padding never read, sentinel output padding never written, results bitwise those of the tight layout.
Batches of different systems equal their single solves bitwise; a singular trajectory in a batch is reported and leaves its
neighbours bitwise alone.  The free steps go through their host entry points on synth.direct_problem, with the reference fed the
device's own blocks.

Bars.  Two backward-stable float64 solves of one system land within a constant of each other, so the bar of a family is a
multiple of the error of the plain float64 host solve (the unrefined splu of qp_reference) against the refined reference, and
never looser than the 1e-9 the direct-method tests used so far.  The multiple is 100 for every family and variant: the device's
orthogonal reduction has up to ten levels of 34-row reflections where the host has one sparse LU (10 sqrt(34) ~ 58, rounded up).
Measured on an MI355X, largest over the sweep and the batches (relative 2-norm of dX, dU, dV, relative cost; p in units of half
the box width), with the refined reference's own error below 1e-11 everywhere:
  family / variant      device      host float64    bar = min(100 x host, 1e-9)
  orthogonal            1.1e-13     1.6e-14         1.6e-12
  scaled                3.7e-12     1.0e-12         1.0e-10
  permutation           1.2e-12     3.6e-14         3.6e-12
  free, free tf: step   3.7e-11     4.3e-11         1e-9 (100 x host is looser)
  free, free tf: p      1.1e-12     3.3e-14         3.3e-12
The optimality-only route of an ambiguous free case (none occurs: 520 cases, active bounds 224 / 208 / 204 times in p1, p2, p3)
checks the reduced gradient to what moving p by 1e-9 of the box changes it by.
The permutation family's arithmetic is exact only in the impulse update without impulses (dV == 0, asserted for every family):
the shared node's column of a pair always holds the F = -I entry, the control weight and a G / H entry, so the reflections have
irrational norms and every other output is rounded."""
import ctypes as C

import numpy as np
import pytest

import lowthrustopt_amd as lto

import direct_helpers as DH
import qp_reference as QR

pytestmark = pytest.mark.gpu

ISP, NSTEPS = 2000.0, 10
SIZES = [1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 21, 43, 85, 15, 16, 17, 31, 32, 33, 63, 64, 65, 254, 255, 256, 257, 511, 512, 513]
PADDED = (17, 257, 513)
BATCHES = [(17, 3), (257, 4), (513, 2)]
BATCH_MIX = [("scaled", QR.SCALED_G[0]), ("permutation", 1.0), ("scaled", QR.SCALED_G[2]), ("orthogonal", 1.0)]
FREE_S = [2, 3, 5, 9, 13, 16, 33, 255, 256, 257, 511, 513]
SENTINEL = -7.25e300
# BARS: family -> bar on the relative forward error of dX, dU, dV (2-norm) and the cost
BARS = {"orthogonal": 1.6e-12, "scaled": 1.0e-10, "permutation": 3.6e-12}
BAR_FREE, BAR_FREE_P = 1e-9, 3.3e-12          # the free steps' update and cost; p in units of half the box width


def _plan(ctx, ns, n, B):
    """DU = TU = 1: c2 = (DU/TU)^2 = 1 exactly (the permutation family's integers stay integers)."""
    return lto.DirectPlan(ctx, ns, n, B, NSTEPS, lto.MU, 1.0, 1.0, ISP)


def _status(plan, B):
    import torch
    torch.cuda.synchronize()
    out = (C.c_int * B)()
    cp = plan.ctx.lib.hipMemcpy                       # resolved through the library's own dependency on the HIP runtime
    cp.restype, cp.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    assert cp(out, plan.qp_status_ptr(), C.sizeof(out), 2) == 0
    return list(out)


def _soa(arrs, ld, fill=np.nan):
    """Per-trajectory [rows, m] arrays -> SoA [rows][ld], entry b * m + i; `fill` in the padding."""
    rows, m = arrs[0].shape
    A = np.full((rows, ld), fill)
    A[:, :len(arrs) * m] = np.stack(arrs, axis=1).reshape(rows, -1)
    return A


def _step(plan, systems, imp, pad=False):
    """One frozen step of the systems (qp_reference.Synthetic, one per trajectory).  Returns dX [ns, n, B], dU [3, n, B], dV [6, B],
    cost [B], status [B]."""
    import torch
    ns, _, S = systems[0].Jt.shape
    B, n = len(systems), S + 1
    ldj, ldd, ldx, ldu = (B * S + 5, B * S + 3, B * n + 7, B * n + 2) if pad else (B * S, B * S, B * n, B * n)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()     # noqa: E731
    Jac = dev(_soa([s.Jt.transpose(1, 0, 2).reshape(-1, S) for s in systems], ldj))      # row col * ns + row
    d = dev(_soa([s.d for s in systems], ldd))
    X = dev(_soa([s.X for s in systems], ldx))
    U = dev(_soa([s.U for s in systems], ldu))
    t = dev(np.stack([s.t for s in systems]))
    tg = dev(np.stack([np.r_[s.targets[0], s.targets[1], s.targets[2], s.targets[3], s.targets[4]] for s in systems]))
    dX = dev(_soa([np.full((ns, n), np.nan)] * B, ldx, SENTINEL))
    dU = dev(_soa([np.full((3, n), np.nan)] * B, ldu, SENTINEL))
    dV = torch.full((B, 6), float("nan"), dtype=torch.float64, device="cuda")
    cost = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
    plan.qp_step(Jac, ldj, d, ldd, X, ldx, U, ldu, t, B, tg, dX, dU, dV, cost, allowImpulsive=imp)
    status = _status(plan, B)
    dX, dU = dX.cpu().numpy(), dU.cpu().numpy()
    assert np.all(dX[:, B * n:] == SENTINEL) and np.all(dU[:, B * n:] == SENTINEL), "output padding written"
    return (dX[:, :B * n].reshape(ns, B, n).transpose(0, 2, 1), dU[:, :B * n].reshape(3, B, n).transpose(0, 2, 1),
            dV.cpu().numpy().T, cost.cpu().numpy(), status)


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[:4], b[:4])) and a[4] == b[4]


def _check_frozen(s, imp, dX, dU, dV, cost, bar, what):
    """Forward error against the refined reference and the residual checks of _check_step.  Returns (device error, host error)."""
    assert np.all(np.isfinite(dX)) and np.all(np.isfinite(dU)) and np.all(np.isfinite(dV)) and np.isfinite(cost), what
    ref, herr = s.sys.frozen(s.d, s.X, s.U, *s.targets)
    assert herr < QR.ERR_FLOOR, (what, "reference", herr)
    errs = [QR.rel(dX, ref.dX), QR.rel(dU, ref.dU), abs(cost - ref.cost) / abs(ref.cost)]
    if imp:
        errs.append(QR.rel(dV, ref.dV))
    else:
        assert np.all(dV == 0), what
    e = max(errs)
    print("\nqp-shapes %s: device %.2e host float64 %.2e (cond %.1e)" % (what, e, herr, s.cond))
    assert e <= bar, (what, errs)
    Jt, ns = s.Jt, s.X.shape[0]
    s0, sf, mass, dV1, dV2 = s.targets
    lin = np.einsum("rci,ci->ri", Jt[:, :ns], dX[:, :-1]) + np.einsum("rci,ci->ri", Jt[:, ns:2 * ns], dX[:, 1:]) + \
        np.einsum("rci,ci->ri", Jt[:, 2 * ns:2 * ns + 3], dU[:, :-1]) + np.einsum("rci,ci->ri", Jt[:, 2 * ns + 3:], dU[:, 1:]) + s.d
    scale = np.abs(s.d).max() + np.abs(Jt).max() * (np.abs(dX).max() + np.abs(dU).max())
    assert np.abs(lin).max() <= 1e-12 * scale, what
    e0 = s.X[:6, 0] + dX[:6, 0] + np.r_[0, 0, 0, dV1 + dV[:3]] - s0
    ef = s.X[:6, -1] + dX[:6, -1] + np.r_[0, 0, 0, dV2 + dV[3:]] - sf
    assert max(np.abs(e0).max(), np.abs(ef).max()) <= 1e-12 * max(1.0, np.abs(s.X[:6]).max()), what
    if ns == 7:
        assert abs(s.X[6, 0] + dX[6, 0] - mass) <= 1e-12 * max(1.0, abs(mass)), what
    return e, herr


def _systems(S, ns, imp):
    """The sweep's systems of one shape: every family, the scaled one at each of its three magnitudes in turn over the sizes."""
    k = SIZES.index(S) if S in SIZES else S
    out = []
    for f, family in enumerate(QR.FAMILIES):
        g = QR.SCALED_G[k % 3] if family == "scaled" else 1.0
        out.append((family, g, QR.synthetic(family, ns, S, 1000 * S + 10 * ns + 2 * imp + f, imp, g=g)))
    return out


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("imp", [False, True], ids=["pinned", "impulsive"])
@pytest.mark.parametrize("ns", [6, 7])
def test_frozen_shape_sweep(gpu_ctx, ns, imp, S):
    plan = _plan(gpu_ctx, ns, S + 1, 1)
    try:
        for family, g, s in _systems(S, ns, imp):
            what = "ns=%d imp=%d S=%d %s g=%g" % (ns, imp, S, family, g)
            out = _step(plan, [s], imp)
            assert out[4] == [0], what
            _check_frozen(s, imp, out[0][..., 0], out[1][..., 0], out[2][:, 0], out[3][0], BARS[family], what)
            assert _same(out, _step(plan, [s], imp)), what                       # a second call: bitwise the same
            if S in PADDED:
                assert _same(out, _step(plan, [s], imp, pad=True)), what
    finally:
        plan.close()


@pytest.mark.parametrize("S,B", BATCHES)
@pytest.mark.parametrize("imp", [False, True], ids=["pinned", "impulsive"])
@pytest.mark.parametrize("ns", [6, 7])
def test_frozen_batch_of_different_systems(gpu_ctx, ns, imp, S, B):
    """Families alternating, the scaled magnitudes mixed (2^-20 next to 2^10: the per-trajectory scale factors of qp_scale differ by
    60 binades within the batch): every trajectory equals its single solve bitwise and matches the reference."""
    systems = [QR.synthetic(f, ns, S, 77 + 13 * b + ns + imp, imp, g=g) for b, (f, g) in enumerate(BATCH_MIX[:B])]
    plan = _plan(gpu_ctx, ns, S + 1, B)
    try:
        out = _step(plan, systems, imp)
    finally:
        plan.close()
    assert out[4] == [0] * B
    single = _plan(gpu_ctx, ns, S + 1, 1)
    try:
        for b, s in enumerate(systems):
            one = _step(single, [s], imp)
            assert _same([o[..., b:b + 1] for o in out[:4]] + [out[4][b:b + 1]], one), b
            _check_frozen(s, imp, out[0][..., b], out[1][..., b], out[2][:, b], out[3][b], BARS[s.family], "batch S=%d b=%d %s" % (S, b, s.family))
    finally:
        single.close()


@pytest.mark.parametrize("ns", [6, 7])
def test_singular_trajectory_in_a_batch(gpu_ctx, ns):
    """B = 3, the middle trajectory's controls without effect (G = H = 0, impulses off: its pinned end states are unreachable):
    status [0, 1, 0], the middle outputs NaN, the outer two bitwise their single solves."""
    S = 17
    systems = [QR.synthetic("orthogonal", ns, S, 500 + b + ns, False) for b in range(3)]
    systems[1].Jt = systems[1].Jt.copy(order="F")
    systems[1].Jt[:, 2 * ns:, :] = 0.0
    plan = _plan(gpu_ctx, ns, S + 1, 3)
    try:
        out = _step(plan, systems, False)
    finally:
        plan.close()
    assert out[4] == [0, 1, 0]
    assert np.all(np.isnan(out[0][..., 1])) and np.all(np.isnan(out[1][..., 1])) and np.all(np.isnan(out[2][:, 1])) and np.isnan(out[3][1])
    single = _plan(gpu_ctx, ns, S + 1, 1)
    try:
        for b in (0, 2):
            one = _step(single, [systems[b]], False)
            assert _same([o[..., b:b + 1] for o in out[:4]] + [out[4][b:b + 1]], one), b
    finally:
        single.close()


# ---- the free steps, through their host entry points
def free_problems(variant, n, ns, seed):
    """The five beta (and tf bound) settings of test_direct_free_gpu._free_problems / test_direct_free_tf_gpu._tf_problems.  The
    absolute tf bounds of setting 3 (tf in [t0 + 1 day, 40 days]) hold only for grids of 20 to 40 days; where this grid's tf lies
    outside them they are moved around it: (1 day, tf - 1/2 day, tf + 10 days), lower bound inside the step as before."""
    if variant == "free":
        from test_direct_free_gpu import _free_problems
        X, U, T, tg, em, betas, host = _free_problems(n, ns, 5, seed)
        return X, U, T, tg, em, None, betas, [h + (None,) for h in host]
    from test_direct_free_tf_gpu import _tf_problems, DAY
    X, U, T, tg, em, tb, betas, host = _tf_problems(n, ns, 5, seed)
    for b in range(5):
        step, lo, hi = host[b][4]
        if not (lo <= T[-1, b] <= hi):
            bounds = (DAY, T[-1, b] - DAY / 2, T[-1, b] + 10 * DAY)
            tb[b] = lto.direct_tf_bounds(*bounds)
            host[b] = host[b][:4] + (bounds,)
    return X, U, T, tg, em, tb, betas, host


def free_reference(variant, Jt, dtf, d, X, U, t, imp, host):
    (s0, sf, g0, gf, c0, cf), mass, dV1, dV2, tfb = host[:5]
    beta = host[5]
    qs = QR.QpSystem(Jt, t, imp, (lto.DU / lto.TU) ** 2)
    return qs.free(d, X, U, s0, sf, mass, dV1, dV2, g0, gf, c0, cf, beta, dtf if variant == "free_tf" else None, tfb)


def _free_call(ctx, variant, X, U, T, tg, em, tb, betas, imp):
    if variant == "free":
        return lto.direct_qp_step_free(X, U, T, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tg, em, betas, allowImpulsive=imp, ctx=ctx)
    return lto.direct_qp_step_free_tf(X, U, T, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tg, em, betas, tb, allowImpulsive=imp, ctx=ctx)


_TALLY = {}          # (variant, S) -> (cases, optimality-only cases, active bounds per coordinate)


def _free_case(ctx, variant, S):
    if (variant, S) in _TALLY:
        return _TALLY[variant, S]
    n = S + 1
    cases = only = 0
    active = [0, 0, 0]
    for ns in (6, 7):
        X, U, T, tg, em, tb, betas, host = free_problems(variant, n, ns, n + ns)
        Jt, dtf, d, _ = lto.direct_jacobian_blocks(X, U, T, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, ctx=ctx)
        for imp in (False, True):
            dX, dU, dV, p, cost = _free_call(ctx, variant, X, U, T, tg, em, tb, betas, imp)
            for b in range(5):
                what = "%s S=%d ns=%d imp=%d b=%d" % (variant, S, ns, imp, b)
                ref = free_reference(variant, Jt[..., b], dtf[..., b], d[..., b], X[..., b], U[..., b], T[:, b], imp, host[b] + (betas[b],))
                pd = p[:, b]
                assert np.all(np.isfinite(pd)) and np.all(pd >= ref.lo) and np.all(pd <= ref.hi), what
                cases += 1
                half = np.maximum((ref.hi - ref.lo) / 2, 1e-300)
                print("\nqp-shapes %s: p %s ref %s on_bound %s ambiguous %d host err %.2e p_err %.2e" % (
                    what, pd, ref.p, ref.on_bound, ref.ambiguous, ref.err, ref.p_err.max()), end="")
                if ref.ambiguous:
                    only += 1
                    opt = ref.optimality(pd, BAR_FREE)
                    print(" optimality %.2e" % opt, end="")
                    assert opt <= 1.0, what
                    continue
                st = ref.step
                for j in range(len(pd)):
                    if ref.on_bound[j]:
                        assert pd[j] == ref.p[j], what                      # the bound value, bit for bit
                        active[j] += 1
                ep = float((np.abs(pd - ref.p) / half).max())
                errs = [DH.rel(dX[..., b], st.dX), DH.rel(dU[..., b], st.dU), abs(cost[b] - st.cost) / abs(st.cost)]
                if imp:
                    errs.append(DH.rel(dV[:, b], st.dV))
                else:
                    assert np.all(dV[:, b] == 0), what
                print(" device p %.2e step %.2e" % (ep, max(errs)), end="")
                assert ep <= BAR_FREE_P and max(errs) <= BAR_FREE, (what, ep, errs)
    assert only < cases, "no trajectory of this size compared directly"
    _TALLY[variant, S] = (cases, only, active)
    return _TALLY[variant, S]


def free_sizes():
    """n - 1 of the free sweep: FREE_S, and 1 where test_qp_reference_host found n = 2 solvable (it is: see N2_FINDING there)."""
    return [1] + FREE_S


@pytest.mark.parametrize("S", [1] + FREE_S)
@pytest.mark.parametrize("variant", ["free", "free_tf"])
def test_free_steps_shape_sweep(gpu_ctx, variant, S):
    _free_case(gpu_ctx, variant, S)


def test_free_sweep_caps(gpu_ctx):
    """Over the whole sweep: the optimality-only route is taken by at most one case in ten, and each of p1, p2, p3 is on a bound
    somewhere (sizes another test of this run has done are not done again)."""
    cases = only = 0
    active = np.zeros(3, dtype=int)
    for variant in ("free", "free_tf"):
        for S in free_sizes():
            c, o, a = _free_case(gpu_ctx, variant, S)
            cases, only, active = cases + c, only + o, active + a
    print("\nqp-shapes free sweep: %d cases, %d by the optimality conditions only, active bounds %s" % (cases, only, active))
    assert 10 * only <= cases and np.all(active > 0)


@pytest.mark.parametrize("S", [256, 512])
@pytest.mark.parametrize("variant", ["free", "free_tf"])
def test_free_steps_batch_equals_single(gpu_ctx, variant, S):
    """n in {257, 513}: each trajectory of the batch equals its single-trajectory call bitwise."""
    X, U, T, tg, em, tb, betas, host = free_problems(variant, S + 1, 7, S)
    out = _free_call(gpu_ctx, variant, X, U, T, tg, em, tb, betas, True)
    for b in range(5):
        one = _free_call(gpu_ctx, variant, X[..., b], U[..., b], T[:, b], tg[b], em[b], None if tb is None else tb[b], betas[b], True)
        for j in range(4):
            assert np.array_equal(out[j][..., b], one[j]), (b, j)
        assert out[4][b] == one[4], b
