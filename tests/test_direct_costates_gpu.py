"""Costates of the direct transcription from the multipliers of the device QP step (k_qp_costates, lto_direct_costates*, DESIGN
4.16) against the multiplier part of qp_reference's refined KKT solution, and the hand-over to the indirect method they are for.

Shapes, read against the kernel (one lane per node, 256-wide blocks): S = 1 has no interior node (kkt_res == 0 exactly), 2 the first
one, 3 and 5 odd counts, 17 more than one level of the reduction, 64 / 65 either side of a wavefront (n = 65 / 66 nodes), 257 past
a block.  The three families of qp_reference.synthetic, ns in {6, 7}, impulses off and on, each through qp_step + costates on a
plan.  At S in {17, 257} padded leading dimensions: NaN input padding never read, sentinel output padding never written, results
bitwise those of the tight layout.  A second call, a batch of different systems and the neighbours of a singular trajectory are
bitwise their single solves; qp_step's own outputs do not move when costates runs before or after it.

Bars.  The rule and the reason of test_direct_qp_shapes_gpu.py: the device's orthogonal reduction and the host's sparse LU are two
backward-stable float64 solves of one system, so the bar of a family is 100 x the error of the plain float64 host solve of the same
quantity (multipliers, Lambda) against the refined reference, largest over the family's cases of this sweep; kkt_res is held to the
Lambda bar.  Measured on an MI355X (relative 2-norm, largest over the sweep; printed by test_shape_sweep):
  family        device mult   host mult   device Lambda   host Lambda   largest kkt_res   bar = 100 x host (mult / Lambda)
  orthogonal    1.1e-13       1.3e-14     1.1e-13         1.3e-14       5.2e-15           1.3e-12 / 1.3e-12
  scaled        9.2e-12       3.2e-13     9.3e-12         3.5e-13       4.6e-13           3.2e-11 / 3.5e-11
  permutation   1.3e-13       2.8e-14     1.3e-13         2.8e-14       5.6e-14           2.8e-12 / 2.8e-12
(the largest of every column is at S = 257; the refined reference's own error is below 1e-11 everywhere).

Covector property and hand-over, on the demo transfer solved by lto_direct_solve (n = 30 and n = 59 over the same 20 days):
e(n) = |lambda_v + 2 c u| / |2 c u| over the nodes, with lambda = c^2 Lambda and c = costate_scale(DU, TU); measured e(30) =
2.06e-2, e(59) = 7.04e-3 (ratio 2.9).  The seed's initial indirect defect (p = 2, 10 N, max-abs): 1.14e-4, against 5.48e-3 at
-lambda, 4.83e-3 at c Lambda and 5.05e-1 at 0.1 randn.  Hand-over: 2 full Newton iterations to 5.6e-16, where the existing route takes
10 adjoints-only + 1 full to 6.2e-11; three starts of multiStart_direct: 2 iterations each."""
import ctypes as C

import numpy as np
import pytest

import lowthrustopt_amd as lto
from lowthrustopt_amd import drivers, synth, _lib

import costates_reference as CR
import direct_helpers as DH
import qp_reference as QR
from test_direct_qp_shapes_gpu import _plan, _status, _soa, SENTINEL, NSTEPS, ISP

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 3, 5, 17, 64, 65, 257]
PADDED = (17, 257)
MIX = [("scaled", QR.SCALED_G[0]), ("permutation", 1.0), ("scaled", QR.SCALED_G[2])]


def _bars(family):
    """(bar of the multipliers, bar of Lambda and kkt_res, host errors): 100 x the plain float64 host solve's error."""
    em, el = CR.host_errors(SIZES, family)
    assert em < QR.ERR_FLOOR and el < QR.ERR_FLOOR, (family, em, el)
    return 100 * em, 100 * el, em, el


def _run(plan, systems, imp, pad=False, order="after", want_mult=True):
    """One frozen step of the systems and the costates from it.  order: "after" (qp_step, costates), "twice" (qp_step, costates,
    qp_step again into fresh outputs, costates again: the second round is returned), "none" (qp_step only).  Returns (Lambda [ns, n,
    B], mult [ns, S, B], kkt_res [B], status [B], (dX, dU, dV, cost) as numpy)."""
    import torch
    ns, _, S = systems[0].Jt.shape
    B, n = len(systems), S + 1
    ldj, ldd, ldx, ldu, ldl, ldm = (B * S + 5, B * S + 3, B * n + 7, B * n + 2, B * n + 9, B * S + 4) if pad else \
        (B * S, B * S, B * n, B * n, B * n, B * S)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()     # noqa: E731
    Jac = dev(_soa([s.Jt.transpose(1, 0, 2).reshape(-1, S) for s in systems], ldj))
    d = dev(_soa([s.d for s in systems], ldd))
    X = dev(_soa([s.X for s in systems], ldx))
    U = dev(_soa([s.U for s in systems], ldu))
    t = dev(np.stack([s.t for s in systems]))
    tg = dev(np.stack([np.r_[s.targets[0], s.targets[1], s.targets[2], s.targets[3], s.targets[4]] for s in systems]))

    def step():
        dX = dev(_soa([np.full((ns, n), np.nan)] * B, ldx, SENTINEL))
        dU = dev(_soa([np.full((3, n), np.nan)] * B, ldu, SENTINEL))
        dV = torch.full((B, 6), float("nan"), dtype=torch.float64, device="cuda")
        cost = torch.full((B,), float("nan"), dtype=torch.float64, device="cuda")
        plan.qp_step(Jac, ldj, d, ldd, X, ldx, U, ldu, t, B, tg, dX, dU, dV, cost, allowImpulsive=imp)
        return dX, dU, dV, cost

    def costates():
        Lam = dev(_soa([np.full((ns, n), 3.5)] * B, ldl, SENTINEL))
        mult = dev(_soa([np.full((ns, S), 3.5)] * B, ldm, SENTINEL)) if want_mult else None
        res = torch.full((B,), -1.0, dtype=torch.float64, device="cuda")
        plan.costates(Jac, ldj, Lam, ldl, res, mult, ldm if want_mult else 0)
        return Lam, mult, res
    out = step()
    cs = None
    if order != "none":
        cs = costates()
    if order == "twice":
        out = step()
        cs = costates()
    status = _status(plan, B)
    qp = tuple(o.cpu().numpy() for o in out)
    if cs is None:
        return None, None, None, status, qp
    Lam, res = cs[0].cpu().numpy(), cs[2].cpu().numpy()
    assert np.all(Lam[:, B * n:] == SENTINEL), "Lambda padding written"
    mult = None
    if want_mult:
        mult = cs[1].cpu().numpy()
        assert np.all(mult[:, B * S:] == SENTINEL), "mult padding written"
        mult = mult[:, :B * S].reshape(ns, B, S).transpose(0, 2, 1)
    return Lam[:, :B * n].reshape(ns, B, n).transpose(0, 2, 1), mult, res, status, qp


def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a[:3], b[:3])) and a[3] == b[3]


_WORST = {}


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("imp", [False, True], ids=["pinned", "impulsive"])
@pytest.mark.parametrize("ns", [6, 7])
def test_shape_sweep(gpu_ctx, ns, imp, S):
    plan = _plan(gpu_ctx, ns, S + 1, 1)
    try:
        for family in QR.FAMILIES:
            s, ref = CR.case(family, ns, S, imp)
            bar_m, bar_l, host_m, host_l = _bars(family)
            what = "ns=%d imp=%d S=%d %s" % (ns, imp, S, family)
            out = _run(plan, [s], imp)
            Lam, mult, res = out[0][..., 0], out[1][..., 0], out[2][0]
            assert out[3] == [0], what
            assert np.all(np.isfinite(Lam)) and np.all(np.isfinite(mult)) and np.isfinite(res), what
            em, el = QR.rel(mult, ref.mult), QR.rel(Lam, ref.Lambda)
            w = _WORST.setdefault(family, [0.0, 0.0, 0.0])
            w[:] = [max(w[0], em), max(w[1], el), max(w[2], res)]
            print("\ncostates %s: device mult %.2e (host %.2e, this case %.2e) Lambda %.2e (host %.2e, this case %.2e) kkt_res %.2e; "
                  "family so far %.2e %.2e %.2e" % (what, em, host_m, ref.err_mult, el, host_l, ref.err_lambda, res, *w))
            assert em <= bar_m and el <= bar_l, (what, em, bar_m, el, bar_l)
            assert res <= bar_l, (what, res, bar_l)
            if S == 1:
                assert res == 0.0, what
            assert _same(out, _run(plan, [s], imp)), what                        # a second call: bitwise the same
            assert np.array_equal(out[0], _run(plan, [s], imp, want_mult=False)[0]), what
            if S in PADDED:
                assert _same(out, _run(plan, [s], imp, pad=True)), what
    finally:
        plan.close()


@pytest.mark.parametrize("imp", [False, True], ids=["pinned", "impulsive"])
@pytest.mark.parametrize("ns", [6, 7])
def test_batch_of_different_systems(gpu_ctx, ns, imp):
    """B = 3 at S = 17, the scaled magnitudes 2^-20 and 2^10 around a permutation system: every trajectory equals its single solve
    bitwise and meets its family's bar."""
    S = 17
    cases = [CR.case(f, ns, S, imp, seed=177 + 13 * b + ns + imp, g=g) for b, (f, g) in enumerate(MIX)]
    systems = [c[0] for c in cases]
    plan = _plan(gpu_ctx, ns, S + 1, 3)
    try:
        out = _run(plan, systems, imp)
        padded = _run(plan, systems, imp, pad=True)
    finally:
        plan.close()
    assert out[3] == [0, 0, 0] and _same(out, padded)
    single = _plan(gpu_ctx, ns, S + 1, 1)
    try:
        for b, (s, ref) in enumerate(cases):
            one = _run(single, [s], imp)
            assert _same([out[0][..., b:b + 1], out[1][..., b:b + 1], out[2][b:b + 1], out[3][b:b + 1]], one), b
            bar_m, bar_l = 100 * ref.err_mult, 100 * ref.err_lambda
            em, el = QR.rel(out[1][..., b], ref.mult), QR.rel(out[0][..., b], ref.Lambda)
            print("\ncostates batch ns=%d imp=%d b=%d %s: mult %.2e (host %.2e) Lambda %.2e (host %.2e) kkt_res %.2e" % (
                ns, imp, b, s.family, em, ref.err_mult, el, ref.err_lambda, out[2][b]))
            assert ref.err_mult < QR.ERR_FLOOR and em <= bar_m and el <= bar_l and out[2][b] <= bar_l, (b, em, bar_m, el, bar_l, out[2][b])
    finally:
        single.close()


@pytest.mark.parametrize("ns", [6, 7])
def test_singular_trajectory_in_a_batch(gpu_ctx, ns):
    """B = 3, the middle trajectory's controls without effect (test_direct_qp_shapes_gpu): status [0, 1, 0], its three outputs NaN,
    the outer two bitwise their single solves."""
    S = 17
    systems = [QR.synthetic("orthogonal", ns, S, 500 + b + ns, False) for b in range(3)]
    systems[1].Jt = systems[1].Jt.copy(order="F")
    systems[1].Jt[:, 2 * ns:, :] = 0.0
    plan = _plan(gpu_ctx, ns, S + 1, 3)
    try:
        out = _run(plan, systems, False)
    finally:
        plan.close()
    assert out[3] == [0, 1, 0]
    assert np.all(np.isnan(out[0][..., 1])) and np.all(np.isnan(out[1][..., 1])) and np.isnan(out[2][1])
    single = _plan(gpu_ctx, ns, S + 1, 1)
    try:
        for b in (0, 2):
            one = _run(single, [systems[b]], False)
            assert np.all(np.isfinite(one[0])) and np.all(np.isfinite(one[1]))
            assert _same([out[0][..., b:b + 1], out[1][..., b:b + 1], out[2][b:b + 1], out[3][b:b + 1]], one), b
    finally:
        single.close()


@pytest.mark.parametrize("ns", [6, 7])
def test_qp_step_outputs_do_not_move(gpu_ctx, ns):
    """dX, dU, dV, cost of qp_step are bitwise the same without a costates call, with one after it, and with one before it (on the
    plan's previous step)."""
    S, B = 65, 2
    systems = [CR.case(f, ns, S, True)[0] for f in ("orthogonal", "scaled")]
    plan = _plan(gpu_ctx, ns, S + 1, B)
    try:
        plain = _run(plan, systems, True, order="none")[4]
        after = _run(plan, systems, True, order="after")[4]
        before = _run(plan, systems, True, order="twice")[4]
    finally:
        plan.close()
    for a, b in ((plain, after), (plain, before)):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert np.all(np.isfinite(plain[3]))


def test_dev_entry_argument_checks(gpu_ctx):
    import torch
    S, B, ns = 5, 2, 6
    n = S + 1
    plan = _plan(gpu_ctx, ns, n, B)
    try:
        z = lambda *sh: torch.zeros(sh, dtype=torch.float64, device="cuda")     # noqa: E731
        Jac, Lam, mult, res = z(ns * (2 * ns + 6), B * S), z(ns, B * n), z(ns, B * S), z(B)

        def code(*a, **k):
            with pytest.raises(lto.LtoError) as ei:
                plan.costates(*a, **k)
            return ei.value.code
        assert code(Jac, B * S, Lam, B * n, res) == _lib.LTO_EINVAL            # no step on this plan yet
        systems = [CR.case("orthogonal", ns, S, False)[0]] * B
        _run(plan, systems, False, order="none")
        assert code(None, B * S, Lam, B * n, res) == _lib.LTO_ENULL
        assert code(Jac, B * S, None, B * n, res) == _lib.LTO_ENULL
        assert code(Jac, B * S, Lam, B * n, None) == _lib.LTO_ENULL
        assert code(Jac, B * S - 1, Lam, B * n, res) == _lib.LTO_EINVAL
        assert code(Jac, B * S, Lam, B * n - 1, res) == _lib.LTO_EINVAL
        assert code(Jac, B * S, Lam, B * n, res, mult, B * S - 1) == _lib.LTO_EINVAL
        plan.costates(Jac, B * S, Lam, B * n, res, mult, B * S)                 # and the same arguments in order pass
        torch.cuda.synchronize()
    finally:
        plan.close()


def _targets(X, B, ns):
    """End targets a little off the problem's end states, an impulse on each end."""
    rng = np.random.default_rng(11)
    return [lto.direct_targets(X[:6, 0, b] + 1e-3 * rng.standard_normal(6), X[:6, -1, b] + 1e-3 * rng.standard_normal(6),
                               (X[6, 0, b] if ns == 7 else 1000.0), 1e-3 * rng.standard_normal(3), 1e-3 * rng.standard_normal(3))
            for b in range(B)]


@pytest.mark.parametrize("ns", [6, 7])
def test_host_entry_equals_the_plan_route(gpu_ctx, ns):
    """lto_direct_costates_batch on synth.direct_problem (n = 6, B = 3, distinct grids) equals jacobian + qp_step + costates on a
    plan bitwise; XC = (X; c^2 Lambda) bitwise; ns = 7 with XC is LTO_EUNSUPPORTED and still returns the multipliers without it."""
    import torch
    n, B = 6, 3
    X, U, T = synth.direct_problem(n, B, nstate=ns)
    T = np.asfortranarray(T * (1.0 + 0.05 * np.arange(B))[None, :])              # distinct grids
    assert X.shape == (ns, n, B) and len({tuple(T[:, b]) for b in range(B)}) == B
    tgs = _targets(X, B, ns)
    if ns == 7:
        with pytest.raises(lto.LtoError) as ei:
            lto.direct_costates(X, U, T, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tgs, True, with_XC=True, ctx=gpu_ctx)
        assert ei.value.code == _lib.LTO_EUNSUPPORTED
    Lam, mult, XC, res, status = lto.direct_costates(X, U, T, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tgs, True, ctx=gpu_ctx)
    assert list(status) == [0] * B and np.all(np.isfinite(Lam)) and np.all(np.isfinite(mult)) and np.all(np.isfinite(res))
    assert (XC is None) == (ns == 7)
    if ns == 6:
        c = lto.costate_scale(lto.DU, lto.TU)
        assert np.array_equal(XC[:6], X) and np.array_equal(XC[6:], (c * c) * Lam)
    one = lto.direct_costates(X[..., 1], U[..., 1], T[:, 1], NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tgs[1], True, ctx=gpu_ctx)
    assert np.array_equal(one[0], Lam[..., 1]) and np.array_equal(one[1], mult[..., 1]) and one[3] == res[1] and one[4] == 0
    # the plan route on the same operands
    S = n - 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()     # noqa: E731
    z = lambda *sh: torch.zeros(sh, dtype=torch.float64, device="cuda")  # noqa: E731
    Xd, Ud = dev(X.transpose(0, 2, 1).reshape(ns, B * n)), dev(U.transpose(0, 2, 1).reshape(3, B * n))
    td = dev(T.T)
    tg = dev(np.stack([np.frombuffer(bytes(t), dtype=np.float64) for t in tgs]))
    Jac, d = z(ns * (2 * ns + 6), B * S), z(ns, B * S)
    dX, dU, dV, cost = z(ns, B * n), z(3, B * n), z(B, 6), z(B)
    Ld, md, rd = z(ns, B * n), z(ns, B * S), z(B)
    plan = lto.DirectPlan(gpu_ctx, ns, n, B, NSTEPS, lto.MU, lto.DU, lto.TU, ISP)
    try:
        plan.jacobian(Xd, B * n, Ud, B * n, td, B, Jac, B * S, defect=d, ldd=B * S)
        plan.qp_step(Jac, B * S, d, B * S, Xd, B * n, Ud, B * n, td, B, tg, dX, dU, dV, cost, allowImpulsive=True)
        plan.costates(Jac, B * S, Ld, B * n, rd, md, B * S)
        torch.cuda.synchronize()
    finally:
        plan.close()
    assert np.array_equal(Ld.cpu().numpy().reshape(ns, B, n).transpose(0, 2, 1), Lam)
    assert np.array_equal(md.cpu().numpy().reshape(ns, B, S).transpose(0, 2, 1), mult)
    assert np.array_equal(rd.cpu().numpy(), res)


def test_host_entry_argument_checks(gpu_ctx):
    n, B = 6, 2
    X, U, T = synth.direct_problem(n, B)
    prm = _lib.LtoDirectParams(lto.MU, lto.DU, lto.TU, ISP)
    tg = (_lib.LtoDirectTargets * B)(*_targets(X, B, 6))
    Lam, res, st = np.zeros((6, n, B), order="F"), np.zeros(B), np.zeros(B, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)     # noqa: E731
    fn = gpu_ctx.fn("direct_costates_batch")
    call = lambda **k: fn(gpu_ctx.handle, k.get("ns", 6), n, B, k.get("X", p(X)), p(U), p(T), k.get("ntg", B), NSTEPS, C.byref(prm),  # noqa: E731
                          C.cast(tg, C.c_void_p), k.get("ntgt", B), 0, k.get("Lam", p(Lam)), None, None, k.get("res", p(res)),
                          k.get("st", p(st)))
    assert call() == _lib.LTO_OK
    assert call(X=None) == _lib.LTO_ENULL and call(Lam=None) == _lib.LTO_ENULL and call(res=None) == _lib.LTO_ENULL
    assert call(st=None) == _lib.LTO_ENULL
    assert call(ns=5) == _lib.LTO_EINVAL and call(ntg=3) == _lib.LTO_EINVAL and call(ntgt=3) == _lib.LTO_EINVAL


# ---- the demo transfer: covector property and hand-over
_DEMO = {}


def _demo_solution(ctx, n):
    """The demo transfer on n nodes over its 20 days, solved by lto_direct_solve, and its costates: computed once per run."""
    if n not in _DEMO:
        X, U, t, tau1, tau2, a, b, c, d = DH.demo().demo_problem(n_nodes=n)
        s0, sf = drivers.interpEndStates(tau1, tau2, a, b, c, d)
        tg = lto.direct_targets(s0, sf, 1000.0, np.zeros(3), np.zeros(3))
        Xs, Us, dV, ts, defect, status, iters, _ = lto.direct_solve(X, U, t, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tg, maxIter=100, ctx=ctx)
        assert status == 0 and np.abs(defect).max() <= 1e-6, (n, status)
        Lam, mult, XC, res, st = lto.direct_costates(Xs, Us, ts, NSTEPS, lto.MU, lto.DU, lto.TU, ISP, tg, ctx=ctx)
        assert st == 0 and np.all(np.isfinite(XC))
        _DEMO[n] = {"X": Xs, "U": Us, "t": ts, "tg": tg, "Lambda": Lam, "XC": XC, "kkt_res": res}
    return _DEMO[n]


def _e(sol):
    c = lto.costate_scale(lto.DU, lto.TU)
    lam_v = (c * c) * sol["Lambda"][3:6]
    return float(np.linalg.norm(lam_v + 2 * c * sol["U"]) / np.linalg.norm(2 * c * sol["U"]))


def test_covector_property_converges(gpu_ctx):
    """lambda_v = c^2 Lambda_v approaches the p = 2 control law's -2 a = -2 c u as the grid is refined: the transcription is second
    order (a quarter per doubling), e(59) <= e(30) / 2 leaves a factor of two for the coarse grid."""
    e30, e59 = _e(_demo_solution(gpu_ctx, 30)), _e(_demo_solution(gpu_ctx, 59))
    print("\ncostates covector: e(30) = %.3e, e(59) = %.3e, ratio %.2f; kkt_res %.2e %.2e" % (
        e30, e59, e30 / e59, _DEMO[30]["kkt_res"], _DEMO[59]["kkt_res"]))
    assert e59 <= e30 / 2


def test_seed_beats_wrong_signs_and_scales(gpu_ctx):
    """The initial indirect defect (p = 2, thrustLimit 10 N, max-abs, lto_indirect_defect) at the seed is strictly smaller than at
    -lambda, at c Lambda (one power of c short) and at the demo's 0.1 randn (seed 0)."""
    sol = _demo_solution(gpu_ctx, 30)
    c = lto.costate_scale(lto.DU, lto.TU)
    prm = lto.make_params(lto.MU, lto.DU, lto.TU, 10.0, 1000.0, 1.0, 2.0, 1.0)
    X, Lam = sol["X"], sol["Lambda"]
    seeds = {"seed": sol["XC"], "minus": np.vstack([X, -(c * c) * Lam]), "c short": np.vstack([X, c * Lam]),
             "randn": np.vstack([X, 0.1 * np.random.default_rng(0).standard_normal((6, 30))])}
    d = {k: float(np.abs(lto.indirect_defectCalc(np.asfortranarray(v), sol["t"], prm, ctx=gpu_ctx)[0]).max()) for k, v in seeds.items()}
    print("\ncostates seeds, initial indirect defect: %s" % ", ".join("%s %.3e" % kv for kv in d.items()))
    assert all(d["seed"] < d[k] for k in ("minus", "c short", "randn")), d


def test_hand_over_converges_without_the_adjoints_only_phase(gpu_ctx):
    """drivers.direct_to_indirect on the demo solution: status 0 at the driver's 1e-10, in no more iterations than the existing
    route (0.1 randn costates, ten adjoints-only iterations, then the full ones), which runs here for the comparison."""
    sol = _demo_solution(gpu_ctx, 30)
    r = drivers.direct_to_indirect(sol["X"], sol["U"], sol["t"], NSTEPS, 1000.0, ISP, lto.MU, lto.DU, lto.TU, 10.0, 50, ctx=gpu_ctx)
    assert np.array_equal(r["seed"][..., 0], sol["XC"])
    prm = lto.make_params(lto.MU, lto.DU, lto.TU, 10.0, 1000.0, 1.0, 2.0, 1.0)
    XC0 = np.asfortranarray(np.vstack([sol["X"], 0.1 * np.random.default_rng(0).standard_normal((6, 30))]))
    XC1, _, st1, it1, _ = lto.indirect_solve(XC0, sol["t"], prm, None, True, 10, ctx=gpu_ctx)
    _, d2, st2, it2, _ = lto.indirect_solve(XC1, sol["t"], prm, None, False, 50, ctx=gpu_ctx)
    old = min(it1, 10) + it2
    print("\ncostates hand-over: %d iterations (status %d, max defect %.2e); existing route %d + %d = %d (status %d, max defect %.2e)" % (
        r["iterations"][0], r["status"][0], r["max_defect"][0], min(it1, 10), it2, old, st2, np.abs(d2).max()))
    assert r["status"][0] == 0 and r["max_defect"][0] <= 1e-10
    assert r["iterations"][0] <= old


def test_multi_start_then_indirect(gpu_ctx):
    """Three starts on n = 30: one indirect status per converged start."""
    a, b, c, d = DH.tables()
    tof = 10.0 * lto.day / lto.TU
    m = drivers.multiStart_direct([0.70, 0.75, 0.80], tof, tof, 30, NSTEPS, 1000.0, ISP, a, b, c, d, lto.MU, lto.DU, lto.TU,
                                  maxIter=100, ctx=gpu_ctx, then_indirect=True)
    ok = np.flatnonzero(m["status"] == 0)
    assert np.array_equal(m["indirect_starts"], ok)
    print("\ncostates multi-start: direct status %s, indirect %s" % (m["status"], None if m["indirect"] is None else (
        m["indirect"]["status"], m["indirect"]["iterations"], m["indirect"]["max_defect"])))
    assert ok.size >= 1
    ind = m["indirect"]
    assert ind["status"].shape == (ok.size,) and ind["XC"].shape == (12, 30, ok.size) and ind["iterations"].shape == (ok.size,)
    assert np.all(np.isin(ind["status"], (0, 1, 2, 3)))
    plain = drivers.multiStart_direct([0.75], tof, tof, 30, NSTEPS, 1000.0, ISP, a, b, c, d, lto.MU, lto.DU, lto.TU, maxIter=100, ctx=gpu_ctx)
    assert "indirect" not in plain
