"""The placement table of the eight-wave contract sweep (kernels_indirect_pipe8.hip, P8Place): which wave of the workgroup runs the
base role, the coefficient role, the three plain column jobs and the two halves of the alternating one, which wave exits, and in
which order the seven resident waves share the row stores of Phi.  A wrong map shows as a segment nobody advances, a job advanced
twice, a row group of Phi stored twice or not at all -- never as a small error -- so the check is bit for bit.

Reference: the twelve-wave form (kernels_indirect_pipe32.hip), which runs the same three roles -- the same arithmetic in the same
order, so the same bits -- with one barrier per step, no flags, every wave resident, and its own fixed wave numbers.  It is built
for the classes whose RK4 stages pair: 12-dim p = 0, p = 1, p = 2 and general p, 14-dim p = 0 and p = 1.  The remaining class of
pipe8, 14-dim with p > 1 (lambda_m on the base wave's chain), is compared with the per-lane kernel at the bounds of
test_pipe_level.py: 1e-12 on the defect, 1e-11 relative on Phi.

Shapes: S = 1 (one lane row), 3, 13 (a partly filled workgroup), 16 (exactly one), 17 (one and a shadow workgroup), 33 (two and a
shadow, and a second workgroup of pipe32); steps = 1 (no full phase), 2 (one), 3 and 5 (odd: the tail step), 64 (the contract's).

The lane order: a fixed-step plan has no step counts to balance by and lto_indirect_plan_rebalance refuses it
(test_pipe_phi_store.py), so the ordered plan at S = 17 is the plan after the refused call -- it must keep its natural order and
give the same bits."""
import numpy as np
import pytest

import lowthrustopt_amd as lto
from lowthrustopt_amd import synth
from lowthrustopt_amd.constants import MU, DU, TU

pytestmark = pytest.mark.gpu

NAMES = {"pipe8": "pipeline8", "pipe32": "pipeline32", "per_lane": "per-lane"}
PAIRING = [(12, 0.0), (12, 1.0), (12, 2.0), (12, 1.5), (14, 0.0), (14, 1.0)]      # every class pipe32 is built for
SIZES = (1, 3, 13, 16, 17, 33)
STEPS = (1, 2, 3, 5, 64)
SENTINEL = 7.0
BOUND_DEFECT, BOUND_PHI = 1e-12, 1e-11


def thrust(p):
    return 10.0 if p > 1.0 else 0.05


def problem(ndim, n, nb=1, seed=5):
    XC, T = synth.indirect_problem(n, n_batch=nb, seed=seed)
    if ndim == 14:
        X = np.zeros((14, n, nb), order="F")
        X[:6] = XC[:6]; X[6] = 1000.0; X[7:13] = XC[6:]; X[13] = 0.2
        return X, T, 2000.0
    return XC, T, 1000.0


def params(p, slot):
    return lto.make_params(MU, DU, TU, thrust(p), slot, 1.0, p, 1.0)


def sweep(ctx, kernel, ndim, prms, X, T, steps, before=None):
    """One STM sweep of a batch [ndim][n][nb], Phi and the defect prefilled with the sentinel."""
    import torch
    n, nb = X.shape[1], X.shape[2]
    S = (n - 1) * nb
    plan = lto.IndirectPlan(ctx, n, nb, prms if nb > 1 else prms[0], lto.integrator(lto.RK4, steps=steps), ndim=ndim)
    plan.set_kernel({"pipe8": plan.KERNEL_PIPE8, "pipe32": plan.KERNEL_PIPE32, "per_lane": plan.KERNEL_PER_LANE}[kernel])
    if before:
        before(plan)
    Xd = torch.from_numpy(synth.to_soa_nodes(X)).cuda()
    td = torch.from_numpy(np.ascontiguousarray(T.T.reshape(-1))).cuda()
    Phi = torch.full((ndim * ndim, S), SENTINEL, dtype=torch.float64, device="cuda")
    d = torch.full((ndim, S), SENTINEL, dtype=torch.float64, device="cuda")
    plan.jacobian(Xd, n * nb, td, nb, Phi, S, d, S)
    torch.cuda.synchronize()
    assert plan.last_kernel() == NAMES[kernel]
    plan.close()
    return Phi.cpu().numpy(), d.cpu().numpy()


def written(P, d):
    return np.all(np.isfinite(P)) and np.all(np.isfinite(d)) and not np.any(P == SENTINEL) and not np.any(d == SENTINEL)


@pytest.mark.parametrize("ndim,p", PAIRING)
def test_pipe8_equals_pipe32_bit_for_bit(gpu_ctx, ndim, p):
    for S in SIZES:
        X, T, slot = problem(ndim, S + 1)
        prms = [params(p, slot)]
        for steps in STEPS:
            P8, d8 = sweep(gpu_ctx, "pipe8", ndim, prms, X, T, steps)
            P32, d32 = sweep(gpu_ctx, "pipe32", ndim, prms, X, T, steps)
            assert written(P8, d8), (S, steps)
            assert np.array_equal(P8, P32), (S, steps)
            assert np.array_equal(d8, d32), (S, steps)


@pytest.mark.parametrize("ndim", [12, 14])
def test_plan_after_a_refused_rebalance_keeps_its_order_and_its_bits(gpu_ctx, ndim):
    S, steps = 17, 5
    X, T, slot = problem(ndim, S + 1)
    prms = [params(1.0, slot)]

    def rebalance(plan):
        with pytest.raises(lto.LtoError):
            plan.rebalance()

    P, d = sweep(gpu_ctx, "pipe8", ndim, prms, X, T, steps)
    Pr, dr = sweep(gpu_ctx, "pipe8", ndim, prms, X, T, steps, before=rebalance)
    P32, d32 = sweep(gpu_ctx, "pipe32", ndim, prms, X, T, steps)
    assert written(Pr, dr)
    assert np.array_equal(P, Pr) and np.array_equal(d, dr)
    assert np.array_equal(Pr, P32) and np.array_equal(dr, d32)


@pytest.mark.parametrize("ndim", [12, 14])
def test_mixed_class_batch_equals_pipe32_and_every_trajectory_alone(gpu_ctx, ndim):
    """One launch per class over the whole batch, the class boundaries inside workgroups (17 segments per trajectory)."""
    laws = (0.0, 1.0, 2.0, 1.5) if ndim == 12 else (0.0, 1.0, 1.0, 0.0)
    n, nb, steps = 18, len(laws), 5
    X, T, slot = problem(ndim, n, nb, seed=17)
    prms = [params(p, slot) for p in laws]
    P, d = sweep(gpu_ctx, "pipe8", ndim, prms, X, T, steps)
    P32, d32 = sweep(gpu_ctx, "pipe32", ndim, prms, X, T, steps)
    assert written(P, d)
    assert np.array_equal(P, P32) and np.array_equal(d, d32)
    for b in range(nb):
        Pb, db = sweep(gpu_ctx, "pipe8", ndim, [prms[b]], np.asfortranarray(X[:, :, b:b + 1]), np.asfortranarray(T[:, b:b + 1]), steps)
        assert np.array_equal(P[:, b * (n - 1):(b + 1) * (n - 1)], Pb), b
        assert np.array_equal(d[:, b * (n - 1):(b + 1) * (n - 1)], db), b


def test_lambda_m_on_the_chain_agrees_with_the_per_lane_kernel(gpu_ctx):
    """14-dim, p = 2: the one-stage-at-a-time base role and the record with mm / Ll; pipe32 is not built for it."""
    worst_d = worst_p = 0.0
    for S in SIZES:
        X, T, slot = problem(14, S + 1)
        prms = [params(2.0, slot)]
        for steps in STEPS:
            P, d = sweep(gpu_ctx, "pipe8", 14, prms, X, T, steps)
            P1, d1 = sweep(gpu_ctx, "per_lane", 14, prms, X, T, steps)
            assert written(P, d), (S, steps)
            e_d = np.abs(d - d1).max() / max(1.0, np.abs(d1).max())
            e_p = np.abs(P - P1).max() / np.abs(P1).max()
            worst_d, worst_p = max(worst_d, e_d), max(worst_p, e_p)
            assert e_d < BOUND_DEFECT and e_p < BOUND_PHI, (S, steps, e_d, e_p)
    print("pipe8_placement 14-dim p=2 against the per-lane kernel: defect %.3e (bound %g), Phi %.3e (bound %g)"
          % (worst_d, BOUND_DEFECT, worst_p, BOUND_PHI))
