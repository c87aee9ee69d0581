"""Phi through the LDS transpose of the three pipeline kernels (pipe_common.hpp, pipe_store_phi): LTO_KERNEL_PIPE8, _PIPE32 and
_PIPE48, 12- and 14-dim.  After the last step barrier the column lanes put their values into a tile in the dead coefficient ring,
together with a table of the workgroup's segment targets (-1 = store nothing), and every resident wave stores whole rows.  Checked
here: the values (against the per-lane kernel, at the tolerances of test_pipe8_edges.py for that pair), that a launch of a
mixed-class batch leaves the other classes' segments alone, that nothing is written past column S - 1 of a ragged batch, and the
unit lambda_m column of the always-thrust-limited laws, NaN spans included.

The lane order: a fixed-step plan has no step counts to balance by and lto_indirect_plan_rebalance refuses it, so no pipeline sweep
can be given a balanced order through the library's interface; the first test states that and compares the plan with itself after
the refused call.  The table of targets that serves an order is the one every other test here goes through."""
import numpy as np
import pytest

import lowthrustopt_amd as lto
from lowthrustopt_amd import synth
from lowthrustopt_amd.constants import MU, DU, TU

pytestmark = pytest.mark.gpu

NAMES = {"pipe8": "pipeline8", "pipe32": "pipeline32", "pipe48": "pipeline48", "per_lane": "per-lane"}
FORMS = [(k, nd) for k in ("pipe8", "pipe32", "pipe48") for nd in (12, 14)]
SENTINEL = 7.0


def pick(plan, kernel):
    plan.set_kernel({"pipe8": plan.KERNEL_PIPE8, "pipe32": plan.KERNEL_PIPE32, "pipe48": plan.KERNEL_PIPE48, "per_lane": plan.KERNEL_PER_LANE}[kernel])


def problem(ndim, n, nb=1, seed=5):
    XC, T = synth.indirect_problem(n, n_batch=nb, seed=seed)
    if ndim == 14:
        X = np.zeros((14, n, nb), order="F")
        X[:6] = XC[:6]; X[6] = 1000.0; X[7:13] = XC[6:]; X[13] = 0.2
        return X, T, 2000.0
    return XC, T, 1000.0


def sweep(ctx, kernel, ndim, prms, X, T, steps=5, pad=0, before=None):
    """One STM sweep of a batch [ndim][n][nb] with Phi and the defect prefilled with the sentinel and `pad` spare columns."""
    import torch
    n, nb = X.shape[1], X.shape[2]
    S = (n - 1) * nb
    plan = lto.IndirectPlan(ctx, n, nb, prms if nb > 1 else prms[0], lto.integrator(lto.RK4, steps=steps), ndim=ndim)
    pick(plan, kernel)
    if before:
        before(plan)
    Xd = torch.from_numpy(synth.to_soa_nodes(X)).cuda()
    td = torch.from_numpy(np.ascontiguousarray(T.T.reshape(-1))).cuda()
    Phi = torch.full((ndim * ndim, S + pad), SENTINEL, dtype=torch.float64, device="cuda")
    d = torch.full((ndim, S + pad), SENTINEL, dtype=torch.float64, device="cuda")
    plan.jacobian(Xd, n * nb, td, nb, Phi, S + pad, d, S + pad)
    torch.cuda.synchronize()
    assert plan.last_kernel() == NAMES[kernel]
    plan.close()
    return Phi.cpu().numpy(), d.cpu().numpy()


def close_to_per_lane(P, d, P1, d1):
    """the bounds test_pipe8_edges.py sets for a pipeline kernel against the per-lane kernel"""
    print("max |dPhi| / max |Phi| = %.3e, max |ddefect| = %.3e" % (np.abs(P - P1).max() / np.abs(P1).max(), np.abs(d - d1).max()))
    assert np.abs(d - d1).max() < 1e-12 * max(1.0, np.abs(d1).max())
    assert np.abs(P - P1).max() < 1e-11 * np.abs(P1).max()


@pytest.mark.parametrize("kernel,ndim", FORMS)
def test_phi_with_and_without_a_lane_order_equals_the_per_lane_kernel(gpu_ctx, kernel, ndim):
    S = 4 * 48 + 29                                  # several workgroups of every form and a ragged last one
    X, T, slot = problem(ndim, S + 1)
    prms = [lto.make_params(MU, DU, TU, 0.05, slot, 1.0, 1.0, 1.0)]

    def rebalance(plan):                             # fixed-step plan: refused, the plan keeps its natural order
        with pytest.raises(lto.LtoError):
            plan.rebalance()

    P, d = sweep(gpu_ctx, kernel, ndim, prms, X, T)
    Pr, dr = sweep(gpu_ctx, kernel, ndim, prms, X, T, before=rebalance)
    P1, d1 = sweep(gpu_ctx, "per_lane", ndim, prms, X, T)
    assert np.all(np.isfinite(P)) and not np.any(P == SENTINEL)
    assert np.array_equal(P, Pr) and np.array_equal(d, dr)
    close_to_per_lane(P, d, P1, d1)


@pytest.mark.parametrize("kernel,ndim", FORMS)
def test_mixed_class_batch_every_launch_stores_its_own_segments_only(gpu_ctx, kernel, ndim):
    """One launch per control-law class, each over the whole batch: a launch that wrote a segment of another class would overwrite
    that class's result (or the sentinel, where its own launch comes later) with values of the wrong law.  Every trajectory is also
    swept alone, where no other launch exists, and must come out the same bit for bit."""
    laws = ((0.0, 0.05, 1.0), (1.0, 0.05, 0.3), (2.0, 10.0, 1.0), (1.5, 0.05, 1.0)) if ndim == 12 else ((0.0, 0.05, 1.0), (1.0, 0.05, 0.3), (1.0, 0.05, 1.0), (0.0, 0.05, 0.5))
    n, nb = 60, len(laws)                            # 59 segments per trajectory: class boundaries inside workgroups of every form
    X, T, slot = problem(ndim, n, nb, seed=17)
    prms = [lto.make_params(MU, DU, TU, thr, slot, 1.0, p, rho) for p, thr, rho in laws]
    P, d = sweep(gpu_ctx, kernel, ndim, prms, X, T, steps=7)
    assert not np.any(P == SENTINEL) and not np.any(d == SENTINEL) and np.all(np.isfinite(P))
    P1, d1 = sweep(gpu_ctx, "per_lane", ndim, prms, X, T, steps=7)
    close_to_per_lane(P, d, P1, d1)
    for b in range(nb):
        Pb, db = sweep(gpu_ctx, kernel, ndim, [prms[b]], np.asfortranarray(X[:, :, b:b + 1]), np.asfortranarray(T[:, b:b + 1]), steps=7)
        assert np.array_equal(P[:, b * (n - 1):(b + 1) * (n - 1)], Pb), b
        assert np.array_equal(d[:, b * (n - 1):(b + 1) * (n - 1)], db), b


@pytest.mark.parametrize("kernel,ndim", FORMS)
@pytest.mark.parametrize("S", [1, 17, 101, 4 * 48 + 47])
def test_ragged_batch_writes_nothing_past_its_last_segment(gpu_ctx, kernel, ndim, S):
    X, T, slot = problem(ndim, S + 1, seed=3)
    prms = [lto.make_params(MU, DU, TU, 0.05, slot, 1.0, 1.0, 1.0)]
    pad = 53
    P, d = sweep(gpu_ctx, kernel, ndim, prms, X, T, pad=pad)
    P0, d0 = sweep(gpu_ctx, kernel, ndim, prms, X, T)
    assert np.all(P[:, S:] == SENTINEL) and np.all(d[:, S:] == SENTINEL)
    assert not np.any(P[:, :S] == SENTINEL) and np.all(np.isfinite(P[:, :S]))
    assert np.array_equal(P[:, :S], P0) and np.array_equal(d[:, :S], d0)


@pytest.mark.parametrize("kernel", ["pipe8", "pipe32", "pipe48"])
@pytest.mark.parametrize("p", [0.0, 1.0])
def test_unit_lambda_m_column_and_nan_spans(gpu_ctx, kernel, p):
    """14-dim, always-thrust-limited laws: d x(t1) / d lambda_m(t0) is the unit vector.  pipe8 and pipe32 do not integrate that column
    (its lane writes the unit vector into the tile), pipe48 integrates it like the others, so there it is the unit vector up to the
    rounding of 3^k 3^-k.  A segment whose span is NaN has NaN in every entry of Phi, that column included."""
    S = 70
    X, T, slot = problem(14, S + 1, seed=9)
    T = T.copy()
    bad = 37
    T[bad, 0] = np.nan                               # the spans of segments bad - 1 and bad
    prms = [lto.make_params(MU, DU, TU, 0.05, slot, 1.0, p, 1.0)]
    P, d = sweep(gpu_ctx, kernel, 14, prms, X, T, steps=6)
    P = P.reshape(14, 14, S)                         # [column][row][segment]
    nan_seg = np.zeros(S, dtype=bool)
    nan_seg[[bad - 1, bad]] = True
    assert np.all(np.isnan(P[:, :, nan_seg]))
    assert np.all(np.isfinite(P[:, :, ~nan_seg]))
    unit = np.zeros((14, 1))
    unit[13] = 1.0
    col = P[13][:, ~nan_seg]
    if kernel == "pipe48":
        assert np.abs(col - unit).max() < 4 * np.finfo(float).eps
    else:
        assert np.array_equal(col, np.broadcast_to(unit, col.shape))
    P1, d1 = sweep(gpu_ctx, "per_lane", 14, prms, X, T, steps=6)
    P1 = P1.reshape(14, 14, S)
    close_to_per_lane(P[:, :, ~nan_seg], d[:, ~nan_seg], P1[:, :, ~nan_seg], d1[:, ~nan_seg])
