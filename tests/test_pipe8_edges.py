"""The eight-wave contract sweep (LTO_KERNEL_PIPE8) at the edges of its phase loop: the base wave loads the end node of its
defect during the drain phase, before the last barrier.  Forced onto pipe8, the outputs equal LTO_KERNEL_PIPE32's (the same roles
under another synchronisation) bit for bit for every control-law class pipe32 is built for, at step counts below, around and at the
pipeline depth, odd and even, and at batch sizes around one full round of workgroups, ragged ones included; the 14-dim unclamped
p > 1 class (base role one stage at a time, no pipe32 form) agrees with the per-lane kernel within rounding; and pipe8 agrees with
the CPU oracle at the suite's tolerances."""
import numpy as np
import pytest

import lowthrustopt_amd as lto
from lowthrustopt_amd import synth
from lowthrustopt_amd.constants import MU, DU, TU

pytestmark = pytest.mark.gpu

STEPS = [1, 2, 3, 5, 63, 64]
SIZES = [17, 4095, 4096, 4097]
KERNELS = {"pipe8": "pipeline8", "pipe32": "pipeline32", "per_lane": "per-lane"}


def problem(ndim, S, seed=5):
    n = S + 1
    XC, T = synth.indirect_problem(n, seed=seed)
    if ndim == 14:
        X = np.zeros((14, n, 1), order="F")
        X[:6] = XC[:6]; X[6] = 1000.0; X[7:13] = XC[6:]; X[13] = 0.2
        return X, T, 2000.0
    return XC, T, 1000.0


def run(ctx, kernel, ndim, p, steps, X, T, slot):
    import torch
    n = X.shape[1]
    S = n - 1
    prm = lto.make_params(MU, DU, TU, 10.0 if p > 1.0 else 0.05, slot, 1.0, p, 1.0)
    plan = lto.IndirectPlan(ctx, n, 1, prm, lto.integrator(lto.RK4, steps=steps), ndim=ndim)
    plan.set_kernel({"pipe8": plan.KERNEL_PIPE8, "pipe32": plan.KERNEL_PIPE32, "per_lane": plan.KERNEL_PER_LANE}[kernel])
    Xd = torch.from_numpy(synth.to_soa_nodes(X)).cuda()
    td = torch.from_numpy(np.ascontiguousarray(T[:, 0])).cuda()
    Phi = torch.full((ndim * ndim, S), 7.0, dtype=torch.float64, device="cuda")
    d = torch.full((ndim, S), 7.0, dtype=torch.float64, device="cuda")
    plan.jacobian(Xd, n, td, 1, Phi, S, d, S)
    torch.cuda.synchronize()
    assert plan.last_kernel() == KERNELS[kernel]
    plan.close()
    return Phi, d


@pytest.mark.parametrize("ndim,p", [(12, 0.0), (12, 1.0), (12, 2.0), (12, 1.5), (14, 0.0), (14, 1.0)])
@pytest.mark.parametrize("steps", STEPS)
def test_pipe8_equals_pipe32_bitwise(gpu_ctx, ndim, p, steps):
    import torch
    for S in SIZES:
        X, T, slot = problem(ndim, S)
        P8, d8 = run(gpu_ctx, "pipe8", ndim, p, steps, X, T, slot)
        P32, d32 = run(gpu_ctx, "pipe32", ndim, p, steps, X, T, slot)
        assert bool(torch.isfinite(P8).all()) and bool(torch.isfinite(d8).all()), S
        assert torch.equal(P8, P32) and torch.equal(d8, d32), S


@pytest.mark.parametrize("steps", STEPS)
def test_pipe8_unpaired_base_role_agrees_with_the_per_lane_kernel(gpu_ctx, steps):
    for S in SIZES:
        X, T, slot = problem(14, S)
        P8, d8 = (x.cpu().numpy() for x in run(gpu_ctx, "pipe8", 14, 2.0, steps, X, T, slot))
        P1, d1 = (x.cpu().numpy() for x in run(gpu_ctx, "per_lane", 14, 2.0, steps, X, T, slot))
        assert np.all(np.isfinite(P8)) and np.all(np.isfinite(d8)), S
        assert np.abs(d8 - d1).max() < 1e-12 * max(1.0, np.abs(d1).max()), S
        assert np.abs(P8 - P1).max() < 1e-11 * np.abs(P1).max(), S


@pytest.mark.parametrize("ndim,p", [(12, 0.0), (12, 1.0), (12, 2.0), (12, 1.5), (14, 0.0), (14, 1.0), (14, 2.0)])
@pytest.mark.parametrize("steps", [1, 5, 64])
def test_pipe8_vs_oracle(gpu_ctx, oracle, ndim, p, steps):
    S = 29
    X, T, slot = problem(ndim, S, seed=2)
    thr = 10.0 if p > 1.0 else 0.05
    Phi, d = run(gpu_ctx, "pipe8", ndim, p, steps, X, T, slot)
    Phi = Phi.cpu().numpy().reshape(ndim, ndim, S).transpose(1, 0, 2)     # [column][row] -> Phi[row, column, segment]
    d = d.cpu().numpy()
    Xh, t = np.asfortranarray(X[:, :, 0]), np.ascontiguousarray(T[:, 0])
    prm = [MU, DU, TU, thr, slot, 1.0, p, 1.0]
    if ndim == 14:
        Phi_o, d_o, rc = oracle.indirect14(Xh, t, prm, oracle.RK4, steps)
    else:
        Phi_o, d_o, rc = oracle.indirect_jacobian(Xh, t, prm, oracle.RK4, steps)
    assert rc == 0
    assert np.linalg.norm(d - d_o) / np.linalg.norm(d_o + Xh[:, 1:]) < 1e-10
    assert np.abs(Phi - Phi_o).max() < 1e-10 * np.abs(Phi_o).max()
