"""The column step of the eight-wave sweep (LTO_KERNEL_PIPE8) at its seams.  pipe8's plain column waves advance the two steps of a
phase as one straight-line body (the column goes y -> z -> y), the alternating job keeps its column in LDS between the steps, an
odd step count ends with a phase of one step in place, and every 256th step the column is multiplied by 3^-256 where it stands.
None of this is reached by 64 steps, so here the sweeps are long enough to take the rescale (256 and 512 steps, and one step either
side) and short enough to end inside the first phase (1, 2, 3 steps).

Forced onto pipe8, the outputs equal LTO_KERNEL_PIPE32's bit for bit: pipe32 advances one step per phase in place with the same
stage code, so any product that landed in another accumulator, a stale register at a seam or a rescale that was skipped, doubled
or applied to the wrong half of the ping-pong shows as a different bit.  S = 17 is one full workgroup plus a ragged one (the
alternating job w4 / w5 and shadow lanes live), S = 13 leaves the alternating job a single live segment.

Against the per-lane kernel, whose column code (var_col14 / var_col12) is independent of the DPP form: the tolerances
test_pipe8_edges.py uses for that pairing, 1e-12 on the defect and 1e-11 relative on Phi.  Before the change to the column step
the sweep stayed inside them at 256 and 257 steps on every shape below (largest figures: defect 6.7e-16 [14-dim, p = 1,
S = 13, 257 steps], Phi 4.4e-15 relative [12-dim, p = 2, S = 13, 257 steps]; profiles/r09_pipe_col_step.txt), so they are not
widened."""
import numpy as np
import pytest

import lowthrustopt_amd as lto
from lowthrustopt_amd import synth
from lowthrustopt_amd.constants import MU, DU, TU

pytestmark = pytest.mark.gpu

CLASSES = [(14, 1.0), (14, 0.0), (12, 1.0), (12, 2.0)]
SIZES = [17, 13]
KERNELS = {"pipe8": "pipeline8", "pipe32": "pipeline32", "per_lane": "per-lane"}


def problem(ndim, S, seed=5):
    n = S + 1
    XC, T = synth.indirect_problem(n, seed=seed)
    if ndim == 14:
        X = np.zeros((14, n, 1), order="F")
        X[:6] = XC[:6]; X[6] = 1000.0; X[7:13] = XC[6:]; X[13] = 0.2
        return X, T, 2000.0
    return XC, T, 1000.0


def run(ctx, kernel, ndim, p, steps, S):
    import torch
    X, T, slot = problem(ndim, S)
    n = S + 1
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


def bitwise(ctx, ndim, p, steps, S):
    import torch
    P8, d8 = run(ctx, "pipe8", ndim, p, steps, S)
    P32, d32 = run(ctx, "pipe32", ndim, p, steps, S)
    assert bool(torch.isfinite(P8).all()) and bool(torch.isfinite(d8).all()), S
    assert not bool((P8 == 7.0).any()) and not bool((d8 == 7.0).any()), S       # every entry written
    assert torch.equal(P8, P32) and torch.equal(d8, d32), S


@pytest.mark.parametrize("ndim,p", CLASSES)
@pytest.mark.parametrize("steps", [255, 256, 257, 512, 513])
def test_pipe8_equals_pipe32_bitwise_across_the_rescale(gpu_ctx, ndim, p, steps):
    for S in SIZES:
        bitwise(gpu_ctx, ndim, p, steps, S)


@pytest.mark.parametrize("ndim,p", CLASSES)
@pytest.mark.parametrize("steps", [1, 2, 3])
def test_pipe8_equals_pipe32_bitwise_when_the_sweep_ends_in_its_first_phases(gpu_ctx, ndim, p, steps):
    bitwise(gpu_ctx, ndim, p, steps, 17)


@pytest.mark.parametrize("ndim,p", CLASSES)
@pytest.mark.parametrize("steps", [256, 257])
def test_pipe8_agrees_with_the_per_lane_kernel_across_the_rescale(gpu_ctx, ndim, p, steps):
    for S in SIZES:
        P8, d8 = (x.cpu().numpy() for x in run(gpu_ctx, "pipe8", ndim, p, steps, S))
        P1, d1 = (x.cpu().numpy() for x in run(gpu_ctx, "per_lane", ndim, p, steps, S))
        assert np.all(np.isfinite(P8)) and np.all(np.isfinite(d8)), S
        e_d = np.abs(d8 - d1).max() / max(1.0, np.abs(d1).max())
        e_p = np.abs(P8 - P1).max() / np.abs(P1).max()
        print("col_step ndim=%d p=%g S=%d steps=%d: defect %.3e (bound 1e-12), Phi rel %.3e (bound 1e-11)" % (ndim, p, S, steps, e_d, e_p))
        assert e_d < 1e-12, S
        assert e_p < 1e-11, S
