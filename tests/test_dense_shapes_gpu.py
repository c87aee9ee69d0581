"""The dense-output kernel (k_indirect_dense, indirect_kernel.hpp) across its shapes, against the CPU oracle (tests/dense_reference.py).

Single trajectories go through lto.densify, batches through lto_indirect_dense_dev (IndirectPlan.dense) on torch device tensors.
Shapes, n nodes -> n_desired samples (dense_reference.SHAPES): 2 -> 2, 2 -> 3, 2 -> 65, 3 -> 2; 13 -> 5 and 66 -> 7 (most
segments own no sample); 13 -> 13 on a LinRange grid (every sample is a node); 13 -> 25; 64 -> 65, 65 -> 64, 66 -> 129, 130 -> 257
(S = 63, 64, 65, 129 lanes in workgroups of 64).  Each shape with two of the (p, thrust, time direction) triples of p in {0, 1, 2,
1.5}, 0.05 and 10 N, +1 and -1 -- the 24 sets cover all 16 -- and with DOP853, RK4 x 8 and RK4 x 64.  Batches: 23 nodes, B = 3 and
5 trajectories of classes p = (1, 2, 0, 1.5, 1) (every class_filter launch runs), one time grid and B, sample counts (30, 7, 45, 23,
64) through one global first[], trajectory 1 with no sample in its first segment.

Checked at every sample j of every trajectory, i its segment:
  from the node   against the oracle's DOP853 flow of XC[:, i] over td[j] - t[i]: 1e-11 (DOP853), 1e-10 (RK4 x 64) relative to
                  max(1, |ref|), the bars of test_densify_vs_oracle.  RK4 x 8 shows its own truncation there and is not compared.
  hop by hop      against the oracle's flow, by the lane's own method and step count, of the device's own sample j-1 over
                  td[j] - td[j-1] (of the node for a segment's first sample): the same bars, 1e-10 for RK4 x 8.
  td[j] == t[i]   the sample is XC[:, i] bit for bit.
  Y               is pre-filled with a sentinel and has ldy > count: every owned column is written (it meets its reference), no
                  other changes.  final_state[c * B + b] is the flow of trajectory b's last segment; without it Y is the same.
  batches         equal their B single-trajectory calls bit for bit.

Largest differences measured on an MI355X over the sweep (device against reference, bar beside it):
                        from the node           hop by hop
  singles  DOP853       3.1e-14  (1e-11)        2.9e-15  (1e-11)
           RK4 x 64     1.4e-13  (1e-10)        3.9e-15  (1e-10)
           RK4 x 8      6.0e-10  (not compared) 2.3e-15  (1e-10)
  batches  DOP853       1.1e-15  (1e-11)        1.0e-16  (1e-11)
           RK4 x 64     4.1e-15  (1e-10)        3.8e-15  (1e-10)
           RK4 x 8      2.3e-12  (not compared) 1.2e-15  (1e-10)
The from-the-node figures are the reference's own (the oracle chained against the oracle from the node gives the same 3.1e-14 and
1.4e-13 on the CPU, test_dense_reference_host.py); every bitwise check held."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_reference as D  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e300
MNAMES = ["dop853", "rk4x8", "rk4x64"]


def _dev_dense(ctx, XC, T, prm_l, first, td, mname, pad, want_final=True):
    """lto_indirect_dense_dev on XC [12 x n x B], T [n x n_tgrids]: (Y [12 x (count + pad)], final [12 x B] or None), both
    pre-filled with the sentinel."""
    import torch
    method, steps = D.METHODS[mname]
    n, B = XC.shape[1], XC.shape[2]
    plan = lto.IndirectPlan(ctx, n, B, [lto.make_params(*q) for q in prm_l], lto.integrator(method, steps=steps))
    Xd = torch.from_numpy(synth.to_soa_nodes(XC)).cuda()
    tg = torch.from_numpy(np.ascontiguousarray(T.T.reshape(-1))).cuda()
    ts = torch.from_numpy(np.ascontiguousarray(td, dtype=np.float64)).cuda()
    fi = torch.from_numpy(np.ascontiguousarray(first, dtype=np.int32)).cuda()
    ldy = int(td.size) + pad
    Y = torch.full((12, ldy), SENTINEL, dtype=torch.float64, device="cuda")
    F = torch.full((12, B), SENTINEL, dtype=torch.float64, device="cuda") if want_final else None
    plan.dense(Xd, n * B, tg, T.shape[1], fi, ts, Y, ldy, F)
    torch.cuda.synchronize()
    plan.close()
    return Y.cpu().numpy(), (F.cpu().numpy() if want_final else None)


def _owners(first, base=0):
    """Segment of every owned column."""
    return np.repeat(np.arange(len(first) - 1), np.diff(first)), range(first[0] - base, first[-1] - base)


@pytest.mark.parametrize("mname", MNAMES)
@pytest.mark.parametrize("case", D.CASES, ids=[c.name for c in D.CASES])
def test_single_trajectory_shapes(gpu_ctx, oracle, case, mname):
    method, steps = D.METHODS[mname]
    tol = D.TOL[mname]
    XC, t, prm_l = D.case_problem(case)
    m = case.n_desired
    td_want, first = D.case_samples(case, t)
    XD, td = lto.densify(XC, t, lto.make_params(*prm_l), m, lto.integrator(method, steps=steps), ctx=gpu_ctx)
    assert XD.shape == (12, m) and np.array_equal(td, td_want)
    assert np.all(np.isfinite(XD))
    node_ref, hop_ref = D.dense_expected(oracle, XC, t, prm_l, td, first, method, steps, Y=XD)
    seg, cols = _owners(first)
    on_node = [j for j in cols if td[j] == t[seg[j]]]
    for j in on_node:
        assert np.array_equal(XD[:, j], XC[:, seg[j]]), j                     # bit for bit
    assert 0 in on_node and (not case.lin or len(on_node) == m - 1)
    en, eh = D.worst_errors(XD, node_ref, hop_ref, cols)
    fn, fh = D.final_expected(oracle, XC, t, prm_l, td, first, method, steps, Y=XD)
    en, eh = max(en, D.rel(XD[:, -1], fn)), max(eh, D.rel(XD[:, -1], fh))
    print("%s %s: S = %d, %d of %d segments empty, from the node %.2e, hop by hop %.2e (bar %.0e)" % (
        case.name, mname, case.n - 1, int(np.count_nonzero(np.diff(first) == 0)), case.n - 1, en, eh, tol))
    assert eh <= tol
    if mname in D.FROM_NODE:
        assert en <= tol
    # the device route on the same data: padded Y, the sentinel outside the owned columns, final_state given and not
    T = np.asfortranarray(t[:, None])
    for want_final in (True, False):
        Y, F = _dev_dense(gpu_ctx, XC[:, :, None], T, [prm_l], first, td, mname, pad=3, want_final=want_final)
        assert np.array_equal(Y[:, :m - 1], XD[:, :m - 1])
        assert np.all(Y[:, m - 1:] == SENTINEL)                                # the last sample is final_state's; the padding
        if want_final:
            assert np.array_equal(F[:, 0], XD[:, -1])


@pytest.mark.parametrize("mname", MNAMES)
@pytest.mark.parametrize("B,n_tgrids", [(3, 1), (3, 3), (5, 1), (5, 5)])
def test_mixed_class_batches(gpu_ctx, oracle, B, n_tgrids, mname):
    method, steps = D.METHODS[mname]
    tol = D.TOL[mname]
    XC, T, prm_l, tds, first, off = D.batch_problem(B, n_tgrids)
    n, S = D.BATCH_N, D.BATCH_N - 1
    assert first.size == B * S + 1 and first[S] == first[S + 1] == off[1]     # trajectory 1: no sample in its first segment
    assert len({q[6] for q in prm_l}) == (3 if B == 3 else 4)                 # the classes present
    td_all = np.concatenate(tds)
    Y, F = _dev_dense(gpu_ctx, XC, T, prm_l, first, td_all, mname, pad=5)
    Y0, _ = _dev_dense(gpu_ctx, XC, T, prm_l, first, td_all, mname, pad=5, want_final=False)
    assert np.array_equal(Y0, Y)
    assert np.all(Y[:, off[-1]:] == SENTINEL)
    assert np.all(np.isfinite(Y[:, :off[-1]])) and np.all(np.isfinite(F))
    en = eh = 0.0
    for b in range(B):
        t = np.array(T[:, b if n_tgrids > 1 else 0])
        f = first[b * S:(b + 1) * S + 1]
        Yb = Y[:, off[b]:off[b + 1]]
        node_ref, hop_ref = D.dense_expected(oracle, XC[:, :, b], t, prm_l[b], tds[b], f, method, steps, Y=Yb, base=off[b])
        seg, cols = _owners(f, off[b])
        assert len(cols) == tds[b].size
        for j in cols:
            if tds[b][j] == t[seg[j]]:
                assert np.array_equal(Yb[:, j], XC[:, seg[j], b]), (b, j)
        e1, e2 = D.worst_errors(Yb, node_ref, hop_ref, cols)
        fn, fh = D.final_expected(oracle, XC[:, :, b], t, prm_l[b], tds[b], f, method, steps, Y=Yb, base=off[b])
        en, eh = max(en, e1, D.rel(F[:, b], fn)), max(eh, e2, D.rel(F[:, b], fh))
        if b == 0:
            assert tds[0][-1] == t[-1] and np.array_equal(F[:, 0], Yb[:, -1])  # the last segment stepped onto t_n already
        else:
            assert tds[b][-1] < t[-1]
        # the same trajectory alone
        Y1, F1 = _dev_dense(gpu_ctx, XC[:, :, b:b + 1], np.asfortranarray(t[:, None]), [prm_l[b]], f - off[b], tds[b], mname, pad=2)
        assert np.array_equal(Y1[:, :tds[b].size], Yb), b
        assert np.all(Y1[:, tds[b].size:] == SENTINEL)
        assert np.array_equal(F1[:, 0], F[:, b]), b
    print("B = %d, %d grid(s), %s: S = %d, from the node %.2e, hop by hop %.2e (bar %.0e)" % (B, n_tgrids, mname, B * S, en, eh, tol))
    assert eh <= tol
    if mname in D.FROM_NODE:
        assert en <= tol
