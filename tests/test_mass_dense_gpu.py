"""Dense output of the 14-row variable-mass system on the device (k_indirect_dense<14>, lto_indirect_dense_mass_dev,
lto_indirect_densify_mass) against the CPU oracle (tests/mass_dense_reference.py).

Singles go through lto.densify_mass and, on the same data, through IndirectPlan.dense_mass with a padded ldx / ldy and a
sentinel-filled Y; the batch through IndirectPlan.dense_mass alone.  Shapes n -> n_desired (mass_dense_reference.DENSE_CASES):
2 -> 2, 2 -> 65, 3 -> 2 (an empty segment), 13 -> 5 (most segments empty), 13 -> 13 on a LinRange grid (every sample a node),
66 -> 129 (S = 65 lanes: a second workgroup), each with DOP853 and RK4 x 64, 2 -> 65 also with RK4 x 8; the six parameter sets once
each.  Bars, per row relative to max(1, max |reference row|): DOP853 1e-11 from the node and hop by hop, RK4 1e-10 hop by hop (against
the oracle's RK4 of the same step count from the device's own previous sample); the mass row besides to max(10 e_m, 64 eps m0) =
1.42e-11 kg absolute (e_m = 6.8e-13 kg, the reference against itself, test_mass_dense_host.py).

Measured on an MI355X (largest over the sweep): DOP853 1.7e-14 from the node, 2.5e-14 hop by hop; RK4 x 64 3.5e-14 and RK4 x 8
8.3e-16 hop by hop; batch 2.1e-14 / 3.9e-15 (DOP853), 7.4e-15 (RK4 x 64).  Mass row: e_m = 6.8e-13 kg on the CPU; the device's largest
difference 6.8e-13 kg from the node and 2.3e-13 kg hop by hop with DOP853, 7.3e-12 kg hop by hop with RK4 x 64 (bar 1.42e-11 kg).
Isp = 1e30 against the 12-row densify 1.5e-14, row 6 == m0.  Every test prints its figures before it asserts (MEASURED lines)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mass_dense_reference as M  # noqa: E402
import dense_reference as D  # noqa: E402
import addtime_reference as A  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import synth  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = -7.25e300
PAD_X, PAD_Y = 5, 3
SINGLES = [(c, m) for c in M.DENSE_CASES for m in c.methods]


def _integ(mname):
    method, steps = M.METHODS[mname]
    return lto.integrator(method, steps=steps)


def _dev_dense(ctx, XC, T, prm_l, first, td, integ, want_final=True, ndim=14, mass=True):
    """IndirectPlan.dense_mass (mass = False: .dense) on XC [rows x n x B], T [n x n_tgrids], X with ldx = n B + PAD_X, Y with ldy =
    count + PAD_Y: (Y, final [rows x B] or None), both pre-filled with the sentinel."""
    import torch
    n, B = XC.shape[1], XC.shape[2]
    rows = XC.shape[0]
    plan = lto.IndirectPlan(ctx, n, B, [lto.make_params(*q) for q in prm_l], integ, ndim=ndim)
    try:
        ldx = n * B + PAD_X
        Xh = np.full((rows, ldx), np.nan)
        Xh[:, :n * B] = synth.to_soa_nodes(XC)
        Xd = torch.from_numpy(Xh).cuda()
        tg = torch.from_numpy(np.ascontiguousarray(T.T.reshape(-1))).cuda()
        ts = torch.from_numpy(np.ascontiguousarray(td, dtype=np.float64)).cuda()
        fi = torch.from_numpy(np.ascontiguousarray(first, dtype=np.int32)).cuda()
        ldy = int(td.size) + PAD_Y
        Y = torch.full((rows, ldy), SENTINEL, dtype=torch.float64, device="cuda")
        F = torch.full((rows, B), SENTINEL, dtype=torch.float64, device="cuda") if want_final else None
        (plan.dense_mass if mass else plan.dense)(Xd, ldx, tg, T.shape[1], fi, ts, Y, ldy, F)
        torch.cuda.synchronize()
        return Y.cpu().numpy(), (F.cpu().numpy() if want_final else None)
    finally:
        plan.close()


def _check(label, mname, Y, node_ref, hop_ref, e_m):
    """The bars of the module docstring on Y against its two references (columns the references hold)."""
    tol = M.TOL[mname]
    scale = M.row_scale(node_ref)
    en, eh = M.rel_rows(Y, node_ref, scale), M.rel_rows(Y, hop_ref, scale)
    mn, mh = float(np.nanmax(np.abs(Y[6] - node_ref[6]))), float(np.nanmax(np.abs(Y[6] - hop_ref[6])))
    bar_m = M.mass_bar(e_m)
    print("MEASURED %s %s: from the node %.3e, hop by hop %.3e (bar %.0e); mass row from the node %.3e kg, hop by hop %.3e kg (bar %.3e kg)"
          % (label, mname, en, eh, tol, mn, mh, bar_m))
    assert np.all(np.isfinite(Y[:, np.isfinite(node_ref[0])]))
    assert eh <= tol
    assert mh <= bar_m
    if mname == "dop853":
        assert en <= tol
        assert mn <= bar_m
    return en, eh, mn, mh


@pytest.mark.parametrize("c,mname", SINGLES, ids=["%s-%s" % (M.case_id(c), m) for c, m in SINGLES])
def test_single_trajectory_shapes(gpu_ctx, oracle, c, mname):
    X, t, prm = M.fixture(c.n, c.k, c.lin)
    method, steps = M.METHODS[mname]
    _, e_m = M.self_errors()
    m = c.n_desired
    XD, td = lto.densify_mass(X, t, lto.make_params(*prm), m, _integ(mname), ctx=gpu_ctx)
    assert XD.shape == (14, m) and np.array_equal(td, A.linrange(t[0], t[-1], m))
    td_ref, node_ref, hop_ref = M.densify_expected(oracle, X, t, prm, m, method, steps, Y=XD)
    first = D.segment_ranges(t, td, False)
    assert np.array_equal(td_ref, td) and not np.any(np.isnan(node_ref))
    seg = np.repeat(np.arange(c.n - 1), np.diff(first))
    on_node = [j for j in range(m - 1) if td[j] == t[seg[j]]]
    for j in on_node:
        assert np.array_equal(XD[:, j], X[:, seg[j]]), j                      # bit for bit
    assert 0 in on_node and (not c.lin or len(on_node) == m - 1)
    assert np.all(np.diff(XD[6]) <= 0.0)                                       # the mass never rises along the trajectory
    _check(M.case_id(c), mname, XD, node_ref, hop_ref, e_m)
    # the device route on the same data: padded X and Y, the sentinel outside the owned columns, final_state given and not
    T = np.asfortranarray(np.array(t)[:, None])
    for want_final in (True, False):
        Y, F = _dev_dense(gpu_ctx, np.asarray(X)[:, :, None], T, [prm], first, td, _integ(mname), want_final=want_final)
        assert np.array_equal(Y[:, :m - 1], XD[:, :m - 1])
        assert np.all(Y[:, m - 1:] == SENTINEL)                                # the last sample is final_state's; the padding
        if want_final:
            assert np.array_equal(F[:, 0], XD[:, -1])


def _batch_problem():
    """B = 3 nine-node fixtures of p = (1, 2, 0), each on its own grid, own sample counts, one global first[]."""
    n, B = M.BATCH_N, len(M.BATCH_SETS)
    fx = [M.fixture(n, k) for k in M.BATCH_SETS]
    XC = np.asfortranarray(np.stack([f[0] for f in fx], axis=2))
    T = np.asfortranarray(np.stack([np.array(f[1]) * (1.0 + 0.125 * b) for b, f in enumerate(fx)], axis=1))   # B different grids
    tds, firsts, off = [], [], [0]
    for b in range(B):
        t = T[:, b]
        lo = t[0] if b != 1 else t[1] + 0.25 * (t[2] - t[1])                    # trajectory 1: no sample in its first segment
        hi = t[-1] if b == 0 else t[-1] - 0.3 * (t[-1] - t[-2])
        td = A.linrange(lo, hi, M.BATCH_COUNTS[b])
        tds.append(td)
        firsts.append(D.segment_ranges(t, td, True)[:-1] + off[-1])
        off.append(off[-1] + td.size)
    first = np.concatenate(firsts + [np.array([off[-1]], dtype=np.int32)]).astype(np.int32)
    return XC, T, [f[2] for f in fx], tds, first, off


@pytest.mark.parametrize("mname", ["dop853", "rk4x64"])
def test_mixed_class_batch_equals_singles(gpu_ctx, oracle, mname):
    XC, T, prm_l, tds, first, off = _batch_problem()
    method, steps = M.METHODS[mname]
    _, e_m = M.self_errors()
    n, B = XC.shape[1], XC.shape[2]
    S = n - 1
    assert [q[6] for q in prm_l] == [1.0, 2.0, 0.0] and first[S] == first[S + 1]
    td_all = np.concatenate(tds)
    Y, F = _dev_dense(gpu_ctx, XC, T, prm_l, first, td_all, _integ(mname))
    Y0, _ = _dev_dense(gpu_ctx, XC, T, prm_l, first, td_all, _integ(mname), want_final=False)
    assert np.array_equal(Y0, Y) and np.all(Y[:, off[-1]:] == SENTINEL)
    for b in range(B):
        t = np.array(T[:, b])
        f = first[b * S:(b + 1) * S + 1]
        Yb = Y[:, off[b]:off[b + 1]]
        # the grids are stretched copies of the fixtures' (the nodes are then no trajectory; every segment is still a flow)
        node_ref, hop_ref = M.dense_expected(oracle, XC[:, :, b], t, prm_l[b], tds[b], f, method, steps, Y=Yb, base=off[b])
        if prm_l[b][6] > 1:
            assert M.clamp_gap(node_ref, prm_l[b]).min() >= M.CLAMP_CLEARANCE
        _check("batch[%d] %s" % (b, M.SETS[M.BATCH_SETS[b]].name), mname, Yb, node_ref, hop_ref, e_m)
        fn, fh = M.final_expected(oracle, XC[:, :, b], t, prm_l[b], tds[b], f, method, steps, Y=Yb, base=off[b])
        _check("batch[%d] final" % b, mname, F[:, b:b + 1], fn[:, None], fh[:, None], e_m)
        Y1, F1 = _dev_dense(gpu_ctx, XC[:, :, b:b + 1], np.asfortranarray(t[:, None]), [prm_l[b]], f - off[b], tds[b], _integ(mname))
        assert np.array_equal(Y1[:, :tds[b].size], Yb), b                          # bitwise equal to the single
        assert np.all(Y1[:, tds[b].size:] == SENTINEL)
        assert np.array_equal(F1[:, 0], F[:, b]), b


@pytest.mark.parametrize("k", range(len(M.SETS)), ids=[s.name for s in M.SETS])
def test_isp_to_infinity_is_the_12_row_dense_output(gpu_ctx, k):
    s = M.SETS[k]
    X, t, prm = M.fixture(9, k, isp=1e30)
    bar = max(1e-11, 10.0 * M.e_inf())
    XD, td = lto.densify_mass(X, t, lto.make_params(*prm), 33, ctx=gpu_ctx)
    X12, td12 = lto.densify(np.asfortranarray(X[M.IDX12]), t, lto.make_params(MU, DU, TU, s.thrust, M.M0, 1.0, s.p, s.rho), 33, ctx=gpu_ctx)
    e = M.rel_rows(XD[M.IDX12], X12)
    print("MEASURED Isp = 1e30 %s: rows 0-5, 7-12 against the 12-row densify %.3e (bar %.1e, e_inf %.2e)" % (s.name, e, bar, M.e_inf()))
    assert np.array_equal(td, td12)
    assert e <= bar
    assert np.all(XD[6] == M.M0)


def _code(fn, *a, **k):
    with pytest.raises(lto.LtoError) as ei:
        fn(*a, **k)
    return ei.value.code


def test_refusals(gpu_ctx):
    X, t, prm = M.fixture(9, 0)
    X = np.asarray(X)
    T = np.asfortranarray(np.array(t)[:, None])
    p = lto.make_params(*prm)
    td = A.linrange(t[0], t[-1], 5)
    first = D.segment_ranges(t, td, False)
    # methods the dense kernels are not built for
    for integ in (lto.integrator(lto.RKF78_FIXED, steps=8), lto.integrator(lto.RKF78_ADAPTIVE)):
        assert _code(lto.densify_mass, X, t, p, 5, integ, ctx=gpu_ctx) == -3
        assert _code(_dev_dense, gpu_ctx, X[:, :, None], T, [prm], first, td, integ) == -3
    # the mass entry on a 12-row plan; the 12-row entries on 14 rows
    X12 = np.asfortranarray(X[M.IDX12])
    assert _code(_dev_dense, gpu_ctx, X12[:, :, None], T, [prm], first, td, lto.integrator(), ndim=12) == -3
    assert _code(_dev_dense, gpu_ctx, X[:, :, None], T, [prm], first, td, lto.integrator(), mass=False) == -3
    assert _code(lto.densify, X, t, p, 5, ctx=gpu_ctx) == -3
    # NULL arguments
    import torch
    plan = lto.IndirectPlan(gpu_ctx, 9, 1, p, lto.integrator(), ndim=14)
    Xd = torch.from_numpy(synth.to_soa_nodes(X[:, :, None])).cuda()
    tg, ts = torch.from_numpy(np.array(t)).cuda(), torch.from_numpy(td).cuda()
    fi = torch.from_numpy(first).cuda()
    Y = torch.full((14, 5), SENTINEL, dtype=torch.float64, device="cuda")
    good = [Xd, 9, tg, 1, fi, ts, Y, 5]
    for k in (0, 2, 4, 5, 6):
        args = list(good)
        args[k] = None
        assert _code(plan.dense_mass, *args) == -2, k
    torch.cuda.synchronize()
    assert bool((Y == SENTINEL).all())                                            # nothing was launched
    plan.close()
    integ = lto.integrator()
    out, tdo = np.zeros((14, 5), order="F"), np.zeros(5)
    import ctypes
    fn = gpu_ctx.fn("indirect_densify_mass")
    ok = [gpu_ctx.handle, 9, X.ctypes.data, np.array(t).ctypes.data, ctypes.byref(p), ctypes.byref(integ), 5, out.ctypes.data, tdo.ctypes.data]
    Xc, tc = np.asfortranarray(X), np.array(t)
    ok[2], ok[3] = Xc.ctypes.data, tc.ctypes.data
    for k in (2, 3, 4, 5, 7, 8):
        args = list(ok)
        args[k] = None
        assert fn(*args) == -2, k
    assert fn(*(ok[:6] + [1] + ok[7:])) == -1                                     # n_desired < 2
    assert fn(*ok) == 0
