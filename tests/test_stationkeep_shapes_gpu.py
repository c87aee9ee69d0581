"""GPU shape sweep of the two one-lane-per-record gain kernels (lto_stationkeep_gains_batch, DESIGN 4.29, and
lto_stationkeep_target_gains_batch): launches with a second block and a partly filled last one, up to 129 records and
five targets, inputs that are not the packaged orbits' (random unit-vector pairs, the eigen family of
tests/test_manifold_shapes_host.py, random finite STMs of magnitude 1 to 1e3), and bad records on both sides of the 64-lane edge.

Both kernels are reproducible on the host bit for bit by contract, so every comparison with the reference loops
(tests/stationkeep_reference.py, tests/stationkeep_target_reference.py) is bit for bit and no bound is needed."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import manifold_reference as MR  # noqa: E402
import stationkeep_reference as SR  # noqa: E402
import stationkeep_target_reference as TR  # noqa: E402
import test_manifold_shapes_host as HS  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import synth  # noqa: E402
from lowthrustopt_amd.constants import MU  # noqa: E402

pytestmark = pytest.mark.gpu


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# --------------------------------------------------------------------------------------------------------------- 1. Floquet gains
def _vector_pairs(P, B):
    """V [6 x 2 x P x B]: the even records random pairs of unit vectors, the odd ones the 50-digit (v_u, v_s) of members of the
    eigen family (P applied to the vectors of one matrix)."""
    rng = np.random.RandomState(100 * P + B)
    e0 = HS.shared_pair("family", HS.family_matrix())
    V = np.empty((6, 2, P, B), order="F")
    for g in range(P * B):
        j, b = g % P, g // P
        if g % 2 == 0:
            v = rng.uniform(-1.0, 1.0, (6, 2))
            V[:, :, j, b] = v / np.linalg.norm(v, axis=0)
        else:
            e = MR.permuted_pair(e0, HS.PERMS[(37 * g) % 720])
            V[:, 0, j, b], V[:, 1, j, b] = e.v_u, e.v_s
    return V


def _same_gains(r, ref):
    return all(np.array_equal(np.asarray(a).reshape(b.shape), b, equal_nan=True) for a, b in zip((r.W, r.G, r.alpha, r.status), ref))


@pytest.mark.parametrize("P,B", [(1, 1), (63, 1), (1, 64), (13, 5), (43, 3)])
def test_floquet_gains_equal_the_reference_loops_bit_for_bit(gpu_ctx, P, B):
    V = _vector_pairs(P, B)
    ref = SR.gains(V, 1e-8)
    r = lto.stationkeep_gains(V, ctx=gpu_ctx)
    print("%d phases x %d orbits = %d records: alpha %.3f .. %.3f, |G| <= %.3g" % (P, B, P * B, ref[2].min(), ref[2].max(), np.abs(ref[1]).max()))
    assert np.all(ref[3] == 0) and r.G.shape == (3, 6, P, B)
    assert _same_gains(r, ref)
    # W and alpha left out: G does not move
    Vf = np.asfortranarray(V)
    G, status = np.zeros((3, 6, P, B), order="F"), np.zeros((P, B), dtype=np.int32, order="F")
    rc = gpu_ctx.fn("stationkeep_gains_batch")(gpu_ctx.handle, P, B, _p(Vf), 1e-8, None, _p(G), None, _p(status))
    assert rc == 0 and np.array_equal(G, ref[1]) and np.array_equal(status, ref[3])


def test_floquet_gains_flag_bad_records_on_both_sides_of_the_block_edge(gpu_ctx):
    """129 records; records 0, 63, 64 and 128 hold a NaN, an Inf, a v_s without a position part (w_v = 0: alpha = 0) and a NaN in
    v_u: status 2, 2, 3, 2 and NaN there and nowhere else."""
    P, B = 43, 3
    V = _vector_pairs(P, B)
    clean = lto.stationkeep_gains(V, ctx=gpu_ctx)
    Vb = V.copy(order="F")
    flat = Vb.reshape(6, 2, P * B, order="F")                        # a view: record g = j + P b
    assert np.shares_memory(flat, Vb)
    flat[2, 1, 0] = np.nan
    flat[3, 0, 63] = np.inf
    flat[:3, 1, 64] = 0.0
    flat[5, 0, 128] = np.nan
    ref = SR.gains(Vb, 1e-8)
    r = lto.stationkeep_gains(Vb, ctx=gpu_ctx)
    want = np.zeros(P * B, dtype=np.int32)
    want[[0, 63, 64, 128]] = 2, 2, 3, 2
    assert np.array_equal(r.status.reshape(-1, order="F"), want) and np.array_equal(ref[3].reshape(-1, order="F"), want)
    assert _same_gains(r, ref)
    bad = want != 0
    W, G, alpha = r.W.reshape(6, -1, order="F"), r.G.reshape(3, 6, -1, order="F"), r.alpha.reshape(-1, order="F")
    assert np.all(np.isnan(W[:, bad])) and np.all(np.isnan(G[:, :, bad])) and np.all(np.isnan(alpha[bad]))
    assert np.array_equal(W[:, ~bad], clean.W.reshape(6, -1, order="F")[:, ~bad])
    assert np.array_equal(G[:, :, ~bad], clean.G.reshape(3, 6, -1, order="F")[:, :, ~bad])
    assert np.array_equal(alpha[~bad], clean.alpha.reshape(-1, order="F")[~bad])


# ----------------------------------------------------------------------------------------------------------- 2. target-point gains
def _random_stms(K, n, seed):
    """Phi [6 x 6 x K x n]: entries uniform in (-1, 1) times a magnitude 10^U(0, 3) of the record's own."""
    rng = np.random.RandomState(seed)
    Phi = rng.uniform(-1.0, 1.0, (6, 6, K, n)) * 10.0 ** rng.uniform(0.0, 3.0, (1, 1, 1, n))
    return np.asfortranarray(Phi)


WEIGHTS = {1: (1.0,), 2: (0.5, 2.0), 3: (1.0, 0.0, 2.0), 5: (1.0, 0.25, 3.0, 1.0, 0.5)}        # one target of the three weighs nothing


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
@pytest.mark.parametrize("K", [1, 2, 3, 5])
def test_target_gains_equal_the_reference_loops_bit_for_bit(gpu_ctx, K, n):
    Phi = _random_stms(K, n, 1000 * K + n)
    q = TR.Q if (K + n) % 2 else 1.0
    G, pivot, status = TR.gains(Phi, q, WEIGHTS[K])
    g = lto.stationkeep_target_gains(Phi, q=q, r=WEIGHTS[K], ctx=gpu_ctx)
    print("%d records x %d targets, q %g: max |Phi| %.3g .. %.3g, pivot %.1e .. %.1e" % (n, K, q, np.abs(Phi).max(axis=(0, 1, 2)).min(),
                                                                                      np.abs(Phi).max(), np.nanmin(pivot), np.nanmax(pivot)))
    assert np.all(status == 0)
    assert np.array_equal(g.G, G) and np.array_equal(g.pivot, pivot) and np.array_equal(g.status, status)


def test_target_gains_of_the_devices_own_stms_with_three_targets(gpu_ctx):
    orbits = MR.packaged_orbits(synth.halo_orbits(), MU)
    s0, per = np.stack([orbits[k][0] for k in (0, 1, 0)], axis=1), np.array([orbits[k][1] for k in (0, 1, 0)])
    s = lto.halo_stm(s0, per, TR.TAUS3, (0.25, 0.5, 1.0), MU=MU, integ=lto.integrator(rtol=TR.RTOL, atol=TR.ATOL), ctx=gpu_ctx)
    assert np.all(s.status == 0) and s.Phi.shape == (6, 6, 3, 3, 3)
    flat = s.Phi.reshape(6, 6, 3, 9, order="F")
    Phi = np.asfortranarray(np.stack([flat[:, :, :, g % 9] * (1.0 + 0.03125 * (g // 9)) for g in range(65)], axis=3))
    for r in (WEIGHTS[3], (1.0, 1.0, 1.0)):
        G, pivot, status = TR.gains(Phi, TR.Q, r)
        g = lto.stationkeep_target_gains(Phi, q=TR.Q, r=r, ctx=gpu_ctx)
        assert np.all(status == 0)
        assert np.array_equal(g.G, G) and np.array_equal(g.pivot, pivot) and np.array_equal(g.status, status)


def test_rank_deficient_records_on_both_sides_of_the_block_edge(gpu_ctx):
    """q = 0, one target: a B_1 of rank two (a zero column in record 0, two equal columns in record 63, a zero row pair that leaves
    rank one in record 64) has no inverse: status 3 there; the records beside them are what their single calls give."""
    Phi = _random_stms(1, 65, 4242)
    Phi[:3, 5, 0, 0] = 0.0
    Phi[:3, 4, 0, 63] = Phi[:3, 3, 0, 63]
    Phi[1:3, 3:, 0, 64] = 0.0
    G, pivot, status = TR.gains(Phi, 0.0, (1.0,))
    g = lto.stationkeep_target_gains(Phi, q=0.0, r=(1.0,), ctx=gpu_ctx)
    want = np.zeros(65, dtype=np.int32)
    want[[0, 63, 64]] = 3
    assert np.array_equal(status, want) and np.array_equal(g.status, want)
    assert np.array_equal(g.G, G, equal_nan=True) and np.array_equal(g.pivot, pivot, equal_nan=True)
    bad = want != 0
    assert np.all(np.isnan(g.G[:, :, bad])) and np.all(np.isnan(g.pivot[bad])) and np.all(np.isfinite(g.G[:, :, ~bad]))
    for b in (1, 62):
        one = lto.stationkeep_target_gains(Phi[:, :, :, b], q=0.0, r=(1.0,), ctx=gpu_ctx)
        assert one.status == 0 and np.array_equal(one.G, g.G[:, :, b]) and one.pivot == g.pivot[b]
    # with q > 0 the same records are regular
    g1 = lto.stationkeep_target_gains(Phi, q=1.0, r=(1.0,), ctx=gpu_ctx)
    ref1 = TR.gains(Phi, 1.0, (1.0,))
    assert np.all(g1.status == 0) and np.array_equal(g1.G, ref1[0]) and np.array_equal(g1.pivot, ref1[1])
