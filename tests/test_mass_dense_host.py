"""CPU checks behind the variable-mass dense-output and re-mesh tests: the fixtures of tests/mass_dense_reference.py
are admitted, the reference agrees with itself inside the bars the GPU tests use, and the new names exist at every layer that can
be inspected without a device.

Measured (printed before each assertion): oracle chained hop by hop against oracle from the node, DOP853: 3.4e-14 per row over
DENSE_CASES; e_m = 6.8e-13 kg (the Isp = 20 s fixture, 99 kg burnt), so the mass bar max(10 e_m, 64 eps m0) is its floor
1.42e-11 kg; same-method RK4 hops: 0 (the reference against itself is the same arithmetic); e_inf = 1.7e-14."""
import numpy as np
import pytest

import mass_dense_reference as M
import lowthrustopt_amd as lto
from lowthrustopt_amd import _lib, drivers
from lowthrustopt_amd.constants import MU, DU, TU

FIXTURES = sorted({(c.n, c.k, c.lin, None) for c in M.DENSE_CASES} | {(9, k, False, None) for k in range(len(M.SETS))}
                  | {(66, 0, False, None), (130, 0, False, None)} | {(n, k, False, g) for n, k, g in M.REMESH_BATCH}, key=str)


@pytest.mark.parametrize("n,k,lin,gseed", FIXTURES)
def test_fixture_is_admitted(oracle, n, k, lin, gseed):
    X, t, prm = M.fixture(n, k, lin, gseed=gseed)
    d = M.fixture_defect(oracle, X, t, prm)
    print("fixture n=%d %s: max |defect| %.3e, max |X| %.3e, mass %.6f -> %.6f kg" % (n, M.SETS[k].name, np.abs(d).max(), np.abs(X).max(), X[6, 0], X[6, -1]))
    assert np.all(np.isfinite(X)) and np.all(np.diff(t) > 0.0)
    assert np.abs(d).max() <= 1e-12 * np.abs(X).max()
    assert X[6, 0] == M.M0 and np.all(np.diff(X[6]) <= 0.0) and X[6, -1] > 0.0
    if prm[6] <= 1:
        assert X[13, -1] == 0.0
    else:
        assert X[13, 0] == M.LAMBDA_M0                       # not shifted: lambda_m feeds back for p > 1
        gap = M.clamp_gap(X, prm).min()
        print("   clamp clearance at the nodes %.4f" % gap)
        assert gap >= M.CLAMP_CLEARANCE


@pytest.mark.parametrize("c", [c for c in M.DENSE_CASES if M.SETS[c.k].p > 1], ids=M.case_id)
def test_clamp_clearance_at_every_sample(c):
    _, node_ref, _ = M.case_reference(c, "dop853")
    gap = M.clamp_gap(node_ref, M.fixture(c.n, c.k, c.lin)[2]).min()
    print("%s: clamp clearance over the samples %.4f" % (M.case_id(c), gap))
    assert gap >= M.CLAMP_CLEARANCE


def test_every_parameter_set_is_covered():
    assert {c.k for c in M.DENSE_CASES} == set(range(len(M.SETS)))
    assert [(c.n, c.n_desired) for c in M.DENSE_CASES] == [(2, 2), (2, 65), (3, 2), (13, 5), (13, 13), (66, 129)]
    assert "rk4x8" in M.DENSE_CASES[1].methods


def test_reference_agrees_with_itself_inside_the_bars():
    e_node, e_m = M.self_errors()
    print("MEASURED oracle hop by hop vs oracle from the node (DOP853): per row %.3e, mass row e_m = %.3e kg; mass bar %.3e kg"
          % (e_node, e_m, M.mass_bar(e_m)))
    assert 10.0 * e_node <= M.TOL["dop853"]
    assert e_m <= 64.0 * M.EPS * M.M0                        # the floor decides the mass bar
    # same-method RK4 hops: the hop-by-hop reference is reproducible bit for bit
    for c in M.DENSE_CASES[:3]:
        X, t, prm = M.fixture(c.n, c.k, c.lin)
        again = M.densify_expected(M.oracle_mod(), X, t, prm, c.n_desired, *M.METHODS["rk4x64"])[2]
        assert np.array_equal(again, M.case_reference(c, "rk4x64")[2], equal_nan=True)


def test_lin_grid_samples_are_the_nodes():
    c = M.DENSE_CASES[4]
    X, t, _ = M.fixture(c.n, c.k, c.lin)
    td, node_ref, hop_ref = M.case_reference(c, "dop853")
    assert np.array_equal(td, t)
    assert np.array_equal(node_ref[:, :-1], X[:, :-1]) and np.array_equal(hop_ref[:, :-1], X[:, :-1])


def test_isp_to_infinity_is_the_12_row_flow():
    e = M.e_inf()
    print("MEASURED e_inf = %.3e (oracle 14-row flow at Isp = 1e30, rows 0-5 and 7-12, against the oracle's 12-row flow)" % e)
    assert e <= 1e-12
    X, _, _ = M.fixture(9, 0, isp=1e30)
    assert np.all(X[6] == M.M0)


NEW_NAMES = ("lto_indirect_dense_mass_dev", "lto_indirect_densify_mass", "lto_indirect_remesh_mass_batch", "lto_indirect_remesh_mass")


def test_new_names_are_bound():
    for name in NEW_NAMES:
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["lto_indirect_dense_mass_dev"][1]) == len(_lib.SIGNATURES["lto_indirect_dense_dev"][1])
    # the mass entries drop ndim
    assert len(_lib.SIGNATURES["lto_indirect_densify_mass"][1]) == len(_lib.SIGNATURES["lto_indirect_densify"][1]) - 1
    assert len(_lib.SIGNATURES["lto_indirect_remesh_mass_batch"][1]) == len(_lib.SIGNATURES["lto_indirect_remesh_batch"][1]) - 1
    assert len(_lib.SIGNATURES["lto_indirect_remesh_mass"][1]) == len(_lib.SIGNATURES["lto_indirect_remesh"][1]) - 1
    for name in ("densify_mass", "indirect_remesh_mass"):
        assert callable(getattr(lto, name))
    assert callable(lto.IndirectPlan.dense_mass) and callable(drivers.meshRefine_indirect_mass)
    assert "densify_mass" in lto.densify.__doc__
    assert lto.load_library().lto_version() == 102


def test_driver_refuses_other_shapes_before_any_library_call(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the library was called")
    monkeypatch.setattr(lto.hotpath, "indirect_remesh_mass", boom)
    monkeypatch.setattr(lto.hotpath, "default_context", boom)
    n = 9
    t = np.linspace(0.0, 1.0, n)
    args = (MU, DU, TU, n, 2000.0, 0.05, 1.0, 1.0)
    with pytest.raises(ValueError):
        drivers.meshRefine_indirect_mass(np.zeros((12, n)), t, *args, verbose=False)
    with pytest.raises(ValueError):
        drivers.meshRefine_indirect_mass(np.zeros((14, n + 1)), t, *args, verbose=False)
    with pytest.raises(ValueError):
        drivers.meshRefine_indirect_mass(np.zeros((14, n)), t[:-1], *args, verbose=False)
    with pytest.raises(ValueError):
        drivers.meshRefine_indirect_mass(np.zeros((14, n)), np.stack([t, t], axis=1), *args, verbose=False)
    with pytest.raises(ValueError):
        lto.densify_mass(np.zeros((12, n)), t, lto.make_params(MU, DU, TU, 0.05, 2000.0, 1.0, 1.0, 1.0), 5)
    with pytest.raises(ValueError):
        lto.indirect_remesh_mass(np.zeros((12, n)), t, lto.make_params(MU, DU, TU, 0.05, 2000.0, 1.0, 1.0, 1.0))
