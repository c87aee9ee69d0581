"""CPU checks of the indirect mesh equidistribution: the properties of the host restatement the GPU tests compare the
device against (tests/remesh_reference.py), and the argument checks of the Python layers that need no device."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import remesh_reference as R  # noqa: E402
import lowthrustopt_amd as lto  # noqa: E402
from lowthrustopt_amd import drivers  # noqa: E402
from lowthrustopt_amd.constants import MU, DU, TU  # noqa: E402


@pytest.mark.parametrize("m", [1, 5, 63, 64, 65, 200, 4096, 4097, 70000])
def test_scan64_of_integers_is_the_running_sum(m):
    w = np.random.default_rng(m).integers(1, 70, m).astype(np.float64)
    assert np.array_equal(R.scan64(w), np.cumsum(w))


def test_scan64_of_reals_is_a_running_sum_to_rounding():
    w = np.random.default_rng(1).uniform(0.1, 5.0, 10000)
    c = R.scan64(w)
    assert np.all(np.diff(c) > 0.0)
    assert np.abs(c - np.cumsum(w)).max() <= 64 * np.finfo(float).eps * c[-1]


@pytest.mark.parametrize("n", [2, 3, 30, 257])
def test_equal_weights_give_back_the_old_grid(n):
    t = np.sort(np.random.default_rng(n).uniform(0.0, 3.0, n))
    t_new, _ = R.new_grid(t, np.ones(n - 1), n)
    assert np.array_equal(t_new, t)


@pytest.mark.parametrize("n,n_new", [(30, 30), (30, 15), (30, 120), (60, 30), (4097, 500)])
def test_grid_is_increasing_keeps_its_ends_and_equidistributes(n, n_new):
    rng = np.random.default_rng(n * 1000 + n_new)
    t = np.cumsum(np.concatenate([[0.25], rng.uniform(0.01, 0.2, n - 1)]))
    for w in (rng.uniform(0.2, 9.0, n - 1), rng.integers(3, 40, n - 1).astype(np.float64)):
        t_new, C = R.new_grid(t, w, n_new)
        assert t_new.shape == (n_new,)
        assert t_new[0] == t[0] and t_new[-1] == t[-1]             # bit for bit
        assert np.all(np.diff(t_new) > 0.0)
        share = R.monitor_share(t, w, t_new)
        assert np.abs(share - C[-1] / (n_new - 1)).max() <= 1e-11 * C[-1]
        i, span = R.sources(t, t_new)
        assert i[0] == 0 and span[0] == 0.0 and i[-1] == n - 1 and span[-1] == 0.0
        assert np.all(span >= 0.0) and np.all(span[1:-1] < np.diff(t)[np.minimum(i[1:-1], n - 2)])


def test_concentrated_monitor_puts_the_nodes_into_its_segment():
    n, n_new, heavy = 30, 30, 17
    t = np.linspace(0.0, 2.9, n)
    w = np.full(n - 1, 1e-9)
    w[heavy] = 1.0
    t_new, _ = R.new_grid(t, w, n_new)
    inside = (t_new > t[heavy]) & (t_new < t[heavy + 1])
    assert inside.sum() == n_new - 2
    assert inside[1:-1].all()


def _xc(n=6):
    return np.zeros((12, n), order="F"), np.linspace(0.0, 1.0, n)


def test_hotpath_argument_checks_need_no_device():
    XC, t = _xc()
    prm = lto.make_params(MU, DU, TU, 10.0, 1e3, 1.0, 1.0, 1.0)

    def code(**kw):
        with pytest.raises(lto.LtoError) as ei:
            lto.indirect_remesh(XC, t, prm, **kw)
        return ei.value.code

    assert code(n_new=1) == -1
    assert code(passes=0) == -1
    assert code(weights=np.ones(5), passes=2) == -1
    for bad in (0.0, -1.0, np.nan, np.inf):
        w = np.ones(5)
        w[2] = bad
        assert code(weights=w, passes=1) == -1
    with pytest.raises(ValueError):
        lto.indirect_remesh(XC, t, prm, weights=np.ones(6), passes=1)
    with pytest.raises(ValueError):
        lto.indirect_remesh(XC, t[:-1], prm)
    with pytest.raises(ValueError):
        lto.indirect_remesh(np.zeros(12), t, prm)


def test_driver_argument_checks_need_no_device():
    XC, t = _xc()
    with pytest.raises(ValueError):
        drivers.meshRefine_indirect(XC, t, MU, DU, TU, 7, 1e3, 10.0, 1.0, 1.0, verbose=False)
    with pytest.raises(ValueError):
        drivers.meshRefine_indirect(XC, t[:-1], MU, DU, TU, 6, 1e3, 10.0, 1.0, 1.0, verbose=False)
    with pytest.raises(lto.LtoError):
        drivers.meshRefine_indirect(XC, t, MU, DU, TU, 6, 1e3, 10.0, 1.0, 1.0, n_new=1, verbose=False)
    with pytest.raises(lto.LtoError):
        drivers.meshRefine_indirect(XC, t, MU, DU, TU, 6, 1e3, 10.0, 1.0, 1.0, weights=np.ones(5), passes=2, verbose=False)


def test_entry_points_are_declared_in_every_layer():
    from lowthrustopt_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "lto.h")).read()
    julia = open(os.path.join(root, "julia", "LowThrustOptHIP.jl")).read()
    for name in ("lto_indirect_remesh_batch", "lto_indirect_remesh"):
        assert name in _lib.SIGNATURES
        assert "int %s(" % name in header
        assert ":%s" % name in julia
