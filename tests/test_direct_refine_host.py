"""CPU checks of the direct mesh refinement's interface (lto_direct_refine_batch).  tests/test_cabi_symbols.py
already holds the header, the ctypes table and the Julia ccall against each other for every entry point; here: the two entries are
there at all, the single-trajectory form is the batch form without n_batch and n_tgrids, and hotpath.direct_refine refuses bad
arguments before it reaches the library."""
import re
import os

import numpy as np
import pytest

import lowthrustopt_amd as lto
from lowthrustopt_amd import _lib, hotpath

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entries_are_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "lto.h")).read()
    julia = open(os.path.join(ROOT, "julia", "LowThrustOptHIP.jl")).read()
    for name in ("lto_direct_refine_batch", "lto_direct_refine"):
        assert re.search(r"\bint %s\(lto_ctx\* ctx," % name, header)
        assert name in _lib.SIGNATURES
    assert "(:lto_direct_refine, liblto)" in julia and re.search(r"^export[^#]*\bdirect_refine\b", julia, re.S | re.M)
    batch, one = _lib.SIGNATURES["lto_direct_refine_batch"], _lib.SIGNATURES["lto_direct_refine"]
    assert batch[0] is one[0]
    args = list(batch[1])
    del args[7]            # n_tgrids
    del args[3]            # n_batch
    assert args == list(one[1])


class NoLibrary:
    """A context whose library must not be reached."""
    handle = None

    def fn(self, name):
        raise AssertionError("the library was called: lto_" + name)

    def check(self, rc):
        raise AssertionError("the library was called")


def test_wrapper_refuses_before_the_library():
    X = np.zeros((6, 5), order="F")
    U = np.zeros((3, 5), order="F")
    t = np.arange(5.0)
    good = dict(nsteps=10, MU=lto.MU, DU=lto.DU, TU=lto.TU, Isp=2000.0, tol_min=1e-16, tol_max=1e-13, max_nodes=8, ctx=NoLibrary())

    def call(X=X, U=U, t=t, **kw):
        return hotpath.direct_refine(X, U, t, **{**good, **kw})

    with pytest.raises(AssertionError, match="the library was called"):
        call()                                           # the good call does get that far
    for bad in (dict(X=np.zeros((5, 5))), dict(X=np.zeros((8, 5))), dict(X=np.zeros(6)), dict(X=np.zeros((6, 5, 2, 2))),
                dict(X=np.zeros((6, 1)), U=np.zeros((3, 1)), t=np.zeros(1)), dict(U=np.zeros((3, 4))), dict(U=np.zeros((2, 5))),
                dict(U=np.zeros((3, 5, 2))), dict(t=np.arange(4.0)), dict(t=np.zeros((5, 2))),
                dict(X=np.zeros((6, 5, 2)), U=np.zeros((3, 5, 2)), t=np.zeros((5, 3)))):
        with pytest.raises(ValueError):
            call(**bad)
    for bad in (dict(nsteps=1), dict(max_nodes=4), dict(tol_min=np.nan), dict(tol_max=np.nan)):
        with pytest.raises(lto.LtoError):
            call(**bad)
