"""Banded device batch, what needs no GPU: the new entry points are bound, the refusals that come
before any device call, and the pattern hash a band batch compares."""

import ctypes as C

import numpy as np
import pytest


def test_new_symbols_are_declared_bound_and_exported():
    import os
    import re

    from pygradflow_amd import _lib

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(repo, "include", "pgf_hip.h")).read()
    lib = _lib.load()
    for name in ("pgf_batch_debug_band_stats", "pgf_sparse_pattern_hash"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    a, b = C.c_int(7), C.c_int(7)
    assert lib.pgf_batch_debug_band_stats(None, C.byref(a), C.byref(b)) == _lib.PGF_INVALID
    assert (a.value, b.value) == (7, 7)


def test_refusals_before_any_device_call():
    from pygradflow_amd import _lib
    from pygradflow_amd.batched import batch_kind

    lib = _lib.load()
    out = C.c_void_p()
    none = (C.c_void_p * 2)(None, None)
    assert lib.pgf_batch_create(none, 2, C.byref(out)) == _lib.PGF_INVALID
    assert lib.pgf_batch_create(none, 0, C.byref(out)) == _lib.PGF_INVALID
    assert lib.pgf_batch_create(None, 2, C.byref(out)) == _lib.PGF_INVALID
    assert not out.value
    # one (n, m) whatever the kind; banded only when every instance is
    assert batch_kind([(300, 0, True)] * 3) == "band"
    assert batch_kind([(300, 0, False)] * 3) == "dense"
    assert batch_kind([(300, 0, True), (300, 0, False)]) == "dense"  # (the library refuses the mix)
    with pytest.raises(ValueError, match=r"one \(n, m\)"):
        batch_kind([(300, 0, True), (301, 0, True)])
    with pytest.raises(ValueError, match=r"one \(n, m\)"):
        batch_kind([(300, 2, False), (300, 0, False)])


def _plan(prob):
    from pygradflow_amd.sparse import BandPlan

    return BandPlan(prob.hess_sparse(), prob.jac_sparse(), prob.num_vars, prob.num_cons)


def test_pattern_hash_follows_the_pattern_and_nothing_else():
    from pygradflow_amd import _lib, problems

    a, b = _plan(problems.multistate_ocp(20, 3, 1, seed=0)), _plan(problems.multistate_ocp(20, 3, 1, seed=1))
    assert a is not b and a.pos is not b.pos and np.array_equal(a.pos, b.pos)
    ha = a.pattern_hash()
    assert ha == b.pattern_hash() == a.pattern_hash() and ha != 0  # other values, other objects
    assert ha != _plan(problems.multistate_ocp(21, 3, 1)).pattern_hash()
    assert _plan(problems.box_qp(64, seed=0)).pattern_hash() == _plan(problems.box_qp(64, seed=3)).pattern_hash()
    # one index differs, in any of the arrays
    for name in ("pos", "Hcol", "Hslot", "Jcol", "Jslot", "JTrow", "JTmap", "Hptr", "JTptr"):
        arr = getattr(b, name)
        keep = arr.copy()
        arr[len(arr) // 2] += 1
        assert b.pattern_hash() != ha, name
        arr[:] = keep
        assert b.pattern_hash() == ha, name
    b.bw += 1
    assert b.pattern_hash() != ha
    # null arrays are an error, not a hash
    out = C.c_uint64(0)
    assert _lib.load().pgf_sparse_pattern_hash(4, 0, 1, None, 0, None, None, None, None, 0, None, None, None,
                                               None, None, None, C.byref(out)) == _lib.PGF_INVALID
