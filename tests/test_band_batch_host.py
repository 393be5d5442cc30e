"""Banded device batch and its routes (wide bands, the device-resident controller, borders on either
route), what needs no GPU: the entry points are declared, bound and exported, every creation flag
has one value everywhere and its own bit, the refusals that come before any device call,
BatchedDeviceNewton passes the flags it was asked for and no others, and the pattern hash a band
batch compares."""

import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


# (entry point, creation flag, its value) each route added (test_new_symbols_are_declared_bound_and_exported
# above has the first route's)
ROUTES = [("pgf_batch_create_ex", None, None),
          ("pgf_batch_debug_band_wide_stats", "WIDE_BAND", 1),
          ("pgf_batch_debug_ctl_stats", "BAND_CTL", 2),
          ("pgf_batch_debug_border_stats", "BORDER", 4),
          (None, "WIDE_BORDER", 8)]
FLAGS = {flag: value for _, flag, value in ROUTES if flag}


@pytest.mark.parametrize("name,flag,value", ROUTES, ids=[flag or name for name, flag, _ in ROUTES])
def test_symbol_and_flag_are_declared_bound_and_exported(name, flag, value):
    from pygradflow_amd import _lib

    header = open(os.path.join(REPO, "include", "pgf_hip.h")).read()
    if name:
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
    if flag:
        m = re.search(r"#define\s+PGF_BATCH_%s\s+(\d+)u" % flag, header)
        assert m and int(m.group(1)) == getattr(_lib, "BATCH_" + flag) == value
        assert all(value & v == 0 for f, v in FLAGS.items() if f != flag)


@pytest.mark.parametrize("name", ["pgf_batch_debug_ctl_stats", "pgf_batch_debug_border_stats"])
def test_stats_of_no_batch_are_refused_and_leave_the_outputs_alone(name):
    from pygradflow_amd import _lib

    stats = getattr(_lib.load(), name)
    a = np.full(3, 7, dtype=np.int32)
    b = np.full(3, 9, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    assert stats(None, a.ctypes.data_as(ip), b.ctypes.data_as(ip)) == _lib.PGF_INVALID
    assert stats(None, None, None) == _lib.PGF_INVALID
    assert list(a) == [7] * 3 and list(b) == [9] * 3


def test_wide_stats_of_no_batch_are_refused_and_leave_the_output_alone():
    from pygradflow_amd import _lib

    lean = C.c_int(7)
    assert _lib.load().pgf_batch_debug_band_wide_stats(None, None, None, C.byref(lean)) == _lib.PGF_INVALID
    assert lean.value == 7


def test_create_ex_refuses_null_handles_under_every_flag():
    """Every subset of the four flags, the first unknown bit and the last."""
    from pygradflow_amd import _lib

    lib = _lib.load()
    out = C.c_void_p()
    none = (C.c_void_p * 2)(None, None)
    assert sum(FLAGS.values()) == 15
    for flags in list(range(17)) + [0x80000000]:
        assert lib.pgf_batch_create_ex(none, 2, flags, C.byref(out)) == _lib.PGF_INVALID, flags
        assert lib.pgf_batch_create_ex(none, 0, flags, C.byref(out)) == _lib.PGF_INVALID, flags
        assert lib.pgf_batch_create_ex(None, 2, flags, C.byref(out)) == _lib.PGF_INVALID, flags
    assert lib.pgf_batch_create_ex(none, 2, 0, None) == _lib.PGF_INVALID
    assert not out.value


class _RecordingLib:
    def __init__(self):
        self.calls = []

    def pgf_batch_create(self, handles, count, out):
        self.calls.append(("pgf_batch_create", count))
        return 0

    def pgf_batch_create_ex(self, handles, count, flags, out):
        self.calls.append(("pgf_batch_create_ex", count, flags))
        return 0


# (attributes the object has, flags _create passes: None for pgf_batch_create).  An object built
# without band_ctl, border or wide_border (older callers of __new__) asks for none of them.
CREATE = [(dict(wide_band=False), None),
          (dict(wide_band=True), 1),
          (dict(wide_band=False, band_ctl=False), None),
          (dict(wide_band=True, band_ctl=False), 1),
          (dict(wide_band=False, band_ctl=True), 2),
          (dict(wide_band=True, band_ctl=True), 3),
          (dict(wide_band=False, band_ctl=False, border=False), None),
          (dict(wide_band=False, band_ctl=False, border=True), 4),
          (dict(wide_band=True, band_ctl=False, border=True), 4 | 1),
          (dict(wide_band=False, band_ctl=True, border=True), 4 | 2),
          (dict(wide_band=True, band_ctl=True, border=False), 3),
          (dict(wide_band=True, band_ctl=False, border=True, wide_border=True), 8 | 4 | 1),
          (dict(wide_band=True, band_ctl=True, border=True, wide_border=True), 15),
          (dict(wide_band=True, band_ctl=False, border=True, wide_border=False), 4 | 1),
          (dict(wide_band=False, band_ctl=False, border=False, wide_border=False), None)]


def test_the_flags_are_passed_only_when_asked():
    from pygradflow_amd import _lib
    from pygradflow_amd.batched import BatchedDeviceNewton

    for keyword in ("wide_band", "band_ctl", "border", "wide_border"):
        assert inspect.signature(BatchedDeviceNewton.__init__).parameters[keyword].default is False
    # (the constructor needs a device for its norms: the GPU tests see what it derives from wide_border)
    for attrs, flags in CREATE:
        bd = object.__new__(BatchedDeviceNewton)
        bd.count, bd._lib = 3, _lib
        for name, value in attrs.items():
            setattr(bd, name, value)
        rec = _RecordingLib()
        assert bd._create(rec, None, None) == 0
        assert rec.calls == [("pgf_batch_create_ex", 3, flags) if flags else ("pgf_batch_create", 3)], attrs


def test_ctl_init_on_a_band_batch_needs_the_flag():
    """Before any library call: a band batch without band_ctl raises the old error."""
    from pygradflow_amd.batched import BatchedDeviceNewton

    bd = object.__new__(BatchedDeviceNewton)
    bd._b, bd.band, bd.band_ctl = object(), True, False
    with pytest.raises(NotImplementedError, match="dense batch only"):
        bd.ctl_init(None)


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
