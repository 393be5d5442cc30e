"""The device-resident controller on band batches, what needs no GPU: the new entry point is
declared, bound and exported, PGF_BATCH_BAND_CTL has one value everywhere, the refusals that come
before any device call, and BatchedDeviceNewton passes the flags it was asked for and no others."""

import ctypes as C
import os
import re

import numpy as np


def test_new_symbol_and_flag_are_declared_bound_and_exported():
    from pygradflow_amd import _lib

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(repo, "include", "pgf_hip.h")).read()
    lib = _lib.load()
    name = "pgf_batch_debug_ctl_stats"
    assert re.search(r"\b%s\s*\(" % name, header)
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    m = re.search(r"#define\s+PGF_BATCH_BAND_CTL\s+(\d+)u", header)
    assert m and int(m.group(1)) == _lib.BATCH_BAND_CTL == 2
    assert _lib.BATCH_BAND_CTL & _lib.BATCH_WIDE_BAND == 0


def test_stats_of_no_batch_are_refused_and_leave_the_outputs_alone():
    from pygradflow_amd import _lib

    lib = _lib.load()
    piv = np.full(3, 7, dtype=np.int32)
    grd = np.full(3, 9, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    assert lib.pgf_batch_debug_ctl_stats(None, piv.ctypes.data_as(ip), grd.ctypes.data_as(ip)) == _lib.PGF_INVALID
    assert lib.pgf_batch_debug_ctl_stats(None, None, None) == _lib.PGF_INVALID
    assert list(piv) == [7] * 3 and list(grd) == [9] * 3


def test_create_ex_refuses_null_handles_under_every_flag():
    from pygradflow_amd import _lib

    lib = _lib.load()
    out = C.c_void_p()
    none = (C.c_void_p * 2)(None, None)
    for flags in (2, 3, 4):  # the new flag, both flags, the first unknown bit
        assert lib.pgf_batch_create_ex(none, 2, flags, C.byref(out)) == _lib.PGF_INVALID
        assert lib.pgf_batch_create_ex(None, 2, flags, C.byref(out)) == _lib.PGF_INVALID
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


def test_the_flags_are_passed_only_when_asked():
    import inspect

    from pygradflow_amd import _lib
    from pygradflow_amd.batched import BatchedDeviceNewton

    assert inspect.signature(BatchedDeviceNewton.__init__).parameters["band_ctl"].default is False
    for wide, ctl, want in ((False, False, ("pgf_batch_create", 3)),
                            (True, False, ("pgf_batch_create_ex", 3, 1)),
                            (False, True, ("pgf_batch_create_ex", 3, 2)),
                            (True, True, ("pgf_batch_create_ex", 3, 3))):
        bd = object.__new__(BatchedDeviceNewton)  # (the constructor needs a device for its norms)
        bd.count, bd.wide_band, bd.band_ctl, bd._lib = 3, wide, ctl, _lib
        rec = _RecordingLib()
        assert bd._create(rec, None, None) == 0
        assert rec.calls == [want], (wide, ctl)


def test_ctl_init_on_a_band_batch_needs_the_flag():
    """Before any library call: a band batch without band_ctl raises the old error."""
    import pytest

    from pygradflow_amd.batched import BatchedDeviceNewton

    bd = object.__new__(BatchedDeviceNewton)
    bd._b, bd.band, bd.band_ctl = object(), True, False
    with pytest.raises(NotImplementedError, match="dense batch only"):
        bd.ctl_init(None)
