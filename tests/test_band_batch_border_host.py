"""Bordered instances in a band batch, what needs no GPU: PGF_BATCH_BORDER has one value everywhere,
the new entry point is declared, bound and exported, the refusals that come before any device call,
and BatchedDeviceNewton passes the flags it was asked for and no others."""

import ctypes as C
import os
import re

import numpy as np


def test_new_symbol_and_flag_are_declared_bound_and_exported():
    from pygradflow_amd import _lib

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(repo, "include", "pgf_hip.h")).read()
    lib = _lib.load()
    name = "pgf_batch_debug_border_stats"
    assert re.search(r"\b%s\s*\(" % name, header)
    assert name in _lib.SIGNATURES and hasattr(lib, name)
    m = re.search(r"#define\s+PGF_BATCH_BORDER\s+(\d+)u", header)
    assert m and int(m.group(1)) == _lib.BATCH_BORDER == 4
    assert _lib.BATCH_BORDER & (_lib.BATCH_BAND_CTL | _lib.BATCH_WIDE_BAND) == 0


def test_stats_of_no_batch_are_refused_and_leave_the_outputs_alone():
    from pygradflow_amd import _lib

    lib = _lib.load()
    fac = np.full(3, 7, dtype=np.int32)
    sol = np.full(3, 9, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    assert lib.pgf_batch_debug_border_stats(None, fac.ctypes.data_as(ip), sol.ctypes.data_as(ip)) == _lib.PGF_INVALID
    assert lib.pgf_batch_debug_border_stats(None, None, None) == _lib.PGF_INVALID
    assert list(fac) == [7] * 3 and list(sol) == [9] * 3


def test_create_ex_refuses_null_handles_under_every_flag():
    from pygradflow_amd import _lib

    lib = _lib.load()
    out = C.c_void_p()
    none = (C.c_void_p * 2)(None, None)
    for flags in (4, 5, 6, 7, 8):  # the new flag alone and with the others, the next unknown bit
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

    assert inspect.signature(BatchedDeviceNewton.__init__).parameters["border"].default is False
    for wide, ctl, border, want in ((False, False, False, ("pgf_batch_create", 3)),
                                    (False, False, True, ("pgf_batch_create_ex", 3, 4)),
                                    (True, False, True, ("pgf_batch_create_ex", 3, 4 | 1)),
                                    (False, True, True, ("pgf_batch_create_ex", 3, 4 | 2)),
                                    (True, True, False, ("pgf_batch_create_ex", 3, 3))):
        bd = object.__new__(BatchedDeviceNewton)  # (the constructor needs a device for its norms)
        bd.count, bd.wide_band, bd.band_ctl, bd.border, bd._lib = 3, wide, ctl, border, _lib
        rec = _RecordingLib()
        assert bd._create(rec, None, None) == 0
        assert rec.calls == [want], (wide, ctl, border)
    # an object built without the attribute (older callers of __new__) asks for no border
    bd = object.__new__(BatchedDeviceNewton)
    bd.count, bd.wide_band, bd.band_ctl, bd._lib = 3, False, False, _lib
    rec = _RecordingLib()
    assert bd._create(rec, None, None) == 0 and rec.calls == [("pgf_batch_create", 3)]
