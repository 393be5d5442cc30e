"""The two creation flags of the device-resident controller on band batches, PGF_BATCH_BORDER_CTL (a
bordered batch under the controller) and PGF_BATCH_CTL_REFINE (refinement inside its loop), and the
entry point pgf_batch_debug_ctl_refine_stats: what needs no GPU.  Declared, bound and exported, one
value everywhere and a bit of their own; the refusals that come before any handle is read;
BatchedDeviceNewton passes the bits it was asked for and no others."""

import ctypes as C
import inspect
import itertools
import os
import re

import numpy as np

from tests.test_band_batch_host import FLAGS, _RecordingLib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"BORDER_CTL": 16, "CTL_REFINE": 32}


def test_flags_are_declared_equal_and_disjoint():
    from pygradflow_amd import _lib

    header = open(os.path.join(REPO, "include", "pgf_hip.h")).read()
    assert sorted(FLAGS.values()) == [1, 2, 4, 8]
    for flag, value in NEW.items():
        m = re.search(r"#define\s+PGF_BATCH_%s\s+(\d+)u" % flag, header)
        assert m and int(m.group(1)) == getattr(_lib, "BATCH_" + flag) == value, flag
        assert all(value & v == 0 for v in FLAGS.values()), flag
    assert NEW["BORDER_CTL"] & NEW["CTL_REFINE"] == 0


def test_the_stats_symbol_is_declared_bound_and_exported():
    from pygradflow_amd import _lib

    name = "pgf_batch_debug_ctl_refine_stats"
    header = open(os.path.join(REPO, "include", "pgf_hip.h")).read()
    assert re.search(r"\b%s\s*\(" % name, header)
    assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)


def test_stats_of_no_batch_are_refused_and_leave_the_outputs_alone():
    from pygradflow_amd import _lib

    stats = _lib.load().pgf_batch_debug_ctl_refine_stats
    a = np.full(3, 7, dtype=np.int32)
    b = np.full(3, 9, dtype=np.int32)
    ip = C.POINTER(C.c_int)
    assert stats(None, a.ctypes.data_as(ip), b.ctypes.data_as(ip)) == _lib.PGF_INVALID
    assert stats(None, None, None) == _lib.PGF_INVALID
    assert list(a) == [7] * 3 and list(b) == [9] * 3


def test_create_ex_refuses_null_handles_under_every_subset_of_the_six_bits():
    from pygradflow_amd import _lib

    lib = _lib.load()
    out = C.c_void_p()
    none = (C.c_void_p * 2)(None, None)
    assert sum(FLAGS.values()) + sum(NEW.values()) == 63
    for flags in list(range(64)) + [64]:
        assert lib.pgf_batch_create_ex(none, 2, flags, C.byref(out)) == _lib.PGF_INVALID, flags
        assert lib.pgf_batch_create_ex(none, 0, flags, C.byref(out)) == _lib.PGF_INVALID, flags
        assert lib.pgf_batch_create_ex(None, 2, flags, C.byref(out)) == _lib.PGF_INVALID, flags
    assert not out.value


KEYWORDS = ("wide_band", "band_ctl", "border", "wide_border", "border_ctl", "ctl_refine")
BITS = dict(zip(KEYWORDS, (1, 2, 4, 8, 16, 32)))


def _created_with(attrs):
    from pygradflow_amd import _lib
    from pygradflow_amd.batched import BatchedDeviceNewton

    bd = object.__new__(BatchedDeviceNewton)
    bd.count, bd._lib = 3, _lib
    for name, value in attrs.items():
        setattr(bd, name, value)
    rec = _RecordingLib()
    assert bd._create(rec, None, None) == 0
    return rec.calls


def test_every_keyword_combination_maps_to_its_bits():
    """_create passes the attributes as they stand (the constructor derives wide_band and border from
    wide_border; the library refuses a bit without its companions): all 64 combinations."""
    from pygradflow_amd.batched import BatchedDeviceNewton

    for keyword in ("border_ctl", "ctl_refine"):
        assert inspect.signature(BatchedDeviceNewton.__init__).parameters[keyword].default is False
    for values in itertools.product((False, True), repeat=6):
        attrs = dict(zip(KEYWORDS, values))
        flags = sum(BITS[k] for k, v in attrs.items() if v)
        want = [("pgf_batch_create_ex", 3, flags) if flags else ("pgf_batch_create", 3)]
        assert _created_with(attrs) == want, attrs


def test_an_object_without_the_new_attributes_asks_for_neither_bit():
    assert _created_with(dict(wide_band=False)) == [("pgf_batch_create", 3)]
    assert _created_with(dict(wide_band=True, band_ctl=True, border=True, wide_border=True)) == \
        [("pgf_batch_create_ex", 3, 15)]
