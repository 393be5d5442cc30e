"""Wide bands in the banded device batch, what needs no GPU: the new entry points are declared, bound
and exported, the refusals that come before any device call, and BatchedDeviceNewton passes
PGF_BATCH_WIDE_BAND only when asked."""

import ctypes as C
import os
import re


def test_new_symbols_are_declared_bound_and_exported():
    from pygradflow_amd import _lib

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(repo, "include", "pgf_hip.h")).read()
    lib = _lib.load()
    for name in ("pgf_batch_create_ex", "pgf_batch_debug_band_wide_stats"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    m = re.search(r"#define\s+PGF_BATCH_WIDE_BAND\s+(\d+)u", header)
    assert m and int(m.group(1)) == _lib.BATCH_WIDE_BAND == 1
    lean = C.c_int(7)
    assert lib.pgf_batch_debug_band_wide_stats(None, None, None, C.byref(lean)) == _lib.PGF_INVALID
    assert lean.value == 7


def test_refusals_before_any_device_call():
    from pygradflow_amd import _lib

    lib = _lib.load()
    out = C.c_void_p()
    none = (C.c_void_p * 2)(None, None)
    for flags in (0, _lib.BATCH_WIDE_BAND, 2, 0x80000000):
        assert lib.pgf_batch_create_ex(none, 2, flags, C.byref(out)) == _lib.PGF_INVALID
        assert lib.pgf_batch_create_ex(none, 0, flags, C.byref(out)) == _lib.PGF_INVALID
        assert lib.pgf_batch_create_ex(None, 2, flags, C.byref(out)) == _lib.PGF_INVALID
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


def test_the_flag_is_passed_only_when_asked():
    import inspect

    from pygradflow_amd import _lib
    from pygradflow_amd.batched import BatchedDeviceNewton

    assert inspect.signature(BatchedDeviceNewton.__init__).parameters["wide_band"].default is False
    for wide, want in ((False, ("pgf_batch_create", 3)),
                       (True, ("pgf_batch_create_ex", 3, _lib.BATCH_WIDE_BAND))):
        bd = object.__new__(BatchedDeviceNewton)  # (the constructor needs a device for its norms)
        bd.count, bd.wide_band, bd._lib = 3, wide, _lib
        rec = _RecordingLib()
        assert bd._create(rec, None, None) == 0
        assert rec.calls == [want]
