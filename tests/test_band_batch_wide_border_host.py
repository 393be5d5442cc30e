"""A border on a wide remainder in a band batch, what needs no GPU: PGF_BATCH_WIDE_BORDER has one
value everywhere and shares no bit with the other creation flags, pgf_batch_create_ex refuses what
comes before any device call, and BatchedDeviceNewton's ``wide_border`` asks for the three bits that
go together."""

import ctypes as C
import inspect
import os
import re


def test_the_flag_has_one_value_and_its_own_bit():
    from pygradflow_amd import _lib

    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(repo, "include", "pgf_hip.h")).read()
    m = re.search(r"#define\s+PGF_BATCH_WIDE_BORDER\s+(\d+)u", header)
    assert m and int(m.group(1)) == _lib.BATCH_WIDE_BORDER == 8
    assert _lib.BATCH_WIDE_BORDER & (_lib.BATCH_WIDE_BAND | _lib.BATCH_BAND_CTL | _lib.BATCH_BORDER) == 0


def test_create_ex_refuses_null_handles_under_the_new_bit_and_the_next():
    from pygradflow_amd import _lib

    lib = _lib.load()
    out = C.c_void_p()
    none = (C.c_void_p * 2)(None, None)
    for flags in list(range(8, 16)) + [16]:  # the bit alone, with every subset of the others, the next unknown one
        assert lib.pgf_batch_create_ex(none, 2, flags, C.byref(out)) == _lib.PGF_INVALID, flags
        assert lib.pgf_batch_create_ex(None, 2, flags, C.byref(out)) == _lib.PGF_INVALID, flags
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


def test_the_keyword_exists_and_asks_for_the_three_bits():
    from pygradflow_amd import _lib
    from pygradflow_amd.batched import BatchedDeviceNewton

    assert inspect.signature(BatchedDeviceNewton.__init__).parameters["wide_border"].default is False
    # (the constructor needs a device for its norms: the GPU tests see what it derives from the keyword)
    for wide, ctl, border, wb, want in ((True, False, True, True, ("pgf_batch_create_ex", 3, 8 | 4 | 1)),
                                        (True, True, True, True, ("pgf_batch_create_ex", 3, 15)),
                                        (True, False, True, False, ("pgf_batch_create_ex", 3, 4 | 1)),
                                        (False, False, False, False, ("pgf_batch_create", 3))):
        bd = object.__new__(BatchedDeviceNewton)
        bd.count, bd.wide_band, bd.band_ctl, bd.border, bd.wide_border, bd._lib = 3, wide, ctl, border, wb, _lib
        rec = _RecordingLib()
        assert bd._create(rec, None, None) == 0
        assert rec.calls == [want], (wide, ctl, border, wb)
    # an object built without the attribute asks for no wide border
    bd = object.__new__(BatchedDeviceNewton)
    bd.count, bd.wide_band, bd.band_ctl, bd.border, bd._lib = 3, True, False, True, _lib
    rec = _RecordingLib()
    assert bd._create(rec, None, None) == 0 and rec.calls == [("pgf_batch_create_ex", 3, 5)]
