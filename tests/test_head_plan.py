"""The unit list of the fused head (``k_chain_head``), walked on the host (CPU).

``pgf_debug_head_plan`` runs the same ``head_unit`` mapping the device workers run and counts,
per entry of K and of the panel V, how many units write it.  The first diagonal chain reads
K[0:256, 0:256] while the workers run, so that block must belong to the launch in front and to
no unit; everything else must be written exactly once.  (The driver fuses nothing for N <= 256;
the list is checked for those sizes all the same.)
"""

import ctypes as C

import numpy as np
import pytest

NI = (1, 8, 255, 256, 257, 263, 264, 300, 519, 768)
M = (0, 24, 70, 256)


def _plan(nI, m, condensed):
    from pygradflow_amd import _lib

    lib = _lib.load()
    N = nI if condensed else nI + m
    mp = (m + 31) // 32 * 32 if condensed else 0
    ku = np.zeros((N, N), dtype=np.int32)
    kh = np.zeros((N, N), dtype=np.int32)
    vu = np.zeros((nI + 1, max(mp, 1)), dtype=np.int32)
    nu = C.c_int(-1)
    ip = C.POINTER(C.c_int)
    rc = lib.pgf_debug_head_plan(
        nI, m, 1 if condensed else 0, ku.ctypes.data_as(ip), kh.ctypes.data_as(ip),
        vu.ctypes.data_as(ip) if mp else None, C.byref(nu))
    assert rc == 0
    return N, mp, ku, kh, vu[:, :mp], nu.value


@pytest.mark.parametrize("condensed", [True, False], ids=["condensed", "natural"])
@pytest.mark.parametrize("m", M)
@pytest.mark.parametrize("nI", NI)
def test_every_entry_is_written_exactly_once(nI, m, condensed):
    N, mp, ku, kh, vu, nunits = _plan(nI, m, condensed)
    i, j = np.indices((N, N))
    lower, upper = j <= i, j > i
    # nothing above the diagonal, by anything
    assert not ku[upper].any() and not kh[upper].any()
    first = lower & (i < 256)
    below = lower & (i >= 256)
    # the block the chain reads while the workers run: the launch in front, and no unit
    assert np.all(kh[first] == 1) and not ku[first].any()
    # the rest of the triangle: exactly one unit, and not the launch in front
    assert np.all(ku[below] == 1) and not kh[below].any()
    # V with its zero-padded columns and the tail row
    assert vu.shape == (nI + 1, mp)
    assert np.all(vu == 1)
    # the list is empty exactly when there are no rows below the first block and no panel
    assert (nunits == 0) == (N <= 256 and (mp == 0 or nI == 0))


def test_empty_list_without_rows_below_and_without_panel():
    for nI, m, condensed in ((256, 0, True), (200, 56, False), (1, 0, False), (256, 0, False)):
        assert _plan(nI, m, condensed)[5] == 0
