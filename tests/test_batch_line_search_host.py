"""The Globalized policy in the device batch, what needs no GPU (CPU): the keyword validation of
``BatchedDeviceNewton(..., line_search=True)``, which must come before any handle is built, and the
flag's value in the binding against the header's."""

import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _never(i):
    raise AssertionError("a problem was built before the keywords were checked")


def test_keywords_are_checked_before_any_handle_is_built():
    from pygradflow_amd.batched import BatchedDeviceNewton

    for kind in ("Simplified", "Full", "ActiveSet"):
        with pytest.raises(ValueError, match="Globalized"):
            BatchedDeviceNewton(_never, 2, kind, 1.0, 1.0, line_search=True)
    for kw in ("border", "wide_border", "band_ctl", "border_ctl", "ctl_refine"):
        with pytest.raises(ValueError, match=kw):
            BatchedDeviceNewton(_never, 2, "Globalized", 1.0, 1.0, line_search=True, **{kw: True})
        with pytest.raises(ValueError, match=kw):
            BatchedDeviceNewton(_never, 2, "Globalized", 1.0, 1.0, line_search=True, sequential=True, **{kw: True})
    for tol in (-1e-8, float("nan")):
        with pytest.raises(ValueError, match="newton_tol"):
            BatchedDeviceNewton(_never, 2, "Globalized", 1.0, 1.0, line_search=True, newton_tol=tol)


def test_without_the_keyword_the_refusal_of_a_globalized_device_batch_stays():
    from pygradflow_amd.batched import BatchedDeviceNewton

    with pytest.raises(NotImplementedError, match="Globalized: not in the device batch"):
        BatchedDeviceNewton(_never, 2, "Globalized", 1.0, 1.0)


def test_flag_value_matches_the_header():
    from pygradflow_amd import _lib

    text = open(os.path.join(REPO, "include", "pgf_hip.h")).read()
    values = dict(re.findall(r"^#define (PGF_BATCH_[A-Z_]+) (\d+)u", text, flags=re.M))
    assert int(values["PGF_BATCH_LINE_SEARCH"]) == _lib.BATCH_LINE_SEARCH == 64
    # one bit of its own
    others = [int(v) for k, v in values.items() if k != "PGF_BATCH_LINE_SEARCH"]
    assert all(_lib.BATCH_LINE_SEARCH & v == 0 for v in others) and len(others) == 6
    for name in ("pgf_batch_set_line_search", "pgf_batch_line_search_stats", "pgf_batch_debug_line_search_stats"):
        assert name in _lib.SIGNATURES
