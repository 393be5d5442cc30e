"""The bars of band_batch_util.same_step, held in place on the host: two fake batches of 3 instances
and 4 variables agree, or differ in exactly one thing."""

import numpy as np
import pytest

from tests.band_batch_util import same_step

PGF_SINGULAR = 3  # (any non-zero status)


class _FakeBatch:
    """What same_step reads of a batch: step_local(), masks(), points()."""

    def __init__(self):
        rng = np.random.default_rng(0)
        self.st = np.zeros(3, dtype=np.int32)
        self.nn = np.array([2, 2, 2], dtype=np.int32)
        self.df = rng.uniform(0.5, 2.0, 3)
        self.mk = rng.uniform(size=(3, 4)) < 0.5
        self.x, self.y = rng.standard_normal((3, 4)), rng.standard_normal((3, 2))

    def step_local(self):
        return self.st, self.nn, self.df

    def masks(self):
        return self.mk

    def points(self):
        return self.x, self.y


def _one_ulp(b):
    b.x[1, 2] = np.nextafter(b.x[1, 2], np.inf)


def _mask_byte(b):
    b.mk[2, 0] = not b.mk[2, 0]


def _status(b):
    b.st[1] = PGF_SINGULAR


def _n_neg(b):
    b.nn[0] += 1


def _step_length(b):
    b.df[2] *= 1.0 + 3e-14


def test_agreeing_batches_pass_and_return_status_and_inertia():
    a, b = _FakeBatch(), _FakeBatch()
    st, nn = same_step(a, b, "same")
    assert st is a.st and nn is a.nn
    b.df[2] *= 1.0 + 5e-15  # (within the 1e-14 of the step length)
    same_step(a, b, "same but for the order of a sum")


@pytest.mark.parametrize("ok", [True, False])
@pytest.mark.parametrize("change", [_one_ulp, _mask_byte, _status, _n_neg, _step_length])
def test_one_difference_is_an_error(change, ok):
    a, b = _FakeBatch(), _FakeBatch()
    change(b)
    with pytest.raises(AssertionError):
        same_step(a, b, change.__name__, ok=ok)
    with pytest.raises(AssertionError):
        same_step(b, a, change.__name__, ok=ok)


def test_a_status_both_report_is_an_error_only_under_ok():
    a, b = _FakeBatch(), _FakeBatch()
    _status(a)
    _status(b)
    with pytest.raises(AssertionError):
        same_step(a, b, "both singular")
    st, _ = same_step(a, b, "both singular", ok=False)
    assert list(st) == [0, PGF_SINGULAR, 0]


def test_inertia_of_an_instance_that_did_not_step_is_not_compared():
    a, b = _FakeBatch(), _FakeBatch()
    _status(a)
    _status(b)
    b.nn[1] += 1
    same_step(a, b, "bad instance", ok=False)
    b.nn[0] += 1  # (on a good instance it still is)
    with pytest.raises(AssertionError):
        same_step(a, b, "good instance", ok=False)
