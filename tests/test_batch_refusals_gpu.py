"""What a DENSE device batch refuses at the C ABI: every return code and the text beside it, and
which of two applicable refusals is the one reported (the banded ones:
test_band_batch_gpu.py::test_what_a_band_batch_refuses).  Behind the refusals one Full step of the
batch agrees with its two instances stepped one by one to the bar of tools/check_batch.py: a
refused call has left the batch as it was."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, M = 8, 2
NAN = float("nan")
PENDING = b"pgf_batch_sync the previous step first"
OUTER_FIRST = b"pgf_batch_advance_outer first"
CTL_FIRST = b"pgf_batch_ctl_init first"
NO_MASK = b"no active set: pgf_batch_update_active_set first"
REFACTOR = b"batch: PGF_STEP_REFACTOR needs PGF_STEP_RECOMPUTE_MASK"
SHARE = b"batch: instances must share n, m and the device"
SYMMETRIC = b"batch: the Symmetric formulation only"
NOT_SET = b"batch: pgf_set_bounds, pgf_qp_set_problem, pgf_qp_set_point first"
STEP_PENDING = b"batch: a step is pending"
LS_ALONE = (b"batch: PGF_BATCH_LINE_SEARCH goes alone or with PGF_BATCH_WIDE_BAND (no border, no "
            b"device-resident controller)")
LS_SINGLE = b"batch: PGF_STEP_LINE_SEARCH is served by single handles only"
LS_HOST = b"batch: PGF_STEP_LINE_SEARCH is for host-driven steps (pgf_batch_step_async)"
NO_LS_FLAG = b"batch: created without PGF_BATCH_LINE_SEARCH"


def make(i, n=N):
    from pygradflow_amd import problems

    return problems.dense_qp(n, M, seed=100 + i, boxed_frac=0.5, box=0.05)


def test_what_a_dense_batch_refuses(pgf):
    from pygradflow_amd import _lib
    from pygradflow_amd.batched import BatchedDeviceNewton
    from pygradflow_amd.newton import DeviceNewton

    lib = _lib.load()
    OK, INVALID, NOT_READY = _lib.PGF_OK, _lib.PGF_INVALID, _lib.PGF_NOT_READY
    FULL = _lib.STEP_RECOMPUTE_MASK | _lib.STEP_REFACTOR

    def newton(i, n=N, **kw):
        return DeviceNewton(make(i, n), "Full", np.zeros(n), np.zeros(M), 1.0, 1.0, **kw)

    good = [newton(0), newton(1)]
    busy, other_n, unsym = newton(2), newton(3, n=N + 1), newton(4, step_solver_type="Standard")
    bare = C.c_void_p()
    assert lib.pgf_create(N, M, 0, 0, C.byref(bare)) == OK
    h = [s._hd.h.value for s in good]

    def create(handles, flags=None, count=None):
        """(return code, the batch) of pgf_batch_create / _create_ex; no handle's message changes
        but the one the caller names afterwards."""
        arr = (C.c_void_p * max(1, len(handles)))(*handles)
        out = C.c_void_p()
        count = len(handles) if count is None else count
        if flags is None:
            return lib.pgf_batch_create(arr, count, C.byref(out)), out
        return lib.pgf_batch_create_ex(arr, count, flags, C.byref(out)), out

    def refused(handles, code, flags=None, count=None, at=None, msg=None):
        """the create is refused with `code`; `msg` is left on the handle `at` and on no other"""
        real = [x for x in handles if x]
        before = [lib.pgf_last_error(x) for x in real]
        rc, out = create(handles, flags, count)
        assert rc == code and not out.value, (rc, code, msg)
        for x, was in zip(real, before):
            now = lib.pgf_last_error(x)
            assert now == (msg if x == at else was), (now, msg, was)

    # ---- count 0, a null handle, a null result
    refused(h, INVALID, count=0)
    refused([h[0], None], INVALID)
    refused([None, h[1]], INVALID)
    assert lib.pgf_batch_create(None, 2, C.byref(C.c_void_p())) == INVALID
    assert lib.pgf_batch_create((C.c_void_p * 2)(*h), 2, None) == INVALID
    # ---- unknown flag bits; the three flags that need companions, without them
    refused(h, INVALID, flags=128)
    refused(h, INVALID, flags=1 << 31)
    for flags in (_lib.BATCH_WIDE_BORDER, _lib.BATCH_WIDE_BORDER | _lib.BATCH_BORDER,
                  _lib.BATCH_WIDE_BORDER | _lib.BATCH_WIDE_BAND,
                  _lib.BATCH_BORDER_CTL, _lib.BATCH_BORDER_CTL | _lib.BATCH_BORDER,
                  _lib.BATCH_BORDER_CTL | _lib.BATCH_BAND_CTL, _lib.BATCH_CTL_REFINE,
                  _lib.BATCH_CTL_REFINE | _lib.BATCH_BORDER):
        refused(h, INVALID, flags=flags)
    # (the line search's own refusal comes first, and names its reason on the first handle)
    refused(h, INVALID, flags=_lib.BATCH_LINE_SEARCH | _lib.BATCH_BORDER, at=h[0], msg=LS_ALONE)
    refused(h, INVALID, flags=_lib.BATCH_LINE_SEARCH | _lib.BATCH_CTL_REFINE, at=h[0], msg=LS_ALONE)
    # ---- what every handle must be: the reason on the FIRST handle that misses, its first miss
    hn, hu, hb = other_n._hd.h.value, unsym._hd.h.value, busy._hd.h.value
    refused([h[0], hn], INVALID, at=hn, msg=SHARE)
    refused([h[0], hu], INVALID, at=hu, msg=SYMMETRIC)
    refused([h[0], hu, hn], INVALID, at=hu, msg=SYMMETRIC)
    refused([h[0], hn, hu], INVALID, at=hn, msg=SHARE)
    refused([h[0], bare.value], NOT_READY, at=bare.value, msg=NOT_SET)
    refused([h[0], bare.value], NOT_READY, flags=_lib.BATCH_LINE_SEARCH, at=bare.value, msg=NOT_SET)
    refused([h[0], bare.value, hu], NOT_READY, at=bare.value, msg=NOT_SET)
    busy.step_async()
    refused([h[0], hb], NOT_READY, at=hb, msg=STEP_PENDING)
    refused([hu, hb], INVALID, at=hu, msg=SYMMETRIC)
    busy.sync()

    # ---- a good batch: the order its calls must come in
    rc, b = create(h)
    assert rc == OK and b.value
    err = lambda: lib.pgf_batch_last_error(b)  # noqa: E731
    ip = C.POINTER(C.c_int)
    out2, out8 = np.zeros(2), np.zeros(8)
    x, y, mk = np.zeros((2, N)), np.zeros((2, M)), np.zeros((2, N), dtype=np.uint8)
    status, n_neg, diff = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32), np.zeros(2)
    ones, zeros = np.ones(2), np.zeros(2)
    acc0 = np.array([1, 0], dtype=np.uint8)
    params = np.array([1e-8, 0.5, 1e-12, 2.0, 0.5, 0.2, 0.05, 0.5])

    def sync():
        return lib.pgf_batch_sync(b, status.ctypes.data_as(ip), n_neg.ctypes.data_as(ip), _lib.dptr(diff))

    # before the first outer step
    assert lib.pgf_batch_step_async(b, FULL, NAN) == NOT_READY and err() == OUTER_FIRST
    assert lib.pgf_batch_step_async(b, 0, NAN) == NOT_READY and err() == OUTER_FIRST  # (not: no mask)
    assert lib.pgf_batch_update_active_set(b, NAN) == NOT_READY and err() == OUTER_FIRST
    assert lib.pgf_batch_residual_norms(b, _lib.dptr(out2), None) == NOT_READY and err() == OUTER_FIRST
    assert lib.pgf_batch_measures(b, 1e-8, _lib.dptr(out8)) == NOT_READY and err() == OUTER_FIRST
    assert lib.pgf_batch_measures(b, 1e-8, None) == INVALID
    assert lib.pgf_batch_get_masks(b, _lib.u8ptr(mk)) == NOT_READY and err() == b"no active set"
    assert sync() == NOT_READY and err() == b"no step pending"
    assert lib.pgf_batch_advance_outer_each(b, _lib.dptr(np.array([1.0, 0.0])), _lib.dptr(ones), None) == INVALID
    assert err() == b"dt and rho must be positive"
    assert lib.pgf_batch_advance_outer_each(b, _lib.dptr(ones), _lib.dptr(np.array([-1.0, 1.0])), None) == INVALID
    assert err() == b"dt and rho must be positive"
    assert lib.pgf_batch_advance_outer_each(b, _lib.dptr(ones), _lib.dptr(ones), _lib.u8ptr(acc0)) == NOT_READY
    assert err() == b"nothing to go back to before the first outer step"
    # (both apply: the scalars are looked at first)
    assert lib.pgf_batch_advance_outer_each(b, _lib.dptr(zeros), _lib.dptr(ones), _lib.u8ptr(acc0)) == INVALID
    assert err() == b"dt and rho must be positive"
    assert lib.pgf_batch_advance_outer_each(b, None, _lib.dptr(ones), None) == INVALID
    assert lib.pgf_batch_ctl_iterate(b, FULL, NAN, 1) == NOT_READY and err() == CTL_FIRST
    assert lib.pgf_batch_ctl_read(b, None, None, None, 0) == NOT_READY and err() == CTL_FIRST
    assert lib.pgf_batch_ctl_iterate(b, FULL | _lib.STEP_LINE_SEARCH, NAN, 1) == INVALID and err() == LS_HOST
    assert lib.pgf_batch_ctl_iterate(b, FULL, NAN, -1) == INVALID
    assert lib.pgf_batch_ctl_init(b, 0.0, 1.0, _lib.dptr(params), 2) == INVALID
    assert lib.pgf_batch_ctl_init(b, 1.0, 1.0, _lib.dptr(params), 0) == INVALID
    assert lib.pgf_batch_set_line_search(b, 1e-8) == INVALID and err() == NO_LS_FLAG
    assert lib.pgf_batch_line_search_stats(b, None, None, None, None, None) == INVALID and err() == NO_LS_FLAG

    assert lib.pgf_batch_advance_outer(b, 1.0, 1.0) == OK
    # a back-solve step without a mask; with the refactor bit besides, the missing mask is reported
    assert lib.pgf_batch_step_async(b, 0, NAN) == NOT_READY and err() == NO_MASK
    assert lib.pgf_batch_step_async(b, _lib.STEP_REFACTOR, NAN) == NOT_READY and err() == NO_MASK
    # the line-search bit on a batch without the flag: before anything else about the policy
    assert lib.pgf_batch_step_async(b, FULL | _lib.STEP_LINE_SEARCH, NAN) == INVALID and err() == LS_SINGLE
    assert lib.pgf_batch_step_async(b, _lib.STEP_LINE_SEARCH, NAN) == INVALID and err() == LS_SINGLE
    assert lib.pgf_batch_update_active_set(b, NAN) == OK
    assert lib.pgf_batch_step_async(b, _lib.STEP_REFACTOR, NAN) == INVALID and err() == REFACTOR
    # the controller's log
    bad = params.copy()
    bad[7] = 0.0
    assert lib.pgf_batch_ctl_init(b, 1.0, 1.0, _lib.dptr(bad), 2) == INVALID
    assert err() == b"theta_ref must be positive"
    assert lib.pgf_batch_ctl_init(b, 1.0, 1.0, _lib.dptr(params), 2) == OK
    more = b"more iterations than pgf_batch_ctl_init reserved a log for"
    assert lib.pgf_batch_ctl_iterate(b, FULL, NAN, 3) == INVALID and err() == more
    assert lib.pgf_batch_ctl_iterate(b, _lib.STEP_REFACTOR, NAN, 3) == INVALID and err() == more
    assert lib.pgf_batch_ctl_iterate(b, _lib.STEP_REFACTOR, NAN, 2) == INVALID and err() == REFACTOR

    # ---- while a step is pending; that step is the one compared below
    assert lib.pgf_batch_step_async(b, FULL, NAN) == OK
    calls = [
        lambda: lib.pgf_batch_advance_outer(b, 1.0, 1.0),
        lambda: lib.pgf_batch_advance_outer_each(b, _lib.dptr(ones), _lib.dptr(ones), None),
        lambda: lib.pgf_batch_advance_outer_each(b, _lib.dptr(zeros), _lib.dptr(ones), None),
        lambda: lib.pgf_batch_set_frozen(b, None),
        lambda: lib.pgf_batch_update_active_set(b, NAN),
        lambda: lib.pgf_batch_step_async(b, FULL, NAN),
        lambda: lib.pgf_batch_step_async(b, _lib.STEP_REFACTOR, NAN),
        lambda: lib.pgf_batch_ctl_init(b, 1.0, 1.0, _lib.dptr(params), 2),
        lambda: lib.pgf_batch_ctl_iterate(b, FULL, NAN, 1),
        lambda: lib.pgf_batch_ctl_iterate(b, FULL, NAN, 3),
        lambda: lib.pgf_batch_profile_read(b, None, None, None),
        lambda: lib.pgf_batch_residual_norms(b, _lib.dptr(out2), None),
        lambda: lib.pgf_batch_measures(b, 1e-8, _lib.dptr(out8)),
        lambda: lib.pgf_batch_get_points(b, _lib.dptr(x), _lib.dptr(y)),
        lambda: lib.pgf_batch_get_masks(b, _lib.u8ptr(mk)),
    ]
    for k, call in enumerate(calls):
        assert call() == NOT_READY and err() == PENDING, k
    assert lib.pgf_batch_set_line_search(b, 1e-8) == INVALID and err() == NO_LS_FLAG
    assert sync() == OK
    assert sync() == NOT_READY and err() == b"no step pending"

    # ---- the step the refusals surrounded, against the two instances one by one
    norms = np.zeros(2)
    assert not status.any()
    assert lib.pgf_batch_residual_norms(b, _lib.dptr(norms), None) == OK
    assert lib.pgf_batch_get_points(b, _lib.dptr(x), _lib.dptr(y)) == OK
    ref = BatchedDeviceNewton(make, 2, "Full", 1.0, 1.0, sequential=True)
    rs, rn, rd = ref.step_local()
    rnorms = ref.residual_norms_local()
    xr, yr = ref.points()
    assert not rs.any() and np.array_equal(rn, n_neg)
    assert np.allclose(norms, rnorms, rtol=1e-9, atol=1e-12), (norms, rnorms)
    assert np.allclose(diff, rd, rtol=1e-9, atol=1e-12), (diff, rd)
    e = max(np.max(np.abs(x - xr)) / max(1.0, np.max(np.abs(xr))),
            np.max(np.abs(y - yr)) / max(1.0, np.max(np.abs(yr))))
    assert np.max(np.abs(xr)) > 0.0 and e <= 1e-11, e
    ref.close()
    assert lib.pgf_batch_destroy(b) == OK
    for s in good + [busy, other_n, unsym]:
        s.close()
    assert lib.pgf_destroy(bare) == OK
