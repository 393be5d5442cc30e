#!/usr/bin/env python3
"""The pivoted LU (csrc/pgf_lu.hip) through HipLinearSolver(symmetric=False) on the GPU, against
tests/lu_util.py: textbook backward-error bounds, LAPACK's pivot sequence, families with an exact
factorisation.  Run in a child process by tests/test_lu_gpu.py: PGF_LU_PANEL (1: every panel
through the streaming k_lu_panel instead of k_lu_panel_reg<R>) is read once per process.

usage: check_lu.py GROUP
  small        Gaussian N = 1 ... 1057 on both sides of every group / panel / solve-block /
               gemv-workgroup boundary and of R = 1 | 2
  exact        wilkinson(100), wilkinson(1000), tie_family and pivot_family at N = 90 and 1300:
               factor and perm bit for bit
  edge         scaling by 2^+-500, the same matrix twice, exact zero pivots in every position,
               NaN / Inf entries (LinearSolverError, and the process goes on), lda > N
  large0..2    Gaussian N = 2048 ... 5153: panels of R = 2 ... 5 rows per thread and the streaming
               kernel (which panels stream is PGF_LU_PANEL's business, the script takes any size)
  large_exact  tie_family and pivot_family at N = 4200: ties and pivots across five register slots

Every factorisation's panel counts (lu_debug) are checked against what the environment asks for
and printed as "panels <N> <reg> <streamed>"; the largest error / bound ratio of each check as
"ratio <check> <value> N=<where>".  Prints "lu ok" at the end."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pygradflow_amd as pgf  # noqa: E402
from pygradflow_amd import _lib  # noqa: E402
from tests import lu_util as LU  # noqa: E402

STREAMING_ONLY = os.environ.get("PGF_LU_PANEL") == "1"
worst = {}


def note(ratios, N):
    for k, v in ratios.items():
        if v >= worst.get(k, (-1.0, 0))[0]:
            worst[k] = (v, N)


def factorise(A):
    """(solver, F, perm) with the panel counts checked."""
    N = A.shape[0]
    sv = pgf.HipLinearSolver(A, symmetric=False)
    perm, reg, streamed = sv.lu_debug()
    print(f"panels {N} {reg} {streamed}", flush=True)
    assert (reg, streamed) == LU.expected_panels(N, STREAMING_ONLY), (N, reg, streamed)
    return sv, sv.factor_matrix(), perm


def gaussian_case(N):
    t0 = time.time()
    A = LU.gaussian(N)
    lu_ref, perm_ref = LU.scipy_lu(A)
    gap = LU.pivot_gap(lu_ref)
    assert gap >= LU.GAP_MIN, (N, gap)
    sv, F, perm = factorise(A)
    try:
        ratios = LU.check_lu(A, F, perm, LU.rhs_set(N), lambda b, tr: sv.solve(b, trans=tr))
    finally:
        sv.close()
    note(ratios, N)
    assert np.array_equal(perm, perm_ref), (N, int(np.count_nonzero(perm != perm_ref)), gap)
    print(f"gaussian {N}: gap {gap:.2e} " + " ".join(f"{k} {v:.2e}" for k, v in ratios.items())
          + f" ({time.time() - t0:.1f} s)", flush=True)


def exact_case(name, case):
    A, F_want, perm_want = case
    sv, F, perm = factorise(A)
    sv.close()
    assert np.array_equal(perm, perm_want), (name, np.flatnonzero(perm != perm_want)[:8])
    bad = np.argwhere(F != F_want)
    assert bad.size == 0, (name, len(bad), bad[:8].tolist())
    print(f"exact {name}: ok", flush=True)


def good_factorisation():
    A = LU.gaussian(33)
    sv, F, perm = factorise(A)
    sv.close()
    assert np.array_equal(perm, LU.scipy_lu(A)[1])
    LU.check_lu(A, F, perm)


def must_fail(name, A):
    """A status return, not a fault: LinearSolverError, then a good factorisation."""
    try:
        pgf.HipLinearSolver(A, symmetric=False).close()
    except pgf.LinearSolverError:
        pass
    else:
        raise AssertionError(f"{name}: no LinearSolverError")
    good_factorisation()
    print(f"error {name}: ok", flush=True)


def raw_factor(buf, N, lda):
    """(F, perm) through the C ABI with a leading dimension of its own."""
    lib = _lib.load()
    h = C.c_void_p()
    _lib.check(lib.pgf_ls_create_dense(N, _lib.dptr(buf), lda, 0, 0, C.byref(h)), None, "pgf_ls_create_dense")
    try:
        F = np.zeros((N, N))
        perm = np.zeros(N, dtype=np.intc)
        _lib.check(lib.pgf_ls_get_factor(h, _lib.dptr(F), N), None, "pgf_ls_get_factor")
        _lib.check(lib.pgf_ls_debug_lu(h, perm.ctypes.data_as(C.POINTER(C.c_int)), None, None), None,
                   "pgf_ls_debug_lu")
    finally:
        lib.pgf_ls_destroy(h)
    return F, perm


def group_small():
    for N in LU.GAUSS_SMALL:
        gaussian_case(N)


def group_exact():
    exact_case("wilkinson100", LU.wilkinson(100))
    exact_case("wilkinson1000", LU.wilkinson(1000))
    for N, far in ((90, LU.FAR_SMALL), (1300, LU.FAR_MID)):
        exact_case(f"tie{N}", LU.tie_family(N, far, seed=N))
        exact_case(f"pivot{N}", LU.pivot_family(N, far, seed=N + 1))


def group_edge():
    # scaling by a power of two changes no pivot and no rounding
    for N in (257, 1057):
        A = LU.gaussian(N)
        sv, F, perm = factorise(A)
        sv.close()
        sv, F2, perm2 = factorise(A)  # the same matrix twice
        sv.close()
        assert np.array_equal(F, F2) and np.array_equal(perm, perm2), N
        for e in (500, -500):
            sv, Fs, perms = factorise(A * 2.0 ** e)
            sv.close()
            assert np.array_equal(perms, perm), (N, e)
            assert np.array_equal(np.tril(Fs, -1), np.tril(F, -1)), (N, e)
            assert np.array_equal(np.triu(Fs), np.triu(F) * 2.0 ** e), (N, e)
        print(f"scaling {N}: ok", flush=True)
    # exact zero pivots: first column, end of the first group, later groups, later panels, and the
    # last panel (4 columns wide, one group of 4)
    for c in (0, 7, 8, 31, 32, 33, 96, 99):
        must_fail(f"singular c={c}", LU.singular_family(100, LU.FAR_SMALL, seed=50 + c, c=c))
    for name, N, i, j, v in (("nan100", 100, 70, 40, np.nan), ("inf100", 100, 70, 40, np.inf),
                             ("nan1100", 1100, 1030, 5, np.nan)):
        A = LU.gaussian(N)
        A[i, j] = v
        must_fail(name, A)
    # lda > N: the padding is never read
    N, lda = 65, 80
    A = LU.gaussian(N)
    buf = np.full((N, lda), np.nan)
    buf[:, :N] = A
    F_pad, perm_pad = raw_factor(buf, N, lda)
    F, perm = raw_factor(np.ascontiguousarray(A), N, N)
    assert np.array_equal(perm_pad, perm) and np.array_equal(F_pad, F)
    assert np.array_equal(perm, LU.scipy_lu(A)[1])
    print("lda: ok", flush=True)


def group_large(sizes):
    for N in sizes:
        gaussian_case(N)


def group_large_exact():
    exact_case("tie4200", LU.tie_family(4200, LU.FAR_LARGE, seed=4200))
    exact_case("pivot4200", LU.pivot_family(4200, LU.FAR_LARGE, seed=4201))


GROUPS = {
    "small": group_small,
    "exact": group_exact,
    "edge": group_edge,
    "large0": lambda: group_large(LU.GAUSS_LARGE[:3]),
    "large1": lambda: group_large(LU.GAUSS_LARGE[3:5]),
    "large2": lambda: group_large(LU.GAUSS_LARGE[5:]),
    "large_exact": group_large_exact,
}

if __name__ == "__main__":
    GROUPS[sys.argv[1]]()
    for k, (v, N) in sorted(worst.items()):
        print(f"ratio {k} {v:.3e} N={N}", flush=True)
    print("lu ok", flush=True)
