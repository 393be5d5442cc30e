"""The inputs and the checker of the pivoted LU's GPU tests (tests/lu_util.py), proven on the CPU
before a GPU sees them: the exact families really have the factorisation they claim, under more
than one order of the operations; no Gaussian case has a near-tie that would let two correct
implementations pick different pivots; ``check_lu`` accepts LAPACK's factors and solves, and
rejects each corruption a wrong kernel could produce.  A checker that cannot fail is not a test."""

from fractions import Fraction

import numpy as np
import pytest
import scipy.linalg as sla

from tests import lu_util as LU


def _families(N, far):
    return [("tie", LU.tie_family(N, far, seed=N)), ("pivot", LU.pivot_family(N, far, seed=N + 1))]


# ---- the exact families ----------------------------------------------------------------------
def test_exact_families_plain_lu_equals_fraction_lu():
    """N = 90: a right-looking LU in doubles and the same LU in exact rationals return the
    construction bit for bit, pivots included."""
    for name, (A, F, perm) in _families(90, LU.FAR_SMALL) + [("wilkinson", LU.wilkinson(90))]:
        Fd, pd = LU.plain_lu(A)
        Ff, pf = LU.plain_lu([[Fraction(v) for v in row] for row in A], dtype=object)
        assert np.array_equal(pd, perm) and np.array_equal(pf, perm), name
        assert np.array_equal(Fd, F), name
        assert np.array_equal(Ff.astype(np.float64), F) and all(Fraction(a) == b for a, b in zip(F.ravel(), Ff.ravel())), name
        assert np.abs(F).max() <= (2.0 ** 89 if name == "wilkinson" else 4.0)
        if name == "pivot":
            assert not np.array_equal(perm, np.arange(90))
            assert np.array_equal(A[perm], np.tril(F, -1) @ np.triu(F) + np.triu(F))


@pytest.mark.parametrize("N,far", [(1300, LU.FAR_MID), (4200, LU.FAR_LARGE)])
def test_exact_families_scipy_equals_construction(N, far):
    """LAPACK's blocked, recursive dgetrf (another order of the operations again) returns the
    construction bit for bit: 1300 is the size of the tests' both processes, 4200 the one that
    puts ties and pivots across all five register slots."""
    for name, (A, F, perm) in _families(N, far):
        lu, p = LU.scipy_lu(A)
        assert np.array_equal(p, perm), name
        assert np.array_equal(lu, F), name
        assert np.abs(F).max() <= 4.0
        # every distance of `far' that fits is present
        low = np.tril(F, -1)
        for d in far:
            assert np.count_nonzero(np.diagonal(low, -d)) > (N - d) // 4, (name, d)


@pytest.mark.parametrize("N", [100, 1000])
def test_wilkinson_scipy_equals_construction(N):
    A, F, perm = LU.wilkinson(N)
    lu, p = LU.scipy_lu(A)
    assert np.array_equal(p, perm) and np.array_equal(lu, F)
    assert np.isfinite(F).all() and F[N - 1, N - 1] == 2.0 ** (N - 1)


@pytest.mark.parametrize("c", [0, 7, 8, 31, 32, 33, 96, 99])
def test_singular_family_has_its_zero_column_at_c(c):
    """Column c is exactly zero at and below the diagonal after c clean eliminations, not before."""
    A = LU.singular_family(100, LU.FAR_SMALL, seed=50 + c, c=c)
    F = np.array(A)
    for k in range(c):
        p = k + int(np.argmax(np.abs(F[k:, k])))
        assert F[p, k] != 0.0, k
        F[[k, p]] = F[[p, k]]
        F[k + 1:, k] /= F[k, k]
        F[k + 1:, k + 1:] -= np.outer(F[k + 1:, k], F[k, k + 1:])
    assert not F[c:, c].any()
    assert np.isfinite(F).all()


# ---- the Gaussian cases ------------------------------------------------------------------------
_REF = {}


def _ref(N):
    """(A, lu, perm) of a Gaussian case: computed once, shared, never written to (the large
    sizes, used once, are not kept)."""
    if N in _REF:
        return _REF[N]
    A = LU.gaussian(N)
    lu, perm = LU.scipy_lu(A)
    for a in (A, lu, perm):
        a.setflags(write=False)
    if N <= LU.FULL_CHECK_MAX:
        _REF[N] = (A, lu, perm)
    return A, lu, perm


@pytest.mark.parametrize("N", LU.GAUSS_SMALL + LU.GAUSS_LARGE + (100, 1100))
def test_gaussian_cases_have_no_near_tie(N):
    """gap >= 1e-8 wherever the tests compare a pivot sequence with LAPACK's (two CPU orders of
    the operations differ by <= 2e-11 in F at N = 1300)."""
    gap = LU.pivot_gap(_ref(N)[1])
    print(f"N={N}: pivot gap {gap:.3e}")
    assert gap >= LU.GAP_MIN


def test_piv_to_perm_is_the_row_order():
    A, lu, perm = _ref(257)
    P, L, U = sla.lu(A)  # A = P L U
    assert np.array_equal(A[perm], P.T @ A)


# ---- the checker ------------------------------------------------------------------------------
def _scipy_solve(A, lu, perm):
    piv = sla.lu_factor(A, check_finite=False)[1]
    return lambda b, tr: sla.lu_solve((lu, piv), b, trans=1 if tr else 0, check_finite=False)


@pytest.mark.parametrize("N", [33, 257, 1025])
def test_check_lu_accepts_lapack(N):
    A, lu, perm = _ref(N)
    ratios = LU.check_lu(A, lu, perm, LU.rhs_set(N), _scipy_solve(A, lu, perm))
    print(f"N={N}: error / bound {ratios}")
    assert set(ratios) == {"factor", "solve", "solve_trans"}
    assert all(0.0 < r <= 1.0 for r in ratios.values())
    probe = LU.check_lu(A, lu, perm, full=False)
    assert set(probe) == {"factor_probe"} and 0.0 < probe["factor_probe"] <= 1.0


def test_check_lu_accepts_the_exact_families():
    for name, (A, F, perm) in _families(90, LU.FAR_SMALL):
        assert LU.check_lu(A, F, perm)["factor"] == 0.0, name


@pytest.mark.parametrize("full", [True, False])
@pytest.mark.parametrize("N", [33, 257, 1025])
def test_check_lu_rejects_a_corrupted_factor(N, full):
    A, lu, perm = _ref(N)
    LU.check_lu(A, lu, perm, full=full)
    i = N // 2
    # one entry of U changed by 1e-9 relative
    bad = np.array(lu)
    bad[i, i] *= 1.0 + 1e-9
    with pytest.raises(AssertionError, match="gamma_N"):
        LU.check_lu(A, bad, perm, full=full)
    # one multiplier's sign flipped (the largest of a column in the middle)
    bad = np.array(lu)
    r = i + 1 + int(np.argmax(np.abs(lu[i + 1:, i])))
    bad[r, i] = -bad[r, i]
    with pytest.raises(AssertionError, match="gamma_N"):
        LU.check_lu(A, bad, perm, full=full)
    # two entries of perm exchanged
    bad = np.array(perm)
    bad[[1, N - 2]] = bad[[N - 2, 1]]
    with pytest.raises(AssertionError, match="gamma_N"):
        LU.check_lu(A, lu, bad, full=full)
    # not a permutation; a multiplier above 1; a NaN
    bad = np.array(perm)
    bad[0] = bad[1]
    with pytest.raises(AssertionError, match="permutation"):
        LU.check_lu(A, lu, bad, full=full)
    bad = np.array(lu)
    bad[N - 1, 0] = 1.0 + 2.0 ** -52
    with pytest.raises(AssertionError, match="multiplier"):
        LU.check_lu(A, bad, perm, full=full)
    bad = np.array(lu)
    bad[0, N - 1] = np.nan
    with pytest.raises(AssertionError, match="finite"):
        LU.check_lu(A, bad, perm, full=full)


@pytest.mark.parametrize("N", [33, 257, 1025])
def test_check_lu_rejects_a_corrupted_solve(N):
    A, lu, perm = _ref(N)
    good = _scipy_solve(A, lu, perm)
    rhs = LU.rhs_set(N)[:1]

    def one_off(b, tr):  # one component off by 1e-8 (relative)
        x = np.array(good(b, tr))
        x[int(np.argmax(np.abs(x)))] *= 1.0 + 1e-8
        return x

    for trans in ((False,), (True,)):
        LU.check_lu(A, lu, perm, rhs, good, trans=trans)
        with pytest.raises(AssertionError, match="rhs 0"):
            LU.check_lu(A, lu, perm, rhs, one_off, trans=trans)
        # the transposed solution handed in as the plain one, and the other way round
        with pytest.raises(AssertionError, match="rhs 0"):
            LU.check_lu(A, lu, perm, rhs, lambda b, tr: good(b, not tr), trans=trans)
    # the solve that forgets the permutation
    with pytest.raises(AssertionError, match="rhs 0"):
        LU.check_lu(A, lu, perm, rhs, lambda b, tr: good(b[perm], tr), trans=(False,))
    with pytest.raises(AssertionError, match="rhs 0"):
        LU.check_solves_with_reference_factor(A, rhs, one_off)
    assert set(LU.check_solves_with_reference_factor(A, rhs, good)) == {"solve", "solve_trans"}


def test_expected_panels():
    assert LU.expected_panels(1, False) == (1, 0)
    assert LU.expected_panels(100, False) == (4, 0) and LU.expected_panels(100, True) == (0, 4)
    assert LU.expected_panels(5120, False) == (160, 0)
    assert LU.expected_panels(5121, False) == (160, 1)
    assert LU.expected_panels(5153, False) == (160, 2)
    assert LU.expected_panels(5153, True) == (0, 162)
