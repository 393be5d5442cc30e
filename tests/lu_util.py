"""Inputs and the checker for the pivoted LU's tests (no GPU here: tests/test_lu_cases.py proves
both on the CPU, tests/check_lu.py and tests/test_lu_gpu.py use them on the device).

Inputs
  * families with an EXACT factorisation: every intermediate value of an LU with partial pivoting
    is a small dyadic rational, so the factor is the same bit for bit under any order of the
    operations (right-looking, left-looking, blocked, with or without FMAs) and the expected
    result is the construction itself.  They put exact ties (``tie_family``, ``wilkinson``: the
    smallest row must win) or one unique maximum (``pivot_family``) in rows chosen by ``far``:
    another lane, another wavefront or another register slot of the panel kernels.
  * Gaussian matrices, compared with LAPACK (``scipy.linalg.lu_factor``: ``idamax`` also takes
    the first maximum).  The pivot sequences can only be compared where no column is a near-tie:
    ``pivot_gap``, computed from the reference alone.

Convention throughout: ``perm`` is the row permutation as one vector, row i of P A is row
``perm[i]`` of A, i.e. ``A[perm] = L U``.

The checker, ``check_lu``, asserts textbook bounds: Higham, Accuracy and Stability of Numerical
Algorithms (2nd ed.), Theorem 9.3 (|L U - P A| <= gamma_N |L||U|) and Theorem 9.4
((A + dA) x = b with |dA| <= gamma_3N P'|L||U|), which hold for any order of the operations and
with FMAs.  u = 2^-53, gamma_k = k u / (1 - k u).  The terms ``gamma_N (|A||x| + |b|)`` and
``gamma_N |A||v|`` are the host's own rounding in forming the residual it tests."""

import numpy as np
import scipy.linalg as sla

U_ROUND = 2.0 ** -53
FULL_CHECK_MAX = 1100  # above: the factor check goes through one probe vector (O(N^2))

# Gaussian sizes of the GPU tests: both sides of every group (8), panel (32), solve-block (64) and
# gemv-workgroup (256) boundary and of R = 1 | 2 (1024 rows; at 1056 the SECOND panel is 1024 tall)
GAUSS_SMALL = (1, 2, 7, 8, 9, 31, 32, 33, 40, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1024,
               1025, 1056, 1057)
# first panel through R = 2, 3, 4, 5 rows per thread and onto the streaming kernel (5153: two
# streamed panels, then R = 5)
GAUSS_LARGE = (2048, 2049, 3073, 4097, 5120, 5121, 5153)
GAP_MIN = 1e-8
FAR_SMALL, FAR_MID, FAR_LARGE = (1, 17, 40), (1, 64, 1024), (1, 64, 1024, 2048, 4096)
REG_ROWS_MAX = 5120  # panels taller than this stream (pgf_lu.hip)


def gamma(k):
    return k * U_ROUND / (1.0 - k * U_ROUND)


# ---------------------------------------------------------------- inputs
def gaussian(N):
    A = np.random.default_rng(900 + N).standard_normal((N, N))
    if N:
        A[0, 0] = 0.0 if N > 1 else 2.0  # a zero in the first pivot position: pivoting must move it
    return A


def rhs_set(N, seed=0):
    """One Gaussian vector, the unit vector e_{N-1}, and magnitudes from 1e-8 to 1e8."""
    rng = np.random.default_rng(7000 + 13 * N + seed)
    e = np.zeros(N)
    e[N - 1] = 1.0
    wide = rng.standard_normal(N) * 10.0 ** np.linspace(-8.0, 8.0, N)[rng.permutation(N)]
    return [rng.standard_normal(N), e, wide]


def wilkinson(N):
    """1 on the diagonal, -1 below it, 1 in the last column: every column ties between the diagonal
    and ALL rows below.  Returns (A, F, perm): no interchange, L = tril(A), U[k, N-1] = 2^k."""
    A = np.eye(N) - np.tril(np.ones((N, N)), -1)
    A[:, N - 1] = 1.0
    F = np.tril(A, -1) + np.eye(N)
    F[:, N - 1] = 2.0 ** np.arange(N)
    return A, F, np.arange(N)


def _unit_lower(N, far, rng, mag):
    L0 = np.eye(N)
    for d in far:
        c = np.arange(max(N - d, 0))
        keep = rng.random(c.size) < 0.5
        sign = np.where(rng.random(c.size) < 0.5, -mag, mag)
        L0[c[keep] + d, c[keep]] = sign[keep]
    return L0


def _upper(N, rng, diag):
    U0 = np.zeros((N, N))
    U0[np.arange(N), np.arange(N)] = diag
    for r in range(N - 1):
        cols = r + 1 + rng.integers(0, N - 1 - r, size=3)  # (a repeated column is written once more)
        U0[r, cols] = rng.choice([-1.0, 1.0, 2.0], size=3)
    return U0


def tie_family(N, far, seed):
    """A = L0 U0, L0 unit lower with +-1 at rows c + d (d in far, each present with probability
    1/2), U0 unit upper with three entries from {-1, 1, 2} per row.  Column c of the remaining
    matrix is L0[c:, c]: a tie between the diagonal row and the rows d below; the smallest row
    wins.  Returns (A, F, perm): no interchange, factor (L0, U0)."""
    rng = np.random.default_rng(seed)
    L0 = _unit_lower(N, far, rng, 1.0)
    U0 = _upper(N, rng, np.ones(N))
    return L0 @ U0, np.tril(L0, -1) + U0, np.arange(N)


def _pivot_parts(N, far, seed):
    rng = np.random.default_rng(seed)
    L0 = _unit_lower(N, far, rng, 0.5)
    U0 = _upper(N, rng, rng.choice([1.0, 2.0, 4.0], size=N))
    return L0, U0, rng.permutation(N)


def _scatter_rows(LU, p):
    A = np.empty_like(LU)
    A[p] = LU  # A[p] = L0 U0: row i of P A is row p[i] of A
    return A


def pivot_family(N, far, seed):
    """The same with the off-diagonal entries of L0 at +-0.5 and diag(U0) from {1, 2, 4}, the rows
    scattered by a random permutation p (A[p] = L0 U0): column c of the remaining matrix is
    U0[c, c] L0[., c], ONE maximum, in row p[c] of A.  Returns (A, F, perm = p)."""
    L0, U0, p = _pivot_parts(N, far, seed)
    return _scatter_rows(L0 @ U0, p), np.tril(L0, -1) + U0, p


def singular_family(N, far, seed, c):
    """pivot_family with U0[c, c] = 0: column c is exactly zero at and below the diagonal when its
    turn comes, after c clean eliminations."""
    L0, U0, p = _pivot_parts(N, far, seed)
    U0[c, c] = 0.0
    return _scatter_rows(L0 @ U0, p)


# ---------------------------------------------------------------- references
def piv_to_perm(piv):
    """LAPACK's interchange sequence (0-based) as one permutation: row i of P A is row perm[i]."""
    perm = np.arange(len(piv))
    for i, p in enumerate(piv):
        perm[i], perm[p] = perm[p], perm[i]
    return perm


def scipy_lu(A):
    """(F, perm) of LAPACK's dgetrf."""
    lu, piv = sla.lu_factor(A, check_finite=False)
    return lu, piv_to_perm(piv)


def plain_lu(A, dtype=np.float64):
    """Right-looking LU with partial pivoting (first maximum), one column at a time; with
    dtype=object on a matrix of fractions.Fraction it is exact.  Returns (F, perm)."""
    F = np.array(A, dtype=dtype)
    N = F.shape[0]
    perm = np.arange(N)
    for c in range(N):
        col = [abs(v) for v in F[c:, c]]
        p = c + max(range(len(col)), key=lambda i: (col[i], -i))
        if p != c:
            F[[c, p]] = F[[p, c]]
            perm[[c, p]] = perm[[p, c]]
        F[c + 1:, c] = F[c + 1:, c] / F[c, c]
        F[c + 1:, c + 1:] = F[c + 1:, c + 1:] - np.outer(F[c + 1:, c], F[c, c + 1:])
    return F, perm


def pivot_gap(lu):
    """1 - max_c max_{i > c} |L[i, c]|: how far the closest runner-up of any column's pivot search
    stayed behind the winner (relative).  From the reference's factor alone."""
    low = np.abs(np.tril(lu, -1))
    return 1.0 - float(low.max(initial=0.0))


def expected_panels(N, streaming_only):
    """(reg, streamed) panels of a factorisation of order N."""
    tall = [N - c0 > REG_ROWS_MAX for c0 in range(0, N, 32)]
    streamed = len(tall) if streaming_only else sum(tall)
    return len(tall) - streamed, streamed


# ---------------------------------------------------------------- the checker
def _ratio(R, B, what):
    """max R / B; R <= B is asserted entry by entry WITHOUT dividing (both sides can be 0)."""
    ok = R <= B
    if not ok.all():
        k = np.unravel_index(int(np.argmax(np.where(ok, -np.inf, R - B))), R.shape)
        raise AssertionError(f"{what}: error {R[k]:.3e} > bound {B[k]:.3e} at {tuple(int(i) for i in k)}, "
                             f"{int((~ok).sum())} entries over")
    pos = B > 0
    return float((R[pos] / B[pos]).max(initial=0.0))


def _check_solves(A, aL, aU, perm, rhs_list, solve, trans, out):
    """Items 5 and 6: aL = |L| without its unit diagonal, aU = |U|."""
    N = A.shape[0]
    gN, aA = gamma(N), np.abs(A)
    inv = np.empty(N, dtype=np.int64)
    inv[perm] = np.arange(N)
    for k, b in enumerate(rhs_list):
        b = np.asarray(b, dtype=np.float64)
        for tr in trans:
            x = np.asarray(solve(b, tr), dtype=np.float64)
            assert x.shape == (N,) and np.isfinite(x).all(), f"rhs {k} trans={tr}: solution not finite"
            ax = np.abs(x)
            if not tr:
                w = aU @ ax
                B = 3.0 * gN * (aL @ w + w)[inv] + gN * (aA @ ax + np.abs(b))
                R = np.abs(b - A @ x)
                key, what = "solve", "|b - A x|"
            else:
                w = ax[perm]
                w = aL.T @ w + w
                B = 3.0 * gN * (aU.T @ w) + gN * (aA.T @ ax + np.abs(b))
                R = np.abs(b - A.T @ x)
                key, what = "solve_trans", "|b - A' x|"
            out[key] = max(out.get(key, 0.0), _ratio(R, B, f"rhs {k}: {what} <= 3 gamma_N |L||U||x| + host"))
    return out


def check_lu(A, F, perm, rhs_list=(), solve=None, full=None, trans=(False, True), probe_seed=1):
    """Assert that (F, perm) is a backward-stable LU with partial pivoting of A and that
    ``solve(b, trans)`` solves with it.  Returns {check: largest error / bound} for information;
    the criterion is the bound.  ``full``: entrywise factor check (default: N <= 1100), else
    through one Gaussian probe vector."""
    A = np.asarray(A, dtype=np.float64)
    F = np.asarray(F, dtype=np.float64)
    N = A.shape[0]
    perm = np.asarray(perm)
    gN = gamma(max(N, 1))
    out = {}
    # 1. a permutation
    assert perm.shape == (N,) and np.array_equal(np.sort(perm), np.arange(N)), "perm is no permutation"
    # 2. finite
    assert F.shape == (N, N) and np.isfinite(F).all(), "factor not finite"
    if N == 0:
        return out
    Lm = np.tril(F, -1)  # strictly lower part: L = Lm + I
    Um = np.triu(F)
    # 3. multipliers: quotients by the column's maximum
    lmax = float(np.abs(Lm).max(initial=0.0))
    assert lmax <= 1.0, f"multiplier {lmax!r} > 1"
    aL, aU = np.abs(Lm), np.abs(Um)
    if full is None:
        full = N <= FULL_CHECK_MAX
    # 4. the factor
    if full:
        R = np.abs(Lm @ Um + Um - A[perm])
        B = gN * (aL @ aU + aU)
        out["factor"] = _ratio(R, B, "|L U - A[perm]| <= gamma_N |L||U|")
    else:
        v = np.random.default_rng(probe_seed).standard_normal(N)
        Uv, aUv = Um @ v, aU @ np.abs(v)
        R = np.abs(Lm @ Uv + Uv - (A @ v)[perm])
        B = gN * (aL @ aUv + aUv) + gN * (np.abs(A) @ np.abs(v))[perm]
        out["factor_probe"] = _ratio(R, B, "|L(Uv) - (A v)[perm]| <= gamma_N (|L||U||v| + (|A||v|)[perm])")
    # 5., 6. the solves
    return _check_solves(A, aL, aU, perm, rhs_list, solve, trans, out)


def check_solves_with_reference_factor(A, rhs_list, solve):
    """Items 5 and 6 for a solver whose factor cannot be read out: |L||U| and perm from LAPACK's
    factorisation of the same matrix (only the bound uses them)."""
    A = np.asarray(A, dtype=np.float64)
    lu, perm = scipy_lu(A)
    return _check_solves(A, np.abs(np.tril(lu, -1)), np.abs(np.triu(lu)), perm, rhs_list, solve,
                         (False, True), {})
