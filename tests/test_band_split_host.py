"""Factor / solve split of the wide block cyclic reduction (csrc/pgf_band_wide.hip), host only.

A numpy restatement of the reduction that keeps, per eliminated block e, inv(D_e), its couplings
L_e, U_e and the two forward multipliers Mr[e] = L_{e+s} inv(D_e), Ml[e] = U_{e-s} inv(D_e), and of
the solve phase that uses nothing else.  It pins the multiplier indexing and the missing-neighbour
cases (a kept block without a right neighbour at some level, the single block) without a GPU.
Also the argument checks of the Python surface: ``pgf_band_split`` and the 2-D ``solve``."""

import numpy as np
import pytest


def bcr_factor(K, B):
    """Kept factors of the block cyclic reduction of K (half-bandwidth <= B) with B x B blocks; the
    last block is padded with the identity."""
    N = K.shape[0]
    nb = -(-N // B)
    Kp = np.eye(nb * B)
    Kp[:N, :N] = K
    blk = lambda i, j: Kp[i * B:(i + 1) * B, j * B:(j + 1) * B].copy()  # noqa: E731
    zero = np.zeros((B, B))
    D = [blk(i, i) for i in range(nb)]
    L = [blk(i, i - 1) if i > 0 else zero.copy() for i in range(nb)]
    U = [blk(i, i + 1) if i + 1 < nb else zero.copy() for i in range(nb)]
    Dinv, Mr, Ml = [None] * nb, [None] * nb, [None] * nb
    levels, s = [], 1
    while s < nb:
        for e in range(s, nb, 2 * s):
            Dinv[e] = np.linalg.inv(D[e])
        for i in range(0, nb, 2 * s):
            le, ri = i - s, i + s
            if le >= 0:
                T = L[i] @ Dinv[le]
                Mr[le] = T
                D[i] = D[i] - T @ U[le]
                L[i] = -T @ L[le]
            else:
                L[i] = zero.copy()
            if ri < nb:
                T = U[i] @ Dinv[ri]
                Ml[ri] = T
                D[i] = D[i] - T @ L[ri]
                U[i] = -T @ U[ri]
            else:
                U[i] = zero.copy()
        levels.append(s)
        s *= 2
    Dinv[0] = np.linalg.inv(D[0])
    return dict(N=N, B=B, nb=nb, levels=levels, Dinv=Dinv, L=L, U=U, Mr=Mr, Ml=Ml)


def bcr_solve(fac, rhs):
    """Solve phase against the kept factors; rhs (N,) or (N, nrhs)."""
    N, B, nb = fac["N"], fac["B"], fac["nb"]
    rhs = np.asarray(rhs, dtype=np.float64)
    cols = rhs.reshape(N, -1)
    f = np.zeros((nb * B, cols.shape[1]))
    f[:N] = cols
    f = [f[i * B:(i + 1) * B].copy() for i in range(nb)]
    for s in fac["levels"]:
        for i in range(0, nb, 2 * s):
            if i - s >= 0:
                f[i] = f[i] - fac["Mr"][i - s] @ f[i - s]
            if i + s < nb:
                f[i] = f[i] - fac["Ml"][i + s] @ f[i + s]
    x = [None] * nb
    x[0] = fac["Dinv"][0] @ f[0]
    for s in reversed(fac["levels"]):
        for e in range(s, nb, 2 * s):
            t = f[e] - fac["L"][e] @ x[e - s]
            if e + s < nb:
                t = t - fac["U"][e] @ x[e + s]
            x[e] = fac["Dinv"][e] @ t
    return np.concatenate(x)[:N].reshape(rhs.shape)


def quasi_definite_band(N, bw, seed):
    """Symmetric band of half-width bw, small off-diagonals, a diagonal of mixed sign in
    +-[2, 3]: diagonally dominant, and with the positive rows first [[H, A'], [A, -G]], H and G
    positive definite."""
    rng = np.random.default_rng(seed)
    K = np.zeros((N, N))
    for k in range(1, min(bw, N - 1) + 1):
        v = 0.04 * rng.uniform(0.5, 1.0, N - k)
        K += np.diag(v, k) + np.diag(v, -k)
    K += np.diag(rng.uniform(2.0, 3.0, N) * np.where(rng.random(N) < 0.4, -1.0, 1.0))
    return K


@pytest.mark.parametrize("nb", [1, 2, 3, 5, 33])
def test_kept_factors_solve(nb):
    B = 16
    N = nb * B - 5  # a padded last block
    K = quasi_definite_band(N, 12, nb)
    rng = np.random.default_rng(100 + nb)
    fac = bcr_factor(K, B)
    assert fac["nb"] == nb and fac["levels"] == [2 ** q for q in range(int(np.ceil(np.log2(nb))))]
    # every block but block 0 was eliminated exactly once and owns at most two multipliers
    for e in range(1, nb):
        assert fac["Dinv"][e] is not None and fac["Ml"][e] is not None
    assert fac["Mr"][0] is None and fac["Ml"][0] is None
    for _ in range(2):  # the factors serve any number of right-hand sides
        rhs = rng.standard_normal(N)
        ref = np.linalg.solve(K, rhs)
        err = np.abs(bcr_solve(fac, rhs) - ref).max() / np.abs(ref).max()
        assert err <= 1e-10, err
    P = rng.standard_normal((N, 17))
    ref = np.linalg.solve(K, P)
    assert np.abs(bcr_solve(fac, P) - ref).max() / np.abs(ref).max() <= 1e-10


def test_full_blocks_without_padding():
    K = quasi_definite_band(5 * 16, 16, 9)  # bw == B, N a multiple of B
    rhs = np.arange(1.0, 81.0)
    ref = np.linalg.solve(K, rhs)
    assert np.abs(bcr_solve(bcr_factor(K, 16), rhs) - ref).max() / np.abs(ref).max() <= 1e-10


# ---------------------------------------------------------------- the Python surface
class _Problem:
    pass


@pytest.mark.parametrize("value,want", [(None, None), (True, True), (False, False), (0, False), (1, True),
                                        (np.bool_(False), False)])
def test_band_split_values(value, want):
    from pygradflow_amd.sparse import band_split

    p = _Problem()
    if value is not None:
        p.pgf_band_split = value
    assert band_split(p) is want


@pytest.mark.parametrize("value", ["off", 2, -1, 0.5, [True]])
def test_band_split_rejects(value):
    from pygradflow_amd.sparse import band_split

    p = _Problem()
    p.pgf_band_split = value
    with pytest.raises(ValueError, match="pgf_band_split"):
        band_split(p)


class _Owner:
    """What ``_DeviceFactorView`` reads of a banded step solver before it calls the library."""

    sparse = True
    formulation = 0
    n, m = 6, 2
    active_set = np.array([False, True, False, False, True, False])


@pytest.mark.parametrize("shape", [(5, 3), (7, 1), (6, 2, 1), ()])
def test_solve_rejects_bad_shapes(shape):
    from pygradflow_amd.step_solver import _DeviceFactorView

    view = _DeviceFactorView(_Owner())  # rows = 4 inactive + 2 = 6
    with pytest.raises(ValueError):
        view.solve(np.zeros(shape))


def test_solve_of_no_columns():
    from pygradflow_amd.step_solver import _DeviceFactorView

    out = _DeviceFactorView(_Owner()).solve(np.zeros((6, 0)))
    assert out.shape == (6, 0)
