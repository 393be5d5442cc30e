"""Host plan of the bordered band (pygradflow_amd/sparse.py, BandPlan(border=...)): which nodes go
into the border, the band of the remainder, and the slot layout -- restated in numpy from
(pos, slots, values, mask) the plan must reproduce the oracle's KKT matrix, permuted, bit for bit.
CPU only."""

import numpy as np
import pytest
import scipy.sparse as sps
from scipy.sparse.csgraph import reverse_cuthill_mckee

from oracle import newton_oracle as O
from pygradflow_amd import problems
from pygradflow_amd.sparse import MAX_BANDWIDTH, BandPlan
from tests.band_util import bordered_lq


def _plan(prob, border):
    return BandPlan(prob.hess_sparse(), prob.jac_sparse(), prob.num_vars, prob.num_cons, border=border)


def restate(plan, hv, jv, mask, lamb, delta):
    """What the device assembles (k_border_set_diag, k_band_scatter_H / _J) as a dense symmetric
    matrix in plan order: band rows, then the border."""
    n, m, Nb, k, kp, ldb = plan.n, plan.m, plan.Nb, plan.k, plan.kp, plan.ldb
    store = np.zeros(plan.store_size)
    for i in range(n + m):
        v = (1.0 if mask[i] else lamb) if i < n else -delta
        p = int(plan.pos[i])
        if p < Nb:
            store[p * ldb] = v
        else:
            store[plan.base_D + (p - Nb) * kp + (p - Nb)] = v
    for j in range(k, kp):
        store[plan.base_D + j * kp + j] = 1.0
    for e in range(plan.nnzH):
        s = plan.Hslot[e]
        if s >= 0 and not (mask[plan.Hrow[e]] or mask[plan.Hcol[e]]):
            store[s] += hv[e]
    for e in range(plan.nnzJ):
        if not mask[plan.Jcol[e]]:
            store[plan.Jslot[e]] = jv[e]
    N = Nb + k
    K = np.zeros((N, N))
    for i in range(Nb):
        for d in range(min(plan.bw, i) + 1):
            K[i, i - d] = K[i - d, i] = store[i * ldb + d]
    if k:
        C = store[plan.base_C: plan.base_C + Nb * kp].reshape(Nb, kp)
        D = store[plan.base_D: plan.base_D + kp * kp].reshape(kp, kp)
        assert not C[:, k:].any()
        assert np.array_equal(D[k:, k:], np.eye(kp - k)) and not D[k:, :k].any()
        K[:Nb, Nb:] = C[:, :k]
        K[Nb:, :Nb] = C[:, :k].T
        Dl = np.tril(D[:k, :k])
        K[Nb:, Nb:] = Dl + np.tril(Dl, -1).T
    return K


def oracle_full(prob, mask, lamb, rho, pos):
    """The oracle's reduced KKT matrix, active variables put back as identity rows, permuted."""
    n, m = prob.num_vars, prob.num_cons
    rows = O.shifted_hess_rows(prob.hess_sparse(), lamb, mask)
    Kr = O.kkt_matrix(rows, prob.jac_sparse().tocsc(), mask, lamb, rho).toarray()
    keep = np.concatenate([np.nonzero(~mask)[0], n + np.arange(m)])
    Kf = np.zeros((n + m, n + m))
    Kf[np.ix_(keep, keep)] = Kr
    act = np.nonzero(mask)[0]
    Kf[act, act] = 1.0
    Kp = np.zeros_like(Kf)
    Kp[np.ix_(pos, pos)] = Kf
    return Kp


def test_budget_row_border_and_layout():
    prob = problems.budget_box_qp(1003)
    n = prob.num_vars
    plan = _plan(prob, "auto")
    assert list(plan.border) == [n]  # the constraint
    assert plan.k == 1 and plan.kp == 16 and plan.Nb == n
    band_only = problems.LinearQuadraticProblem(prob.Q, prob.q, sps.csr_matrix((0, n)), np.zeros(0),
                                                prob.var_lb, prob.var_ub)
    assert plan.bw == _plan(band_only, None).bw == 1
    assert _plan(prob, None).bw == 1001  # the one dense row, without a border
    assert plan.supported and plan.block_size == 8
    assert sorted(plan.pos) == list(range(n + 1)) and plan.pos[n] == n
    hv, jv = plan.values(prob.hess_sparse(), prob.jac_sparse())
    dt, rho = 0.7, 1.3
    lamb = 1.0 / dt
    delta = lamb / (1.0 + lamb * rho)
    rng = np.random.default_rng(0)
    for mask in (rng.uniform(size=n) < 0.5, rng.uniform(size=n) < 0.1, np.ones(n, dtype=bool)):
        assert np.array_equal(restate(plan, hv, jv, mask, lamb, delta),
                              oracle_full(prob, mask, lamb, rho, plan.pos))


def test_global_parameters_are_the_border():
    prob = problems.ocp_global_parameter(40, 4, 2, 3)
    n = prob.num_vars
    plan = _plan(prob, "auto")
    assert list(plan.border) == [n - 3, n - 2, n - 1]
    assert plan.bw <= 16 and plan.supported
    # variables in the border, a mask that makes one of them active: the layout still holds
    hv, jv = plan.values(prob.hess_sparse(), prob.jac_sparse())
    mask = np.random.default_rng(1).uniform(size=n) < 0.3
    mask[n - 2] = True
    mask[n - 1] = False
    lamb, rho = 2.0, 1.0
    assert np.array_equal(restate(plan, hv, jv, mask, lamb, lamb / (1.0 + lamb * rho)),
                          oracle_full(prob, mask, lamb, rho, plan.pos))


def test_explicit_border_is_honoured():
    prob = problems.budget_box_qp(203)
    n = prob.num_vars
    plan = _plan(prob, [n, 17, 5])  # the dense row and two ordinary band variables
    assert list(plan.border) == [5, 17, n]  # variables before constraints
    assert [int(plan.pos[i]) for i in (5, 17, n)] == [plan.Nb, plan.Nb + 1, plan.Nb + 2]
    assert plan.bw <= 2 and plan.supported
    hv, jv = plan.values(prob.hess_sparse(), prob.jac_sparse())
    mask = np.random.default_rng(2).uniform(size=n) < 0.4
    mask[5], mask[17] = True, False
    lamb, rho = 1.0, 1.0
    assert np.array_equal(restate(plan, hv, jv, mask, lamb, lamb / (1.0 + lamb * rho)),
                          oracle_full(prob, mask, lamb, rho, plan.pos))
    with pytest.raises(ValueError):
        _plan(prob, list(range(65)))
    with pytest.raises(ValueError):
        _plan(prob, [n + 1])
    with pytest.raises(ValueError):
        _plan(prob, "widest")


@pytest.mark.parametrize("k", [33, 48, 49])
def test_layout_at_padded_widths_48_and_64(k):
    """k = 33, 48 (kp = 48: the first and the last width of that padding) and 49 (kp = 64), border
    variables and constraints mixed, one border variable active and one not: C, the lower triangle
    of D and the padding land where the device reads them."""
    kv = k // 3
    prob = bordered_lq(45, 2, 12, kv, k - kv, seed=k)
    n, m = prob.num_vars, prob.num_cons
    plan = _plan(prob, prob.pgf_border)
    assert plan.k == k and plan.kp == (48 if k <= 48 else 64) and plan.Nb == 57 and plan.supported
    assert list(plan.border) == list(range(45, n)) + list(range(n + 12, n + m))
    assert np.array_equal(plan.pos[plan.border], 57 + np.arange(k))
    hv, jv = plan.values(prob.hess_sparse(), prob.jac_sparse())
    mask = np.random.default_rng(k).uniform(size=n) < 0.4
    mask[45], mask[46] = True, False
    lamb, rho = 0.8, 1.7
    assert np.array_equal(restate(plan, hv, jv, mask, lamb, lamb / (1.0 + lamb * rho)),
                          oracle_full(prob, mask, lamb, rho, plan.pos))


def test_more_than_64_border_nodes_is_unsupported():
    prob = problems.multistate_ocp(300, 24, 8)
    assert not _plan(prob, None).supported
    plan = _plan(prob, "auto")
    assert plan.supported is False
    assert plan.bw > MAX_BANDWIDTH and plan.k == 64


def test_plan_without_border_is_unchanged():
    """pos, bw and the slots of a plain plan, against the formulas as they stood before the border
    existed, written out here."""
    prob = problems.sparse_ocp(200)
    n, m = prob.num_vars, prob.num_cons
    plan = _plan(prob, None)
    assert plan.k == 0 and plan.border.size == 0
    H, J = prob.hess_sparse(), prob.jac_sparse()
    Hp = sps.csr_matrix((np.ones(H.nnz), H.indices, H.indptr), shape=(n, n))
    Jp = sps.csr_matrix((np.ones(J.nnz), J.indices, J.indptr), shape=(m, n))
    pat = sps.bmat([[Hp + Hp.T + sps.identity(n), Jp.T], [Jp, sps.identity(m)]], format="csr")
    perm = reverse_cuthill_mckee(pat, symmetric_mode=True)
    pos = np.empty(n + m, dtype=np.int64)
    pos[perm] = np.arange(n + m)
    coo = pat.tocoo()
    bw = int(np.max(np.abs(pos[coo.row] - pos[coo.col])))
    ldb = (bw + 2) // 2 * 2
    assert plan.bw == bw and plan.ldb == ldb
    assert np.array_equal(plan.pos, pos)
    hrow = np.repeat(np.arange(n), np.diff(H.indptr))
    pi, pj = pos[hrow], pos[H.indices]
    use = (pi >= pj) | ~(np.asarray(Hp[H.indices, hrow]).ravel() > 0)
    assert np.array_equal(plan.Hslot, np.where(use, np.maximum(pi, pj) * ldb + np.abs(pi - pj), -1))
    jrow = np.repeat(np.arange(m), np.diff(J.indptr))
    pa, pb = pos[n + jrow], pos[J.indices]
    assert np.array_equal(plan.Jslot, np.maximum(pa, pb) * ldb + np.abs(pa - pb))
