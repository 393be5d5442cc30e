"""Banded device batch (csrc/pgf_sparse.hip, csrc/pgf_api_band_batch.hip): many banded instances
of one sparsity pattern advanced by one launch sequence per Newton step.

Two references.  ``sequential=True`` drives the same instances one by one through their own handles:
both routes run the same device functions in the same order, so masks, x and y are compared bit for
bit (``np.array_equal``), the inertia exactly, and the step length within 1e-14 relative (its sum is
taken in another order).  The CPU oracle: masks identical, x and y within ``band_util.TOL`` (1e-10),
n_neg = m.  Shapes are the smallest that reach each kernel branch.
"""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

from oracle import newton_oracle as O
from tests import golden_util as G
from tests.band_util import (TOL, band_problem, bordered_lq, head_of_first_eliminated, mask_changes,
                             plan_of, refined_solve)

pytestmark = pytest.mark.gpu

POLICIES = ("Simplified", "Full", "ActiveSet")


def _forced(prob):
    prob.pgf_force_band = True
    return prob


def _batch(probs, pol, dt=1.0, rho=1.0, sequential=False):
    from pygradflow_amd.batched import BatchedDeviceNewton

    return BatchedDeviceNewton(lambda i: probs[i], len(probs), pol, dt, rho, sequential=sequential)


def _same_step(bd, ref, tag):
    """One step of the batch and of the sequential loop: the bars of the module docstring."""
    st, nn, df = bd.step_local()
    st2, nn2, df2 = ref.step_local()
    assert not st.any() and not st2.any(), (tag, st, st2)
    assert np.array_equal(bd.masks(), ref.masks()), tag
    (x, y), (x2, y2) = bd.points(), ref.points()
    assert np.array_equal(x, x2), (tag, G.rel_err(x, x2))
    assert np.array_equal(y, y2), (tag, G.rel_err(y, y2))
    assert np.array_equal(nn, nn2), (tag, nn, nn2)
    assert np.all(np.abs(df - df2) <= 1e-14 * np.abs(df2)), (tag, df, df2)
    return nn


def _same_as_sequential(probs, policies=(("Full", 2), ("Simplified", 1))):
    """Fresh instances per policy, batch against sequential=True."""
    for pol, steps in policies:
        bd, ref = _batch(probs, pol), _batch(probs, pol, sequential=True)
        assert bd.band
        for k in range(steps):
            nn = _same_step(bd, ref, (pol, k))
            assert np.all(nn == probs[0].num_cons), (pol, k, nn)
        assert bd.band_stats()[0] == steps
        bd.close()
        ref.close()


def _against_oracle(probs, policies=tuple((p, 3) for p in POLICIES), dt=1.0, rho=1.0):
    """Every instance of the batch against NewtonOracle from zero; returns the number of steps whose
    mask differs from the step before, summed over instances and policies."""
    n, m = probs[0].num_vars, probs[0].num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    churn = 0
    for pol, steps in policies:
        recs = [O.NewtonOracle(p, pol, x0, y0, dt, rho).run(x0, y0, steps) for p in probs]
        bd = _batch(probs, pol, dt, rho)
        assert bd.band
        for k in range(steps):
            st, nn, _ = bd.step_local()
            assert not st.any(), (pol, k, st)
            mk = bd.masks()
            x, y = bd.points()
            for i, rec in enumerate(recs):
                assert np.array_equal(mk[i], rec[k]["mask"]), (pol, k, i)
                assert G.rel_err(x[i], rec[k]["xn"]) <= TOL, (pol, k, i)
                assert G.rel_err(y[i], rec[k]["yn"]) <= TOL, (pol, k, i)
                assert nn[i] == m, (pol, k, i, nn[i])
        bd.close()
        churn += sum(int(not np.array_equal(a["mask"], b["mask"])) for r in recs for a, b in zip(r, r[1:]))
    return churn


# ------------------------------------------------------------------ 1: the batch exists
def test_banded_instances_form_a_device_batch_and_take_the_batched_route(pgf):
    from pygradflow_amd import problems

    probs = [_forced(problems.box_qp(264, seed=i)) for i in range(3)]
    bd = _batch(probs, "Full")
    assert bd.band and bd._b is not None
    for _ in range(2):
        st, _, _ = bd.step_local()
        assert not st.any()
    # one batched reduction (and assembly) per step, whatever the number of instances
    assert bd.band_stats() == (2, 2)
    assert bd.factor_kind() == 0
    bd.close()


# ------------------------------------------------------------------ 2: every branch of the plan
def _sweep_problems(kind, size, B=3):
    from pygradflow_amd import problems

    make = problems.box_qp if kind == "box" else problems.sparse_ocp
    return [_forced(make(size, seed=size + 7 * i)) for i in range(B)]


@pytest.mark.parametrize("kind,size", [("box", n) for n in (7, 9, 256, 257, 513, 1033)]
                         + [("ocp", m) for m in (3, 85, 86, 171, 343)])
def test_same_as_one_by_one_on_every_branch_of_the_launch_plan(pgf, kind, size):
    """Block counts 1 (ragged), 2, 32 (the most the tail takes), 33 (single level, odd), 65 (pair),
    130 (pair whose last workgroup lies beyond nb, plus single s = 4) and 2, 32, 33, 65, 129: the
    table of test_band_narrow_gpu.py::test_block_counts_on_every_branch_of_the_launch_plan."""
    probs = _sweep_problems(kind, size)
    plan = plan_of(probs[0])
    assert plan.block_size == 8 and plan.bw <= 8
    _same_as_sequential(probs)


# ------------------------------------------------------------------ 3, 4: against the oracle
def _ocp(i):
    from pygradflow_amd import problems

    return _forced(problems.multistate_ocp(60, 3, 1, seed=i))  # bw 7, N = 420, boxed controls


def test_against_the_oracle_constrained(pgf):
    probs = [_ocp(i) for i in range(5)]
    assert plan_of(probs[0]).bw == 7 and probs[0].num_vars + probs[0].num_cons == 420
    for pol in ("Full", "ActiveSet"):  # (Simplified keeps its mask by definition)
        assert any(mask_changes(p, pol, 3) > 0 for p in probs)
    assert _against_oracle(probs) > 0


def test_against_the_oracle_box_qp(pgf):
    from pygradflow_amd import problems

    probs = [_forced(problems.box_qp(600, seed=i)) for i in range(5)]
    for pol in ("Full", "ActiveSet"):
        assert any(mask_changes(p, pol, 3) > 0 for p in probs)
    assert _against_oracle(probs) > 0


def test_values_differ_per_instance_not_only_vectors(pgf):
    """H_i = (1 + i / 4) H and J_i = (1 - i / 8) J on one pattern."""
    from pygradflow_amd import problems

    base = _ocp(0)
    H, J = base.hess_sparse(), base.jac_sparse()
    probs = [_forced(problems.LinearQuadraticProblem(sps.csr_matrix(H * (1 + i / 4)), base.q,
                                                     sps.csr_matrix(J * (1 - i / 8)), base.b,
                                                     base.var_lb, base.var_ub)) for i in range(4)]
    assert _against_oracle(probs) > 0


# ------------------------------------------------------------------ 5: bandwidths 1 .. 8
def _bandwidth_case(bw, k):
    """Instance k of the problems of test_band_narrow_gpu.py::_bandwidth_case (same pattern, other
    data)."""
    from pygradflow_amd import problems

    if bw in (2, 3, 4):
        n = 300
        d = 2.5 + np.random.default_rng(bw + 10 * k).uniform(0.0, 0.5, n)
        return band_problem(n, d, bw + 10 * k, bw, lb=np.full(n, -0.2), ub=np.full(n, 0.2))
    return {1: lambda: problems.box_qp(300, seed=1 + k), 5: lambda: problems.grid_box_qp(5, 40, seed=k),
            6: lambda: problems.multistate_ocp(50, 2, 1, seed=k), 7: lambda: problems.multistate_ocp(50, 3, 1, seed=k),
            8: lambda: problems.multistate_ocp(400, 3, 2, seed=k)}[bw]()


@pytest.mark.parametrize("bw", [1, 2, 3, 4, 5, 6, 7, 8])
def test_every_bandwidth_up_to_8(pgf, bw):
    probs = [_forced(_bandwidth_case(bw, k)) for k in range(2)]
    plan = plan_of(probs[0])
    assert plan.bw == bw and plan.block_size == 8
    _same_as_sequential(probs)


# ------------------------------------------------------------------ 6: B edge cases
def test_batch_of_one_equals_the_single_handle(pgf):
    from pygradflow_amd import problems

    prob = _forced(problems.box_qp(264, seed=5))
    bd = _batch([prob], "Full")
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(264), np.zeros(0), 1.0, 1.0)
    assert bd.band and dn.sparse
    for k in range(2):
        st, nn, df = bd.step_local()
        d1, n1 = dn.step()
        x, y = bd.points()
        x1, y1 = dn.point()
        assert st[0] == 0 and nn[0] == n1 and abs(df[0] - d1) <= 1e-14 * abs(d1), k
        assert np.array_equal(x[0], x1) and np.array_equal(y[0], y1), k
        assert np.array_equal(bd.masks()[0], dn.mask()), k
    bd.close()
    dn.close()


def test_seventy_tiny_instances_with_all_active_and_unbounded_ones(pgf):
    """More instances than the first cache lines of the table hold, tiny N = 40 (5 blocks: the LDS
    tail alone); instance 3 has bounds 0.0 (every variable active), instance 5 has none, the others
    are ordinary."""
    from pygradflow_amd import problems

    probs = [_forced(problems.box_qp(40, seed=i, bound={3: 0.0, 5: np.inf}.get(i, 0.5))) for i in range(70)]
    bd, ref = _batch(probs, "Full"), _batch(probs, "Full", sequential=True)
    for k in range(2):
        _same_step(bd, ref, k)
    mk = bd.masks()
    assert mk[3].all() and not mk[5].any() and mk[0].any() and not mk[0].all()
    bd.close()
    ref.close()
    assert _against_oracle(probs[:8], (("Full", 2), ("Simplified", 1))) > 0


# ------------------------------------------------------------------ 7: per-instance outer steps
def test_per_instance_outer_steps_rejection_and_freezing(pgf):
    from pygradflow_amd import problems

    probs = [_forced(problems.box_qp(264, seed=20 + i)) for i in range(3)]
    dt = np.array([0.5, 1.0, 2.0])
    bd, ref, free = _batch(probs, "Full"), _batch(probs, "Full", sequential=True), _batch(probs, "Full")
    for run in (bd, ref, free):
        run.step_local()
        run.advance_outer_each(dt, 1.0)
    outer = bd.points()
    for k in range(2):
        _same_step(bd, ref, ("dt", k))
        free.step_local()
    # instance 1 is rejected: back to its outer point, bit for bit; the others go on
    moved, m0 = bd.points(), bd.masks()
    for run in (bd, ref, free):
        run.advance_outer_each(dt / 2, 1.0, accepted=[True, False, True])
    x, y = bd.points()
    assert np.array_equal(x[1], outer[0][1]) and np.array_equal(y[1], outer[1][1])
    assert np.array_equal(x[0], moved[0][0]) and np.array_equal(x[2], moved[0][2])
    assert not np.array_equal(x[1], moved[0][1])
    # instance 1 frozen: its point and mask stay, the others step as if nothing were frozen
    bd.set_frozen([0, 1, 0])
    ref.set_frozen([0, 1, 0])
    for k in range(2):
        st, _, df = bd.step_local()
        ref.step_local()
        free.step_local()
        assert not st.any() and df[1] == 0.0
    x, y = bd.points()
    xr, yr = ref.points()
    xf, yf = free.points()
    assert np.array_equal(x[1], outer[0][1]) and np.array_equal(bd.masks()[1], m0[1])
    assert not np.array_equal(xf[1], outer[0][1])  # (left to itself it moves)
    assert np.array_equal(x, xr) and np.array_equal(y, yr)
    for i in (0, 2):
        assert np.array_equal(x[i], xf[i]) and np.array_equal(bd.masks()[i], free.masks()[i])
    for run in (bd, ref, free):
        run.close()


# ------------------------------------------------------------------ 8: one bad instance
def _decoupled(good, v):
    """``good`` with variable v decoupled and H[v, v] = -1 (K[v, v] = 0 at dt = 1) ON THE SAME
    PATTERN: the entries of row and column v stay stored, as zeros."""
    from pygradflow_amd import problems

    H = sps.csr_matrix(good.hess_sparse(), copy=True)
    rows = np.repeat(np.arange(H.shape[0]), np.diff(H.indptr))
    H.data[(rows == v) | (H.indices == v)] = 0.0
    H.data[(rows == v) & (H.indices == v)] = -1.0
    return problems.LinearQuadraticProblem(H, good.q, good.jac_sparse(), good.b, good.var_lb, good.var_ub)


def test_one_singular_instance_does_not_spoil_the_batch(pgf):
    from pygradflow_amd import _lib

    n, v = 600, 333
    goods = [_forced(band_problem(n, 2.5 + np.random.default_rng(9 + i).uniform(0.0, 0.5, n), 3 + i, 5))
             for i in range(3)]
    bad = _forced(_decoupled(goods[1], v))
    K = bad.hess_sparse().toarray() + np.eye(n)
    assert not K[v].any() and plan_of(bad).block_size == 8
    assert plan_of(bad).pattern_hash() == plan_of(goods[0]).pattern_hash()
    bd = _batch([goods[0], bad, goods[2]], "Full")
    two = _batch([goods[0], goods[2]], "Full")
    st, _, _ = bd.step_local()
    st2, _, _ = two.step_local()
    assert list(st) == [0, _lib.PGF_SINGULAR, 0] and not st2.any()
    (x, _), (x2, _) = bd.points(), two.points()
    assert not x[1].any()  # the point it started from
    assert np.array_equal(x[0], x2[0]) and np.array_equal(x[2], x2[1])
    # the step after: the bad instance fails again, the others go on as in the batch of two
    st, _, _ = bd.step_local()
    two.step_local()
    assert list(st) == [0, _lib.PGF_SINGULAR, 0]
    (x, _), (x2, _) = bd.points(), two.points()
    assert not x[1].any() and np.array_equal(x[0], x2[0]) and np.array_equal(x[2], x2[1])
    bd.close()
    two.close()
    # a well-posed batch on the pooled handles
    bd = _batch(goods, "Full")
    st, nn, _ = bd.step_local()
    assert not st.any() and not nn.any()
    x, _ = bd.points()
    for i, p in enumerate(goods):
        assert G.rel_err(x[i], -np.linalg.solve(p.hess_sparse().toarray() + np.eye(n), p.q)) <= TOL
    bd.close()


# ------------------------------------------------------------------ 9: guard repair
def _normwise(K, x, b):
    """The guard's measure (band_residual_rel_of): max |b - K x| / max (|K| |x| + |b|)."""
    return np.abs(b - K @ x).max() / (np.abs(K) @ np.abs(x) + np.abs(b)).max()


def _gj_inverse(M):
    """Unpivoted Gauss-Jordan inverse in float64 (gj_inverse8 of pgf_bcr_dev.h)."""
    M = M.copy()
    for k in range(M.shape[0]):
        d = 1.0 / M[k, k]
        row, col = M[k, :].copy(), M[:, k].copy()
        M -= np.outer(col * d, row)
        M[k, :] = row * d
        M[:, k] = -col * d
        M[k, k] = d
    return M


def _level_one_solve(Kp, f):
    """The first level of the 8 x 8 cyclic reduction on the permuted matrix, in float64: the odd
    blocks are inverted unpivoted as they stand and eliminated; what is left is solved by LAPACK."""
    N = Kp.shape[0]
    blk = np.arange(N) // 8
    o, e = np.nonzero(blk % 2 == 1)[0], np.nonzero(blk % 2 == 0)[0]
    Dinv = np.zeros((o.size, o.size))
    for b in np.unique(blk[o]):
        idx = np.nonzero(blk[o] == b)[0]
        Dinv[np.ix_(idx, idx)] = _gj_inverse(Kp[np.ix_(o[idx], o[idx])])
    Keo, Koe = Kp[np.ix_(e, o)], Kp[np.ix_(o, e)]
    xe = np.linalg.solve(Kp[np.ix_(e, e)] - Keo @ Dinv @ Koe, f[e] - Keo @ (Dinv @ f[o]))
    x = np.zeros(N)
    x[e] = xe
    x[o] = Dinv @ (f[o] - Koe @ xe)
    return x


def test_an_unstable_pivot_in_one_instance_is_repaired_on_its_handle(pgf):
    """The recipe of test_band_narrow_gpu.py::test_narrow_unstable_pivot_is_refined at bw 5 and block
    size 8: a tiny K[v, v] at the head of block 1, which level one inverts as it stands.  The pivot
    is 1e-11 and not that test's 1e-9: at 1e-9 the emulated plain solve below misses refine_tol by a
    factor of 3 only (3.0e-11), at 1e-11 by 250 (2.5e-9), and one refinement step still brings it
    to 5e-17."""
    n, bw, eps = 300, 5, 1e-11
    rng = np.random.default_rng(7)
    ds = [2.5 + rng.uniform(0.0, 0.5, n) for _ in range(3)]
    v = head_of_first_eliminated(_forced(band_problem(n, ds[1], 1, bw)), 8)
    ds[1][v] = -1.0 + eps  # lambda = 1: K[v, v] = eps
    probs = [_forced(band_problem(n, ds[i], 1 + i, bw)) for i in range(3)]
    plan = plan_of(probs[1])
    assert plan.bw == bw and plan.block_size == 8
    K = probs[1].hess_sparse().toarray() + np.eye(n)
    assert abs(K[v, v]) < 1e-8 and np.linalg.cond(K) < 1e5
    # on the CPU first: the plain float64 solve in the reduction's order misses refine_tol, one
    # refinement step with the same solve brings it below
    refine_tol = 1e-11
    perm = np.argsort(plan.pos)
    Kp, f = K[np.ix_(perm, perm)], probs[1].q[perm]
    s0 = _level_one_solve(Kp, f)
    assert _normwise(Kp, s0, f) > refine_tol
    s1 = s0 + _level_one_solve(Kp, f - Kp @ s0)
    assert _normwise(Kp, s1, f) <= refine_tol
    ref, plain = refined_solve(K, probs[1].q)
    assert G.rel_err(plain, ref) < 1e-11
    bd = _batch(probs, "Full")
    assert bd.repaired() == 0
    st, nn, df = bd.step_local()
    x, _ = bd.points()
    print(f"status {st}, repaired {bd.repaired()}, x error {G.rel_err(x[1], -ref):.3e}")
    # (a tiny positive diagonal entry beside off-diagonal ones: K is indefinite, and the inertia
    # the reduction counts is that of K)
    neg = int((np.linalg.eigvalsh(K) < 0).sum())
    assert neg == 1 and not st.any() and list(nn) == [0, neg, 0]
    assert bd.repaired() >= 1
    assert G.rel_err(x[1], -ref) <= TOL
    assert abs(df[1] - np.linalg.norm(ref)) <= 1e-9 * np.linalg.norm(ref)
    for i in (0, 2):
        Ki = probs[i].hess_sparse().toarray() + np.eye(n)
        assert G.rel_err(x[i], -np.linalg.solve(Ki, probs[i].q)) <= TOL
    # the step after a repair: from the repaired point, evaluated afresh
    st, _, _ = bd.step_local()
    x2, _ = bd.points()
    assert not st.any() and G.rel_err(x2[1], -ref) <= TOL
    bd.close()


# ------------------------------------------------------------------ 10: refusals
def test_what_a_band_batch_refuses(pgf):
    from pygradflow_amd import _lib, problems

    n = 300
    d = 2.5 + np.random.default_rng(3).uniform(0.0, 0.5, n)
    with pytest.raises(ValueError, match="dense and banded"):
        _batch([_forced(problems.box_qp(n, seed=1)), problems.box_qp(n, seed=2, dense=True)], "Full")
    with pytest.raises(ValueError, match="dense and banded"):
        _batch([problems.box_qp(n, seed=2, dense=True), _forced(problems.box_qp(n, seed=1))], "Full")
    with pytest.raises(ValueError, match="one sparsity pattern"):
        _batch([_forced(problems.box_qp(n, seed=1)), _forced(band_problem(n, d, 1, 3))], "Full")
    wide = [_forced(problems.multistate_ocp(50, 8, 4, seed=i)) for i in range(2)]
    assert plan_of(wide[0]).block_size > 8
    with pytest.raises(ValueError, match="wide band"):
        _batch(wide, "Full")
    with pytest.raises(ValueError, match="bordered band"):
        _batch([bordered_lq(100, 3, 10, 1, 1, seed=i) for i in range(2)], "Full")
    with pytest.raises(ValueError, match=r"one \(n, m\)"):
        _batch([_forced(problems.box_qp(n, seed=1)), _forced(problems.box_qp(n + 1, seed=1))], "Full")
    bd = _batch([_forced(problems.box_qp(n, seed=i)) for i in range(2)], "Full")
    with pytest.raises(NotImplementedError, match="dense batch only"):
        bd.ctl_init(pgf.Params())
    lib = _lib.load()
    vals = np.ones(8)
    assert lib.pgf_batch_ctl_init(bd._b, 1.0, 1.0, _lib.dptr(vals), 4) == _lib.PGF_INVALID
    assert b"controller" in lib.pgf_batch_last_error(bd._b)
    assert lib.pgf_batch_ctl_iterate(bd._b, 3, float("nan"), 1) == _lib.PGF_INVALID
    assert lib.pgf_batch_ctl_read(bd._b, None, None, None, 0) == _lib.PGF_INVALID
    assert lib.pgf_batch_debug_fail_next_helper(bd._b) == _lib.PGF_INVALID
    assert lib.pgf_batch_debug_factor_kind(bd._b) == 0
    st, _, _ = bd.step_local()  # and the batch is none the worse for it
    assert not st.any() and bd.factor_kind() == 0
    bd.close()


# ------------------------------------------------------------------ 11: measures and norms
def test_measures_and_norms_as_one_by_one(pgf):
    probs = [_ocp(10 + i) for i in range(3)]
    bd, ref = _batch(probs, "Full"), _batch(probs, "Full", sequential=True)

    def close(a, b):
        return np.all(np.abs(a - b) <= 1e-13 * np.abs(b))

    for k in range(2):
        assert close(bd.residual_norms_local(), ref.residual_norms_local()), k
        assert close(bd.measures(), ref.measures()), k
        _same_step(bd, ref, k)
    assert close(bd.measures(), ref.measures()) and close(bd.residual_norms_local(), ref.residual_norms_local())
    assert bd.measures()[:, 3].max() > 0.0  # (multipliers have moved: the measures are not all zero)
    # the stream the launches went to is the batch's own
    s = C.c_void_p()
    assert bd._lib.load().pgf_batch_stream(bd._b, C.byref(s)) == 0 and s.value
    bd.close()
    ref.close()
