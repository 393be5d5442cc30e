"""Narrow banded path (half-bandwidths 1 .. 10, csrc/pgf_sparse.hip and the automatic routing of
bw 9 .. 10) against the CPU oracle, on every route a problem can take into it.

Bars as in test_gpu_parity.py: masks bit-identical, x and y within 1e-10 relative, n_neg = m.
The launch-plan switches of the 8 x 8 reduction (read once per process) run in child processes:
tests/test_gpu_schedules.py, tests/check_band.py.

The banded path exposes no factorisation counter.  That the second Simplified step is a back-solve
step is checked through its result where the test says so (section A, two Simplified steps, with
simplified_mask_goes_stale asserted: the active set at the point after step one differs from the
one the policy keeps, so a refactorisation with the current mask would miss the oracle).  The
single Simplified step of the other cases is the factorising first step and checks no such thing.
"""

import numpy as np
import pytest
import scipy.sparse as sps

from tests import golden_util as G
from tests.band_util import (SWEEP_BOX, SWEEP_OCP, TOL, _against_oracle, band_problem, forced,
                             head_of_first_eliminated, mask_changes, plan_of, refined_solve,
                             simplified_mask_goes_stale)

pytestmark = pytest.mark.gpu


def _rebound(prob, lb, ub):
    """The same linear-quadratic problem with other bounds."""
    from pygradflow_amd import problems

    return forced(problems.LinearQuadraticProblem(prob.hess_sparse(), prob.q, prob.jac_sparse(), prob.b,
                                                   lb, ub))


# ------------------------------------------------------------------ A: bw 9, 10, automatic route
@pytest.mark.parametrize("W", [9, 10])
def test_auto_route_unconstrained_churning_mask(pgf, W):
    from pygradflow_amd import problems

    prob = forced(problems.grid_box_qp(W, 60))
    plan = plan_of(prob)
    assert plan.bw in (9, 10) and plan.block is None
    assert mask_changes(prob, "Full", 3) > 0 and mask_changes(prob, "ActiveSet", 3) > 0
    assert simplified_mask_goes_stale(prob)
    churn = _against_oracle(pgf, prob, (("Full", 3), ("ActiveSet", 2), ("Simplified", 2)), n_neg=0)
    assert churn > 0


@pytest.mark.parametrize("shape", [(50, 4, 1), (400, 4, 2)])
def test_auto_route_constrained_indefinite(pgf, shape):
    from pygradflow_amd import problems

    prob = forced(problems.multistate_ocp(*shape))
    plan = plan_of(prob)
    assert plan.bw in (9, 10) and plan.block is None
    assert simplified_mask_goes_stale(prob)
    churn = _against_oracle(pgf, prob, (("Full", 3), ("Simplified", 2)), n_neg=prob.num_cons)
    assert churn > 0  # the control bounds are met


@pytest.mark.parametrize("W,L", [(9, 155), (9, 156), (9, 320), (10, 118), (10, 119), (10, 300)])
def test_auto_route_around_the_walk_panel(pgf, W, L):
    """N = 1395, 1404, 2880 and 1180, 1190, 3000 on the B = 16 reduction: just below, just above
    and well above what was one LDS panel of the retired sequential band walk (1396 rows at ldb 10,
    1181 at ldb 12), the route these bandwidths once took."""
    from pygradflow_amd import problems

    prob = forced(problems.grid_box_qp(W, L, seed=L))
    assert plan_of(prob).bw in (9, 10)
    churn = _against_oracle(pgf, prob, (("Full", 2), ("Simplified", 1)), n_neg=0)
    assert churn > 0


@pytest.mark.parametrize("bound", [0.0, np.inf])
def test_auto_route_all_and_none_active(pgf, bound):
    from pygradflow_amd import problems

    prob = forced(problems.grid_box_qp(9, 60, seed=2, bound=bound))
    assert plan_of(prob).bw in (9, 10)
    _against_oracle(pgf, prob, (("Full", 2), ("Simplified", 1)), n_neg=0)
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(540), np.zeros(0), 1.0, 1.0)
    dn.step()
    assert dn.mask().all() if bound == 0.0 else not dn.mask().any()
    dn.close()


def _linear_solver_view(pgf, prob, seed, with_rcond):
    n, m = prob.num_vars, prob.num_cons
    params = pgf.Params(newton_type="Full", step_solver=pgf.HipStepSolver, report_rcond=with_rcond)
    it = pgf.Iterate(prob, params, np.zeros(n), np.zeros(m))
    sv = pgf.HipStepSolver(prob, params, it, 1.0, 1.0)
    assert sv.sparse
    sv.update_active_set(sv.func.compute_active_set(it, 1.0))
    sv.update_derivs(it)
    res = sv.solve(it)
    assert sv._hd.plan.bw in (9, 10) and sv._hd.plan.block is None
    K = sv._host_reduced_kkt().toarray()
    cond = np.linalg.cond(K)
    assert cond < 1e5
    if with_rcond:
        assert res.rcond is not None and 0.2 / cond <= res.rcond <= 5.0 / cond
    rng = np.random.default_rng(seed)
    rhs = rng.standard_normal(K.shape[0])
    for trans, mat in ((False, K), (True, K.T)):
        ref, plain = refined_solve(mat, rhs)
        # the float64 reference is itself two orders below the bar: 1e-10 tests the kernel
        assert G.rel_err(plain, ref) < 1e-11
        assert G.rel_err(sv.solver.solve(rhs, trans=trans), ref) <= TOL
    assert sv.solver.num_neg_eigvals() == int((np.linalg.eigvalsh(K) < 0).sum()) == m
    sv.close()


def test_auto_route_exposes_linear_solver_and_rcond(pgf):
    from pygradflow_amd import problems

    _linear_solver_view(pgf, forced(problems.grid_box_qp(9, 60, seed=3)), 1, True)  # m = 0
    _linear_solver_view(pgf, forced(problems.multistate_ocp(50, 4, 1, seed=3)), 2, True)


# ------------------------------------------------------------------ B: the guard at bw 9, 10
def _block_in_use(prob):
    plan = plan_of(prob)
    assert plan.bw in (9, 10) and plan.block is None
    return plan.block_size


def _badly_placed(prob):
    """Variable whose diagonal entry the route in use takes as a pivot as it stands: the head of
    block 1 of the cyclic reduction (inverted unpivoted by level one)."""
    return head_of_first_eliminated(prob, _block_in_use(prob))


@pytest.mark.parametrize("bw", [9, 10])
def test_narrow_unstable_pivot_is_refined(pgf, bw):
    n = 300
    eps = 1e-9
    rng = np.random.default_rng(7)
    d = 2.5 + rng.uniform(0.0, 0.5, n)
    v = _badly_placed(forced(band_problem(n, d, 1, bw)))
    d[v] = -1.0 + eps  # lambda = 1: K[v, v] = eps
    prob = forced(band_problem(n, d, 1, bw))
    block = _block_in_use(prob)
    K = prob.hess_sparse().toarray() + np.eye(n)
    assert abs(K[v, v]) < 1e-8 and np.linalg.cond(K) < 1e5
    params = pgf.Params(newton_type="Full")
    it = pgf.Iterate(prob, params, np.zeros(n), np.zeros(0))
    sv = pgf.HipStepSolver(prob, params, it, 1.0, 1.0)
    assert sv.sparse
    sv.update_active_set(np.zeros(n, dtype=bool))
    sv.update_derivs(it)
    before = sv.refinement_stats()
    res = sv.solve(it)
    after = sv.refinement_stats()
    assert sv._hd.plan.block_size == block
    F = sv.func.value_at(it, 1.0, np.zeros(n, dtype=bool))
    s = np.linalg.solve(K, F)
    print(f"bw {bw} block {block} v {v}: refined {before[0]} -> {after[0]}, last_rel_residual {after[2]:.3e}, "
          f"dx error {G.rel_err(res.dx, s):.3e}")
    assert after[0] > before[0], "the guard did not refine"
    assert after[2] <= 1e-11
    assert G.rel_err(res.dx, s) <= 1e-9
    rhs = np.arange(1.0, n + 1.0)
    assert G.rel_err(sv.solver.solve(rhs), np.linalg.solve(K, rhs)) <= 1e-9
    sv.close()
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(n), np.zeros(0), 1.0, 1.0)
    dn.step()
    x, _ = dn.point()
    assert G.rel_err(x, -s) <= 1e-9
    dn.close()


@pytest.mark.parametrize("bw", [9, 10])
def test_narrow_not_quasi_definite_is_a_step_solver_error(pgf, bw):
    """K[v, v] = 0 exactly where the route in use pivots on it as it stands: the matrix is regular
    but not quasi-definite, and the unpivoted solve must say so rather than step."""
    from pygradflow_amd.errors import StepSolverError

    n = 300
    rng = np.random.default_rng(8)
    d = 2.5 + rng.uniform(0.0, 0.5, n)
    v = _badly_placed(forced(band_problem(n, d, 2, bw)))
    d[v] = -1.0
    prob = forced(band_problem(n, d, 2, bw))
    K = prob.hess_sparse().toarray() + np.eye(n)
    assert K[v, v] == 0.0 and np.linalg.cond(K) < 1e6
    params = pgf.Params(newton_type="Full")
    it = pgf.Iterate(prob, params, np.zeros(n), np.zeros(0))
    sv = pgf.HipStepSolver(prob, params, it, 1.0, 1.0)
    sv.update_active_set(np.zeros(n, dtype=bool))
    sv.update_derivs(it)
    with pytest.raises(StepSolverError):
        sv.solve(it)
    sv.close()


def test_device_newton_after_the_plugin_solver_on_a_pooled_handle(pgf):
    """DeviceNewton on problem A, then HipStepSolver on problem B of the same shape (same pooled
    handle: H, J of B become resident, q and b do not), then DeviceNewton on B: it must send B's q
    rather than step with A's.  (Found by test_narrow_unstable_pivot_is_refined[10] running after
    [9].)"""
    n = 300
    d = 2.5 + np.random.default_rng(11).uniform(0.0, 0.5, n)
    A, B = forced(band_problem(n, d, 21, 9)), forced(band_problem(n, d, 22, 9))
    x0, y0 = np.zeros(n), np.zeros(0)
    dn = pgf.DeviceNewton(A, "Full", x0, y0, 1.0, 1.0)
    dn.step()
    handle = dn._hd
    dn.close()
    params = pgf.Params(newton_type="Full")
    it = pgf.Iterate(B, params, x0, y0)
    sv = pgf.HipStepSolver(B, params, it, 1.0, 1.0)
    assert sv._hd is handle
    sv.update_active_set(np.zeros(n, dtype=bool))
    sv.update_derivs(it)
    sv.solve(it)
    sv.close()
    dn = pgf.DeviceNewton(B, "Full", x0, y0, 1.0, 1.0)
    assert dn._hd is handle
    dn.step()
    x, _ = dn.point()
    K = B.hess_sparse().toarray() + np.eye(n)
    assert G.rel_err(x, -np.linalg.solve(K, B.q)) <= TOL
    dn.close()


# ------------------------------------------------------------------ D: edges of the 8 x 8 reduction
def _sweep_problem(kind, size):
    from pygradflow_amd import problems

    prob = problems.box_qp(size, seed=size) if kind == "box" else problems.sparse_ocp(size, seed=size)
    return forced(prob)


@pytest.mark.parametrize("kind,size", [("box", n) for n in SWEEP_BOX] + [("ocp", m) for m in SWEEP_OCP])
def test_block_counts_on_every_branch_of_the_launch_plan(pgf, kind, size):
    """nb = ceil(N / 8) blocks against the branches of sp_launch_bcr_solve (computed on the CPU from
    its loop, band_util.bcr_launch_plan; "single" one level per launch, "pair" two, "tail" the
    blocks the LDS tail starts with):

      box_qp n      N%8  nb   levels before the tail                tail
      1, 7, 8       1,7,0  1  --                                    1 (single block, N < 8, N = 8)
      9             1      2  --                                    2
      255, 256      7,0   32  --                                    32 (the most the tail takes)
      257, 263, 264 1,7,0 33  single(left 33, 16 eliminated: odd)   17
      265           1     34  single(34, 17)                        17
      511, 512      7,0   64  single(64, 32)                        32
      513, 520      1,0   65  pair(65: odd, 16 workgroups)          17
      1024          0    128  pair(128, 32)                         32
      1025, 1031    1,7  129  pair(129, 32) + single(s = 4, 33, 16) 17
      1033          1    130  pair(130, 33: the last workgroup's j  17
                              lies beyond nb) + single(s = 4)
      sparse_ocp m  (N = 3 m)
      1, 2          3,6    1  --                                    1
      3, 11         1,1  2,5  --                                    2, 5 (odd)
      85            7     32  --                                    32
      86            2     33  single(33, 16)                        17
      171, 172      1,4   65  pair(65, 16)                          17
      342, 343      2,5  129  pair(129, 32) + single(s = 4, 33, 16) 17

    tests/check_band.py --sweep runs the same sizes with PGF_BCR_PAIRS=0 and PGF_BCR_FUSED=0 (every
    pair above becomes two single levels: 65 and 128 blocks single(s = 1) + single(s = 2), 129 and
    130 three single levels) and with PGF_BCR_PAIR_MAX=128, the mixed plan: up to 128 blocks as
    above, 129 and 130 blocks single(s = 1) + pair(s = 2) and 17 blocks in the tail, i.e.
    k_bcr_level2 entered at stride 2 and k_bcr_back2 run before k_bcr_back.  (PGF_BCR_PAIR_MAX=64
    would pair nothing: a pair needs more than 32 blocks left after its first level, hence more
    than 64 before it.)

    The launch guards ne > 0 and nj > 0 cannot be false: a level is only entered with st < nb
    (ne >= 1), a pair only with 2 st < nb (nj >= 1); no size reaches them."""
    prob = _sweep_problem(kind, size)
    plan = plan_of(prob)
    assert plan.block_size == 8 and plan.bw <= 8
    _against_oracle(pgf, prob, (("Full", 2), ("Simplified", 1)), n_neg=prob.num_cons)


def _bandwidth_case(bw):
    from pygradflow_amd import problems

    if bw in (2, 3, 4):
        n = 300
        d = 2.5 + np.random.default_rng(bw).uniform(0.0, 0.5, n)
        return band_problem(n, d, bw, bw, lb=np.full(n, -0.2), ub=np.full(n, 0.2))
    return {1: lambda: problems.box_qp(300, seed=1), 5: lambda: problems.grid_box_qp(5, 40),
            6: lambda: problems.multistate_ocp(50, 2, 1), 7: lambda: problems.multistate_ocp(50, 3, 1),
            8: lambda: problems.multistate_ocp(400, 3, 2)}[bw]()


@pytest.mark.parametrize("bw", [1, 2, 3, 4, 5, 6, 7, 8])
def test_every_bandwidth_up_to_8(pgf, bw):
    prob = forced(_bandwidth_case(bw))
    plan = plan_of(prob)
    assert plan.bw == bw and plan.block_size == 8
    churn = _against_oracle(pgf, prob, (("Full", 2), ("Simplified", 1)), n_neg=prob.num_cons)
    assert churn > 0


def _base(m_positive):
    from pygradflow_amd import problems

    if m_positive:
        return problems.multistate_ocp(60, 3, 1, seed=4)  # bw 7, N = 420
    n = 500
    return band_problem(n, 2.5 + np.random.default_rng(5).uniform(0.0, 0.5, n), 5, 5)


@pytest.mark.parametrize("m_positive", [False, True])
def test_mixed_bounds(pgf, m_positive):
    """Per variable in turn: only an upper bound, only a lower one, both, none."""
    base = _base(m_positive)
    n = base.num_vars
    k = np.arange(n) % 4
    lb = np.where((k == 1) | (k == 2), -0.15, -np.inf)
    ub = np.where((k == 0) | (k == 2), 0.1, np.inf)
    prob = _rebound(base, lb, ub)
    assert plan_of(prob).block_size == 8
    churn = _against_oracle(pgf, prob, (("Full", 2), ("Simplified", 1)), n_neg=prob.num_cons)
    assert churn > 0


@pytest.mark.parametrize("m_positive", [False, True])
def test_start_exactly_on_a_bound(pgf, m_positive):
    base = _base(m_positive)
    n = base.num_vars
    k = np.arange(n) % 3
    lb, ub = np.full(n, -0.2), np.full(n, 0.25)
    x0 = np.where(k == 0, lb, np.where(k == 1, ub, 0.0))
    prob = _rebound(base, lb, ub)
    assert plan_of(prob).block_size == 8
    churn = _against_oracle(pgf, prob, (("Full", 2), ("Simplified", 1)), n_neg=prob.num_cons, x0=x0)
    assert churn > 0


@pytest.mark.parametrize("m_positive", [False, True])
def test_fixed_variables(pgf, m_positive):
    """lb == ub for every fifth variable (started there), a box for the others."""
    base = _base(m_positive)
    n = base.num_vars
    fixed = np.arange(n) % 5 == 0
    lb = np.where(fixed, 0.125, -0.3)
    ub = np.where(fixed, 0.125, 0.3)
    prob = _rebound(base, lb, ub)
    assert plan_of(prob).block_size == 8
    churn = _against_oracle(pgf, prob, (("Full", 2), ("Simplified", 1)), n_neg=prob.num_cons,
                            x0=np.where(fixed, 0.125, 0.0))
    assert churn > 0


def test_singular_matrix_is_an_error_and_the_handle_survives(pgf):
    """m = 0, one variable decoupled with H[v, v] = -lambda: K has a zero row, every elimination
    order meets the exact zero pivot.  N = 600 is 75 blocks: a paired level before the tail.  The
    solve must come back with StepSolverError (a status, not a device fault), and the same pooled
    handle must then solve a well-posed problem of the same shape."""
    from pygradflow_amd import problems
    from pygradflow_amd.errors import StepSolverError

    n, v = 600, 333
    good = band_problem(n, 2.5 + np.random.default_rng(9).uniform(0.0, 0.5, n), 3, 5)
    H = sps.lil_matrix(good.hess_sparse())
    H[v, :] = 0.0
    H[:, v] = 0.0
    H[v, v] = -1.0
    bad = forced(problems.LinearQuadraticProblem(sps.csr_matrix(H), good.q, good.jac_sparse(), good.b,
                                                  good.var_lb, good.var_ub))
    K = bad.hess_sparse().toarray() + np.eye(n)
    assert not K[v].any() and plan_of(bad).block_size == 8
    params = pgf.Params(newton_type="Full")
    it = pgf.Iterate(bad, params, np.zeros(n), np.zeros(0))
    sv = pgf.HipStepSolver(bad, params, it, 1.0, 1.0)
    assert sv.sparse
    sv.update_active_set(np.zeros(n, dtype=bool))
    sv.update_derivs(it)
    with pytest.raises(StepSolverError):
        sv.solve(it)
    handle = sv._hd
    sv.close()
    dn = pgf.DeviceNewton(bad, "Full", np.zeros(n), np.zeros(0), 1.0, 1.0)
    assert dn._hd is handle
    with pytest.raises(StepSolverError):
        dn.step()
    dn.close()
    dn = pgf.DeviceNewton(forced(good), "Full", np.zeros(n), np.zeros(0), 1.0, 1.0)
    assert dn._hd is handle
    _, nn = dn.step()
    x, _ = dn.point()
    Kg = good.hess_sparse().toarray() + np.eye(n)
    assert nn == 0 and G.rel_err(x, -np.linalg.solve(Kg, good.q)) <= TOL
    dn.close()
    _against_oracle(pgf, forced(good), (("Full", 2), ("Simplified", 1)), n_neg=0)
