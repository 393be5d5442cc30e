"""Wide block cyclic reduction of the banded path (half-bandwidths up to 64, B x B blocks with
B in {16, 32, 64}, csrc/pgf_band_wide.hip) against the committed goldens and the CPU oracle.

Bars as in test_gpu_parity.py: masks bit-identical, x and y within 1e-10 relative.
"""

import numpy as np
import pytest

from oracle import newton_oracle as O
from tests import golden_util as G
from tests.band_util import TOL, _against_oracle, _as_sparse_lq, head_of_first_eliminated, wide_band_problem

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ A: the goldens
@pytest.mark.parametrize("block", [16, 32, 64])
@pytest.mark.parametrize("name", ["ocp_m40", "box_qp_n256", "boxed_qp49"])
def test_wide_blocks_golden(pgf, name, block):
    case = G.load_case(name)
    problem = _as_sparse_lq(G.rebuild_problem(case), block)
    dt, rho, tau = float(case["dt"]), float(case["rho"]), G.case_tau(case)
    for pol in case["policies"]:
        params = pgf.Params(newton_type=str(pol), step_solver=pgf.HipStepSolver)
        orig = pgf.Iterate(problem, params, case["x0"], case["y0"])
        gen = pgf.newton_steps(problem, params, orig, dt, rho, tau)
        dn = pgf.DeviceNewton(problem, str(pol), case["x0"], case["y0"], dt, rho, tau)
        assert dn.sparse and dn._hd.plan.block_size == block
        for k in range(int(case["steps"])):
            pre = f"{pol}/{k}/"
            step = next(gen)
            assert np.array_equal(step.active_set, case[pre + "mask"]), (pol, k)
            assert G.rel_err(step.iterate.x, case[pre + "xn"]) <= TOL, (pol, k)
            assert G.rel_err(step.iterate.y, case[pre + "yn"]) <= TOL, (pol, k)
            diff, n_neg = dn.step()
            x, y = dn.point()
            assert np.array_equal(dn.mask(), case[pre + "mask"]), (pol, k)
            assert G.rel_err(x, case[pre + "xn"]) <= TOL, (pol, k)
            assert G.rel_err(y, case[pre + "yn"]) <= TOL, (pol, k)
            assert abs(diff - float(case[pre + "diff"])) <= TOL * max(1.0, diff)
            assert n_neg == int(case[pre + "n_neg"])
        dn.close()


# ------------------------------------------------------------------ B: multi-state OCP
@pytest.mark.parametrize("shape,block", [((400, 8, 4), 32), ((300, 16, 8), 64), ((250, 20, 10), 64)])
def test_multistate_ocp_against_oracle(pgf, shape, block):
    from pygradflow_amd import problems
    from pygradflow_amd.sparse import BandPlan

    prob = problems.multistate_ocp(*shape)
    prob.pgf_force_band = True
    n, m = prob.num_vars, prob.num_cons
    assert BandPlan(prob.hess_sparse(), prob.jac_sparse(), n, m).block_size == block
    churn = _against_oracle(pgf, prob, (("Full", 3), ("Simplified", 2), ("ActiveSet", 3)), n_neg=m)
    assert churn > 0  # the control bounds are met


# ------------------------------------------------------------------ C: beyond the dense limit
def test_multistate_ocp_beyond_dense_limit(pgf):
    from pygradflow_amd import problems

    prob = problems.multistate_ocp(5000, 8, 4)  # N = 100 000, bw 22: B = 32
    m = prob.num_cons
    churn = _against_oracle(pgf, prob, (("Full", 3),), n_neg=m)
    assert churn > 10000


# ------------------------------------------------------------------ D: 2-D grid strip
def test_grid_box_qp_against_oracle(pgf):
    from pygradflow_amd import problems

    prob = problems.grid_box_qp(40, 2000)  # N = 80 000, bw 41: B = 64
    churn = _against_oracle(pgf, prob, (("Full", 6),), step_solver=False, n_neg=0)
    assert churn > 0


# ------------------------------------------------------------------ E: edges
@pytest.mark.parametrize("T", [1, 3, 4, 5, 47, 48, 52])
def test_block_counts(pgf, T):
    """multistate_ocp(T, 4, 2): N = 10 T, forced B = 16 -> 1, 2, 3, 4, 30, 30, 33 blocks (the
    single block N <= B, the last-block kernel with 1 .. 3 blocks, powers of two around 32)."""
    from pygradflow_amd import problems

    prob = problems.multistate_ocp(T, 4, 2, seed=T)
    prob.pgf_force_band = True
    prob.pgf_band_block = 16
    _against_oracle(pgf, prob, (("Full", 2), ("Simplified", 1)), n_neg=prob.num_cons)


@pytest.mark.parametrize("block", [32, 64])
def test_single_block(pgf, block):
    from pygradflow_amd import problems

    prob = problems.multistate_ocp(2, 6, 3, seed=5)  # N = 30 <= B
    prob.pgf_force_band = True
    prob.pgf_band_block = block
    _against_oracle(pgf, prob, (("Full", 2),), n_neg=prob.num_cons)


def test_all_variables_active(pgf):
    from pygradflow_amd import problems

    prob = problems.grid_box_qp(20, 30, seed=2, bound=0.0)
    prob.pgf_force_band = True
    prob.pgf_band_block = 32
    _against_oracle(pgf, prob, (("Full", 2),))
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(600), np.zeros(0), 1.0, 1.0)
    dn.step()
    assert dn.mask().all()
    dn.close()


@pytest.mark.parametrize("block", [16, 32, 64])
def test_unconstrained_forced_block(pgf, block):
    from pygradflow_amd import problems

    prob = problems.grid_box_qp(12, 50, seed=1, bound=0.4)  # m = 0, bw 12
    prob.pgf_force_band = True
    prob.pgf_band_block = block
    _against_oracle(pgf, prob, (("Full", 3), ("ActiveSet", 2)), n_neg=0)


# ------------------------------------------------------------------ F: LinearSolver view
@pytest.mark.parametrize("block", [32, 64])
def test_wide_factor_exposes_linear_solver_and_rcond(pgf, block):
    case = G.load_case("box_qp_n256")
    problem = _as_sparse_lq(G.rebuild_problem(case), block)
    dt, rho = float(case["dt"]), float(case["rho"])
    params = pgf.Params(newton_type="Full", step_solver=pgf.HipStepSolver, report_rcond=True)
    it = pgf.Iterate(problem, params, case["x0"], case["y0"])
    sv = pgf.HipStepSolver(problem, params, it, dt, rho)
    assert sv.sparse
    sv.update_active_set(sv.func.compute_active_set(it, rho))
    sv.update_derivs(it)
    res = sv.solve(it)
    assert sv._hd.plan.block_size == block
    K = sv._host_reduced_kkt().toarray()
    cond = np.linalg.cond(K)
    assert res.rcond is not None and 0.2 / cond <= res.rcond <= 5.0 / cond
    rng = np.random.default_rng(block)
    rhs = rng.standard_normal(K.shape[0])
    assert G.rel_err(sv.solver.solve(rhs), np.linalg.solve(K, rhs)) <= 1e-10
    assert G.rel_err(sv.solver.solve(rhs, trans=True), np.linalg.solve(K.T, rhs)) <= 1e-10
    sv.close()
    # with constraints: the multi-state OCP (indefinite, n_neg = m)
    from pygradflow_amd import problems

    problem = problems.multistate_ocp(30, 6, 3, seed=3)
    problem.pgf_force_band = True
    problem.pgf_band_block = block
    params = pgf.Params(newton_type="Full", step_solver=pgf.HipStepSolver)
    x0, y0 = np.zeros(problem.num_vars), np.zeros(problem.num_cons)
    it = pgf.Iterate(problem, params, x0, y0)
    sv = pgf.HipStepSolver(problem, params, it, 1.0, 1.0)
    sv.update_active_set(sv.func.compute_active_set(it, 1.0))
    sv.update_derivs(it)
    sv.solve(it)
    K = sv._host_reduced_kkt().toarray()
    rhs = rng.standard_normal(K.shape[0])
    assert G.rel_err(sv.solver.solve(rhs), np.linalg.solve(K, rhs)) <= 1e-10
    assert G.rel_err(sv.solver.solve(rhs, trans=True), np.linalg.solve(K.T, rhs)) <= 1e-10
    assert sv.solver.num_neg_eigvals() == int((np.linalg.eigvalsh(K) < 0).sum())
    sv.close()


# ------------------------------------------------------------------ G: the guard
@pytest.mark.parametrize("block", [16, 64])
def test_wide_unstable_pivot_is_refined(pgf, block):
    n = 300
    eps = 1e-9
    rng = np.random.default_rng(7)
    d = 2.5 + rng.uniform(0.0, 0.5, n)
    v = head_of_first_eliminated(wide_band_problem(n, d, 1, block), block)
    d[v] = -1.0 + eps  # lambda = 1: K[v, v] = eps
    prob = wide_band_problem(n, d, 1, block)
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


@pytest.mark.parametrize("block", [16, 64])
def test_not_quasi_definite_is_a_step_solver_error(pgf, block):
    """K[v, v] = 0 exactly at the head of a block inverted as it stands: the matrix is regular
    but not quasi-definite, and the unpivoted reduction must say so rather than step."""
    from pygradflow_amd.errors import StepSolverError

    n = 300
    rng = np.random.default_rng(8)
    d = 2.5 + rng.uniform(0.0, 0.5, n)
    v = head_of_first_eliminated(wide_band_problem(n, d, 2, block), block)
    d[v] = -1.0
    prob = wide_band_problem(n, d, 2, block)
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


# ------------------------------------------------------------------ H: limits
def test_beyond_bandwidth_64(pgf):
    from pygradflow_amd import problems

    prob = problems.multistate_ocp(300, 24, 8)  # bw 70
    prob.pgf_force_band = True
    n, m = prob.num_vars, prob.num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    with pytest.raises(NotImplementedError, match="64"):
        pgf.DeviceNewton(prob, "Full", x0, y0, 1.0, 1.0)
    recs = O.NewtonOracle(prob, "Full", x0, y0, 1.0, 1.0).run(x0, y0, 2)
    params = pgf.Params(newton_type="Full", step_solver=pgf.HipStepSolver)
    gen = pgf.newton_steps(prob, params, pgf.Iterate(prob, params, x0, y0), 1.0, 1.0)
    for k, rec in enumerate(recs):
        step = next(gen)
        assert np.array_equal(step.active_set, rec["mask"]), k
        assert G.rel_err(step.iterate.x, rec["xn"]) <= TOL and G.rel_err(step.iterate.y, rec["yn"]) <= TOL


def test_block_smaller_than_bandwidth_is_rejected(pgf):
    from pygradflow_amd import problems

    prob = problems.multistate_ocp(100, 8, 4)  # bw 22
    prob.pgf_force_band = True
    prob.pgf_band_block = 16
    n, m = prob.num_vars, prob.num_cons
    with pytest.raises(ValueError, match="block size"):
        pgf.DeviceNewton(prob, "Full", np.zeros(n), np.zeros(m), 1.0, 1.0)
    params = pgf.Params(newton_type="Full", step_solver=pgf.HipStepSolver)
    gen = pgf.newton_steps(prob, params, pgf.Iterate(prob, params, np.zeros(n), np.zeros(m)), 1.0, 1.0)
    with pytest.raises(ValueError, match="block size"):
        next(gen)
