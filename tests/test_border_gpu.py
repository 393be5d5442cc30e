"""Bordered band (a band plus up to 64 dense rows / columns of the KKT pattern: csrc/pgf_border.hip,
BandPlan(border=...)) against the CPU oracle.

Bars as in test_gpu_parity.py: masks bit-identical, x and y within 1e-10 relative, inertia m.
Shapes are the smallest that reach every kernel branch: Nb = 1003 band rows are 126 blocks of 8 --
no power of two, a padded last block, seven panel levels and the LDS tail of the single reduction
behind two of its level launches; k = 1 (kp = 16), 17 (kp = 32, variables and constraints, S not
diagonal) and 64 (the limit); remainders at B = 8 (panel reduction), 16 and 32 (repeated solves).
"""

import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sps

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__" and REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import newton_oracle as O  # noqa: E402
from tests import golden_util as G  # noqa: E402
from tests.band_util import TOL, _against_oracle  # noqa: E402

pytestmark = pytest.mark.gpu

CASE1_POLICIES = (("Full", 3), ("ActiveSet", 3), ("Simplified", 3))


def budget_case(n=1003, seed=0, border="auto"):
    """Tridiagonal H (diagonal in [1, 2], off-diagonal 0.2), one dense row uniform(0.5, 1.5), b = 0,
    q ~ N(0, 1), bounds +-0.5: problems.budget_box_qp."""
    from pygradflow_amd import problems

    prob = problems.budget_box_qp(n, seed)
    if border is not None:
        prob.pgf_border = border
    return prob


def oracle_run(prob, pol, steps, dt=1.0, rho=1.0):
    x0, y0 = np.zeros(prob.num_vars), np.zeros(prob.num_cons)
    return O.NewtonOracle(prob, pol, x0, y0, dt, rho).run(x0, y0, steps)


def device_trajectory(pgf, prob, policies):
    """(x, y) after every DeviceNewton step of the policies, from zero."""
    x0, y0 = np.zeros(prob.num_vars), np.zeros(prob.num_cons)
    out = []
    for pol, steps in policies:
        dn = pgf.DeviceNewton(prob, pol, x0, y0, 1.0, 1.0)
        for _ in range(steps):
            dn.step()
            out.extend(dn.point())
        dn.close()
    return out


# ------------------------------------------------------------------ 1: budget row, k = 1
def test_budget_row_against_oracle(pgf):
    prob = budget_case()
    n, m = prob.num_vars, prob.num_cons
    masks = [r["mask"] for r in oracle_run(prob, "Full", 3)]
    counts = [int(np.count_nonzero(mk)) for mk in masks]
    print("active counts", counts)
    assert any(not np.array_equal(a, b) for a, b in zip(masks, masks[1:]))  # the mask churns
    assert any(0.1 * n < c < 0.9 * n for c in counts)
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(n), np.zeros(m), 1.0, 1.0)
    plan = dn._hd.plan
    assert list(plan.border) == [n] and plan.bw == 1 and plan.block_size == 8 and plan.Nb == 1003
    assert dn.border_stats()[0] == 1
    dn.close()
    _against_oracle(pgf, prob, CASE1_POLICIES, n_neg=m)


# ------------------------------------------------------------------ 2: the factor is kept
def test_simplified_reuses_the_border_factor(pgf):
    prob = budget_case()  # a new problem object: the pattern (and the border) are uploaded anew
    n, m = prob.num_vars, prob.num_cons
    recs = oracle_run(prob, "Simplified", 3)
    dn = pgf.DeviceNewton(prob, "Simplified", np.zeros(n), np.zeros(m), 1.0, 1.0)
    assert dn.border_stats() == (1, 0, 0)
    for rec in recs:
        dn.step()
        x, y = dn.point()
        assert G.rel_err(x, rec["xn"]) <= TOL and G.rel_err(y, rec["yn"]) <= TOL
    k, factorisations, solves = dn.border_stats()
    dn.close()
    assert k == 1 and factorisations == 1 and solves >= 3, (k, factorisations, solves)


# ------------------------------------------------------------------ 3: panel reduction against repeated solves
def test_multi_rhs_against_repeated_solves(pgf, tmp_path):
    """Y = inv(B) C by the multi-right-hand-side reduction (this process) and by k single solves
    (PGF_BORDER_MULTI=0, read once per process: a fresh child): the child meets the oracle on its
    own, and the two routes agree to 1e-12."""
    out = str(tmp_path / "repeated.npz")
    env = dict(os.environ, PGF_BORDER_MULTI="0")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=REPO,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    theirs = np.load(out)
    ours = device_trajectory(pgf, budget_case(), CASE1_POLICIES)
    assert len(ours) == len(theirs.files) == 18
    for i, v in enumerate(ours):
        err = G.rel_err(v, theirs[f"a{i}"])
        assert err <= 1e-12, (i, err)


def _child(out):
    import pygradflow_amd as pgf

    assert os.environ.get("PGF_BORDER_MULTI") == "0"
    prob = budget_case()
    _against_oracle(pgf, prob, CASE1_POLICIES, n_neg=prob.num_cons)
    traj = device_trajectory(pgf, budget_case(), CASE1_POLICIES)
    np.savez(out, **{f"a{i}": v for i, v in enumerate(traj)})


# ------------------------------------------------------------------ 4: k = 17, mixed border
def mixed_border_case():
    """ocp_global_parameter(60, 4, 2, 3) and 14 dense constraint rows over all variables: the border
    holds 3 variables and 14 constraints, S is a full 17 x 17 matrix.  |p| <= 0.5 makes two of
    the parameters active at the oracle's first step."""
    from pygradflow_amd import problems

    base = problems.ocp_global_parameter(60, 4, 2, 3, pbound=0.5)
    n = base.num_vars
    rng = np.random.default_rng(7)
    A = sps.vstack([base.jac_sparse(), sps.csr_matrix(rng.uniform(-1, 1, (14, n)) / np.sqrt(n))],
                   format="csr")
    b = np.concatenate([base.b, 0.1 * rng.standard_normal(14)])
    prob = problems.LinearQuadraticProblem(base.hess_sparse(), base.q, A, b, base.var_lb, base.var_ub)
    prob.pgf_border = "auto"
    return prob


def test_mixed_border_k17(pgf):
    from pygradflow_amd.sparse import BandPlan

    prob = mixed_border_case()
    n, m = prob.num_vars, prob.num_cons
    plan = BandPlan(prob.hess_sparse(), prob.jac_sparse(), n, m, border="auto")
    assert plan.k == 17 and plan.kp == 32
    assert list(plan.border) == [n - 3, n - 2, n - 1] + [n + m - 14 + r for r in range(14)]
    assert 8 < plan.bw <= 16 and plan.block_size == 16  # too wide for the 8 x 8 reduction
    recs = oracle_run(prob, "Full", 3)
    assert any(rec["mask"][n - 3:].any() for rec in recs)      # a border variable is active ...
    assert any(not rec["mask"][n - 3:].all() for rec in recs)  # ... and one is not
    _against_oracle(pgf, prob, (("Full", 3),), n_neg=m)


# ------------------------------------------------------------------ 5: k = 64, the limit
def test_border_of_64_and_beyond(pgf):
    from pygradflow_amd import problems

    base = problems.budget_box_qp(520)
    rng = np.random.default_rng(5)
    A = sps.csr_matrix(rng.standard_normal((64, 520)) / np.sqrt(520))
    prob = problems.LinearQuadraticProblem(base.hess_sparse(), base.q, A, 0.1 * rng.standard_normal(64),
                                           base.var_lb, base.var_ub)
    prob.pgf_border = "auto"
    churn = _against_oracle(pgf, prob, (("Full", 2),), n_neg=64)
    assert churn > 0
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(520), np.zeros(64), 1.0, 1.0)
    assert dn.border_stats()[0] == 64 and dn._hd.plan.kp == 64
    dn.close()
    prob65 = problems.LinearQuadraticProblem(base.hess_sparse(), base.q, A, prob.b, base.var_lb, base.var_ub)
    prob65.pgf_border = list(range(520, 584)) + [0]
    with pytest.raises(ValueError):
        pgf.DeviceNewton(prob65, "Full", np.zeros(520), np.zeros(64), 1.0, 1.0)
    # the C ABI itself: k > 64 and dense handles are PGF_INVALID
    from pygradflow_amd import _lib

    lib = _lib.load()
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(520), np.zeros(64), 1.0, 1.0)
    assert lib.pgf_sparse_set_border(dn._hd.h, 65) == _lib.PGF_INVALID
    assert dn.border_stats()[0] == 64  # (refused: nothing changed)
    dn.close()
    dense = pgf.DeviceNewton(problems.dense_qp(8, 2, seed=0), "Full", np.zeros(8), np.zeros(2), 1.0, 1.0)
    assert lib.pgf_sparse_set_border(dense._hd.h, 1) == _lib.PGF_INVALID
    dense.close()


# ------------------------------------------------------------------ 6: wide remainder
def test_wide_remainder(pgf):
    from pygradflow_amd import problems

    prob = problems.ocp_global_parameter(100, 8, 4, 2)
    prob.pgf_border = "auto"
    n, m = prob.num_vars, prob.num_cons
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(n), np.zeros(m), 1.0, 1.0)
    plan = dn._hd.plan
    dn.close()
    assert list(plan.border) == [n - 2, n - 1] and plan.bw == 22 and plan.block_size == 32
    churn = _against_oracle(pgf, prob, (("Full", 2), ("Simplified", 2)), n_neg=m)
    assert churn > 0


# ------------------------------------------------------------------ 7: the guard covers the border
def test_guard_measures_the_full_bordered_residual(pgf):
    """No dt in [1e3, 1e8] makes the Schur-complement solve of a budget problem inaccurate -- B is
    symmetric positive definite and diagonally dominant, a float64 numpy restatement of the block
    elimination stays below 7e-17 relative residual (cond(K) = 23) -- so nothing
    is perturbed here: at dt = 1e5 the relative residual the guard reports for a linear solve
    (k_border_residual: all band rows, C z in them, and the border row) must be the residual of
    the full K at the returned solution, recomputed on the host, within a factor of 2."""
    prob = budget_case()
    n, m = prob.num_vars, prob.num_cons
    dt, rho = 1e5, 1.0
    rng = np.random.default_rng(3)
    mask = rng.uniform(size=n) < 0.4
    params = pgf.Params()
    it = pgf.Iterate(prob, params, np.zeros(n), np.zeros(m))
    sv = pgf.HipStepSolver(prob, params, it, dt, rho)
    assert sv.sparse
    sv.update_active_set(mask)
    sv.update_derivs(it)
    lamb = 1.0 / dt
    K = O.kkt_matrix(O.shifted_hess_rows(prob.hess_sparse(), lamb, mask), prob.jac_sparse().tocsc(), mask,
                     lamb, rho).toarray()
    rhs = rng.standard_normal(K.shape[0])
    view = sv.solver_for_tests()
    s = view.solve(rhs)
    refined, lu, rel_dev = sv.refinement_stats()
    assert sv.border_stats()[0] == 1
    assert view.num_neg_eigvals() == m
    sv.close()
    assert G.rel_err(s, np.linalg.solve(K, rhs)) <= TOL
    # the residual of the returned solution itself: accumulated in extended precision, as
    # band_util.refined_solve does (a float64 K @ s carries rounding of its own 600-term dense row
    # that is larger than the residual it is to measure)
    r = np.asarray(rhs.astype(np.longdouble) - K.astype(np.longdouble) @ s.astype(np.longdouble), dtype=np.float64)
    den = np.max(np.abs(K) @ np.abs(s) + np.abs(rhs))
    rel_host = np.max(np.abs(r)) / den
    print("relative residual: device", rel_dev, "host", rel_host, "host, float64 products",
          np.max(np.abs(rhs - K @ s)) / den)
    assert 0.0 < rel_dev <= 1e-11
    assert 0.5 * rel_host <= rel_dev <= 2.0 * rel_host, (rel_dev, rel_host)


# ------------------------------------------------------------------ 8: beyond the dense limit
def test_large_problem_is_rescued_by_an_automatic_border(pgf):
    """n + m = 70 001 > DENSE_MAX and one dense row: no band, no dense matrix -- refused before the
    border existed; now the step solver tries an automatic border before it gives up."""
    prob = budget_case(70_000, border=None)
    n, m = prob.num_vars, prob.num_cons
    rec = oracle_run(prob, "Full", 1)[0]
    params = pgf.Params(newton_type="Full", step_solver=pgf.HipStepSolver)
    step = next(pgf.newton_steps(prob, params, pgf.Iterate(prob, params, np.zeros(n), np.zeros(m)), 1.0, 1.0))
    assert np.array_equal(step.active_set, rec["mask"])
    assert G.rel_err(step.iterate.x, rec["xn"]) <= TOL
    assert G.rel_err(step.iterate.y, rec["yn"]) <= TOL
    assert 0.1 * n < np.count_nonzero(rec["mask"]) < 0.9 * n


# ------------------------------------------------------------------ 9: nothing changes without a border
def test_without_pgf_border_the_routes_are_unchanged(pgf):
    prob = budget_case(border=None)
    prob.pgf_force_band = True
    n, m = prob.num_vars, prob.num_cons
    with pytest.raises(NotImplementedError, match="64"):
        pgf.DeviceNewton(prob, "Full", np.zeros(n), np.zeros(m), 1.0, 1.0)
    params = pgf.Params(newton_type="Full", step_solver=pgf.HipStepSolver)
    method = pgf.newton_method(prob, params, pgf.Iterate(prob, params, np.zeros(n), np.zeros(m)), 1.0, 1.0)
    curr = pgf.Iterate(prob, params, np.zeros(n), np.zeros(m))
    for rec in oracle_run(prob, "Full", 2):
        step = method.step(curr)
        assert np.array_equal(step.active_set, rec["mask"])
        assert G.rel_err(step.iterate.x, rec["xn"]) <= TOL
        assert G.rel_err(step.iterate.y, rec["yn"]) <= TOL
        curr = step.iterate
    assert not method.step_solver.sparse  # it left the banded path for the dense one
    assert method.step_solver.border_stats() == (0, 0, 0)


if __name__ == "__main__":
    _child(sys.argv[1])
