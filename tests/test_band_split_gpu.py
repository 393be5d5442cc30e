"""Factor / solve split of the wide block cyclic reduction (B in {16, 32, 64},
csrc/pgf_band_wide.hip): the reduction keeps its factors, a solve on the same matrix runs the
solve phase against them -- one right-hand side (back-solve steps, LinearSolver.solve, refinement
corrections) or a panel of them (pgf_linear_solve_multi, Y of a bordered band).

Bars as in test_band_wide_gpu.py: masks identical, 1e-10 relative (band_util.TOL), 1e-9 in the
unstable-pivot cases; the split itself must not change a bit (np.array_equal against a solver
with ``pgf_band_split = False``).  The route is read from pgf_debug_band_stats (band_stats():
reductions, solve phases, panel solves), always as a difference: handles are pooled.
"""

import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__" and REPO not in sys.path:
    sys.path.insert(0, REPO)

from oracle import newton_oracle as O  # noqa: E402
from tests import golden_util as G  # noqa: E402
from tests.band_util import (TOL, _against_oracle, _as_sparse_lq, bordered_lq, head_of_first_eliminated,  # noqa: E402
                             mask_changes, multistate_ocp, plan_of, refined_solve, wide_band_problem)

pytestmark = pytest.mark.gpu


def _delta(after, before):
    return tuple(a - b for a, b in zip(after, before))


def _step_solver(pgf, prob, mask=None, dt=1.0, rho=1.0, newton_type="Full"):
    """HipStepSolver at the zero iterate with the active set of the residual function (or `mask`)."""
    params = pgf.Params(newton_type=newton_type, step_solver=pgf.HipStepSolver)
    it = pgf.Iterate(prob, params, np.zeros(prob.num_vars), np.zeros(prob.num_cons))
    sv = pgf.HipStepSolver(prob, params, it, dt, rho)
    assert sv.sparse
    sv.update_active_set(sv.func.compute_active_set(it, rho) if mask is None else mask)
    sv.update_derivs(it)
    return sv, it


# ------------------------------------------------------------------ 1: block-count edges
EDGE_CASES = [((T, 4, 2, T), 16) for T in (1, 3, 4, 5, 47, 48, 52)] + [
    ((2, 6, 3, 0), 32), ((2, 6, 3, 0), 64), ((30, 6, 3, 0), 32), ((30, 6, 3, 0), 64)]


@pytest.mark.parametrize("args,block", EDGE_CASES)
def test_block_count_edges(pgf, args, block):
    """multistate_ocp(T, 4, 2) at B = 16: 1, 2, 3, 4, 30, 30, 33 blocks -- the single block, a
    missing right neighbour at every level, powers of two on either side of 32; (2, 6, 3) and
    (30, 6, 3) at B = 32, 64.  Against the oracle, and the route of a Simplified trajectory: one
    reduction, then solve phases only."""
    prob = multistate_ocp(*args, block)
    n, m = prob.num_vars, prob.num_cons
    _against_oracle(pgf, prob, (("Full", 1), ("Simplified", 3)), n_neg=m)
    x0, y0 = np.zeros(n), np.zeros(m)
    recs = O.NewtonOracle(prob, "Simplified", x0, y0, 1.0, 1.0).run(x0, y0, 4)
    dn = pgf.DeviceNewton(prob, "Simplified", x0, y0, 1.0, 1.0)
    assert dn._hd.plan.block_size == block
    b0, r0 = dn.band_stats(), dn.refinement_stats()
    for k, rec in enumerate(recs):
        _, nn = dn.step()
        x, y = dn.point()
        assert nn == m, k  # a solve phase leaves the inertia the reduction reported
        assert G.rel_err(x, rec["xn"]) <= TOL and G.rel_err(y, rec["yn"]) <= TOL, k
    red, sol, pan = _delta(dn.band_stats(), b0)
    refined = dn.refinement_stats()[0] - r0[0]
    dn.close()
    assert red == 1 and pan == 0 and sol >= 3, (red, sol, pan)
    if refined == 0:
        assert sol == 3


# ------------------------------------------------------------------ 2: bit identity
@pytest.mark.parametrize("args,block", [((47, 4, 2, 47), 16), ((30, 6, 3, 0), 32), ((30, 6, 3, 0), 64)])
def test_split_returns_the_same_bits(pgf, args, block):
    """The KEEP reduction against today's reduction (res.dx, res.dy of the fused solve) and the
    solve phase against a whole reduction on the same right-hand side (solver.solve)."""
    rng = np.random.default_rng(block)
    out = {}
    for split in (True, False):
        prob = multistate_ocp(*args, block, split=split)
        sv, it = _step_solver(pgf, prob)
        b0 = sv.band_stats()
        res = sv.solve(it)
        rows = sv._host_reduced_kkt().shape[0]
        if "rhs" not in out:
            out["rhs"] = rng.standard_normal(rows)
        x1 = sv.solver.solve(out["rhs"])
        x2 = sv.solver.solve(out["rhs"], trans=True)
        red, sol, _ = _delta(sv.band_stats(), b0)
        assert sv._hd.plan.block_size == block
        sv.close()
        out[split] = (res.dx.copy(), res.dy.copy(), x1, x2)
        if split:
            assert red == 1 and sol >= 2, (red, sol)
        else:  # today's route: every solve a whole reduction
            assert sol == 0 and red >= 3, (red, sol)
    for a, b in zip(out[True], out[False]):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------ 3: invalidation
def test_active_set_changes_invalidate_the_kept_factors(pgf):
    """ActiveSet on grid_box_qp(12, 50) at B = 16, dt = 10: the oracle's mask changes on the first
    steps and then settles.  A step whose mask changed is a reduction, every other one a solve
    phase; a new outer step (new lambda) is a reduction again."""
    from pygradflow_amd import problems

    prob = problems.grid_box_qp(12, 50, seed=1, bound=0.4)
    prob.pgf_force_band = True
    prob.pgf_band_block = 16
    n, dt, steps = prob.num_vars, 10.0, 8
    x0, y0 = np.zeros(n), np.zeros(0)
    changes = mask_changes(prob, "ActiveSet", steps, dt=dt)
    assert 0 < changes < steps - 1  # some steps change the mask, some do not
    recs = O.NewtonOracle(prob, "ActiveSet", x0, y0, dt, 1.0).run(x0, y0, steps)
    dn = pgf.DeviceNewton(prob, "ActiveSet", x0, y0, dt, 1.0)
    assert dn._hd.plan.block_size == 16
    prev, seen = None, 0
    for k, rec in enumerate(recs):
        b0, r0 = dn.band_stats(), dn.refinement_stats()[0]
        dn.step()
        red, sol, _ = _delta(dn.band_stats(), b0)
        refined = dn.refinement_stats()[0] - r0
        x, _ = dn.point()
        assert np.array_equal(dn.mask(), rec["mask"]), k
        assert G.rel_err(x, rec["xn"]) <= TOL, k
        changed = prev is None or not np.array_equal(prev, rec["mask"])
        seen += int(changed and prev is not None)
        assert red == (1 if changed else 0), (k, changed, red, sol)
        if not changed:
            assert sol >= 1 and (refined or sol == 1), (k, sol, refined)
        prev = rec["mask"]
    assert seen == changes
    # the outer step advances with another dt: the matrix changes, the kept factors go
    xh, yh = dn.point()
    dn.advance_outer(dt=5.0)
    rec = O.NewtonOracle(prob, "ActiveSet", xh, yh, 5.0, 1.0).run(xh, yh, 1)[0]
    b0 = dn.band_stats()
    dn.step()
    red, sol, _ = _delta(dn.band_stats(), b0)
    x, _ = dn.point()
    mask = dn.mask()
    dn.close()
    assert red == 1, (red, sol)
    assert np.array_equal(mask, rec["mask"])
    assert G.rel_err(x, rec["xn"]) <= TOL


def test_new_values_invalidate_the_kept_factors(pgf):
    prob = multistate_ocp(30, 6, 3, 3, 32)
    sv, it = _step_solver(pgf, prob)
    b0 = sv.band_stats()
    res = sv.solve(it)
    rows = sv._host_reduced_kkt().shape[0]
    rhs = np.random.default_rng(5).standard_normal(rows)
    x1 = sv.solver.solve(rhs)
    assert _delta(sv.band_stats(), b0)[:2] == (1, 1)
    prob.Q = prob.Q.copy()  # an assignment: the resident values are stale and go up again
    sv.update_derivs(it)
    b1 = sv.band_stats()
    res2 = sv.solve(it)
    assert _delta(sv.band_stats(), b1)[0] == 1
    assert np.array_equal(res.dx, res2.dx) and np.array_equal(res.dy, res2.dy)
    K = sv._host_reduced_kkt().toarray()
    assert G.rel_err(x1, refined_solve(K, rhs)[0]) <= TOL
    assert G.rel_err(sv.solver.solve(rhs), refined_solve(K, rhs)[0]) <= TOL
    sv.close()


# ------------------------------------------------------------------ 4: panel solve
def _check_panels(sv, rng, counts):
    K = sv._host_reduced_kkt().toarray()
    rows = K.shape[0]
    for nrhs in counts:
        for trans in (False, True):
            rhs = rng.standard_normal((rows, nrhs))
            b0 = sv.band_stats()
            sol = sv.solver.solve(rhs, trans=trans)
            red, _, pan = _delta(sv.band_stats(), b0)
            assert sol.shape == (rows, nrhs)
            ref = refined_solve(K, rhs)[0]
            for j in range(nrhs):
                err = G.rel_err(sol[:, j], ref[:, j])
                assert err <= TOL, (nrhs, trans, j, err)
            assert pan == -(-nrhs // 64) and red == 0, (nrhs, red, pan)


@pytest.mark.parametrize("block", [16, 32, 64])
def test_panel_solve(pgf, block):
    """(rows, nrhs) right-hand sides through _DeviceFactorView.solve: panels of at most 64 columns
    against the factors the step left; 1, 2 (one tile of 16 columns, mostly padding), 16, 17, 64,
    65 (a second panel of one column)."""
    prob = multistate_ocp(30, 6, 3, 3, block)
    sv, it = _step_solver(pgf, prob)
    sv.solve(it)
    assert sv._hd.plan.block_size == block
    _check_panels(sv, np.random.default_rng(block), (1, 2, 16, 17, 64, 65))
    sv.close()


def test_panel_solve_factorises_on_its_own(pgf):
    """No step before the first 2-D solve: one factor-only reduction, then the panel."""
    case = G.load_case("box_qp_n256")
    prob = _as_sparse_lq(G.rebuild_problem(case), 32)
    sv, it = _step_solver(pgf, prob, dt=float(case["dt"]), rho=float(case["rho"]))
    view = sv.solver_for_tests()
    K = sv._host_reduced_kkt().toarray()
    rhs = np.random.default_rng(1).standard_normal((K.shape[0], 17))
    b0 = sv.band_stats()
    sol = view.solve(rhs)
    assert _delta(sv.band_stats(), b0) == (1, 0, 1)
    assert sv._hd.plan.block_size == 32
    ref = refined_solve(K, rhs)[0]
    assert max(G.rel_err(sol[:, j], ref[:, j]) for j in range(17)) <= TOL
    assert view.num_neg_eigvals() == 0
    sv.solver = view
    _check_panels(sv, np.random.default_rng(2), (1, 65))
    sv.close()


@pytest.mark.parametrize("kind", ["dense", "block8", "split_off"])
def test_multi_rhs_elsewhere_is_the_loop(pgf, kind):
    """Every other kind of handle: pgf_linear_solve column by column, bit for bit."""
    case = G.load_case("box_qp_n256")
    dense = G.rebuild_problem(case)
    if kind == "dense":
        prob = dense
    else:
        prob = _as_sparse_lq(dense, 32 if kind == "split_off" else None)
        if kind == "split_off":
            prob.pgf_band_split = False
    params = pgf.Params(newton_type="Full", step_solver=pgf.HipStepSolver)
    it = pgf.Iterate(prob, params, case["x0"], case["y0"])
    sv = pgf.HipStepSolver(prob, params, it, float(case["dt"]), float(case["rho"]))
    sv.update_active_set(sv.func.compute_active_set(it, float(case["rho"])))
    sv.update_derivs(it)
    sv.solve(it)
    assert sv.sparse == (kind != "dense")
    if sv.sparse:
        assert sv._hd.plan.block_size == (32 if kind == "split_off" else 8)
    rows = sv.solver._rows()
    rhs = np.random.default_rng(3).standard_normal((rows, 3))
    b0 = sv.band_stats()
    sol = sv.solver.solve(rhs)
    assert _delta(sv.band_stats(), b0)[1:] == (0, 0)
    for j in range(3):
        assert np.array_equal(sol[:, j], sv.solver.solve(rhs[:, j]))
    sv.close()


# ------------------------------------------------------------------ 5: border on wide blocks
BORDER_POLICIES = (("Full", 2), ("Simplified", 2), ("ActiveSet", 3))
BORDER_K = {1: (0, 1), 17: (9, 8), 64: (32, 32)}


def _border_case(k, block):
    """bordered_lq with bw 12 and 6 local constraints: the remainder's half-bandwidth is 13 (local
    constraints widen it; 20 of them would make it 37, too wide for B = 16 and 32), Nb = 209 is no
    multiple of 16, 32 or 64."""
    kv, kc = BORDER_K[k]
    prob = bordered_lq(203, 12, 6, kv, kc, seed=7 * k + block, block=block)
    plan = plan_of(prob)
    assert (plan.k, plan.Nb, plan.block_size) == (k, 209, block) and plan.bw <= 16
    return prob


def _border_trajectory(pgf, prob, policies, stats=None):
    x0, y0 = np.zeros(prob.num_vars), np.zeros(prob.num_cons)
    out = []
    for pol, steps in policies:
        dn = pgf.DeviceNewton(prob, pol, x0, y0, 1.0, 1.0)
        b0, s0 = dn.band_stats(), dn.border_stats()
        for _ in range(steps):
            dn.step()
            out.extend(dn.point())
        if stats is not None:
            stats.append((_delta(dn.band_stats(), b0), _delta(dn.border_stats(), s0)))
        dn.close()
    return out


@pytest.mark.parametrize("block", [16, 32, 64])
@pytest.mark.parametrize("k", [1, 17, 64])
def test_border_on_wide_blocks(pgf, k, block):
    """One factor-only reduction and ONE panel solve per factor phase (not k reductions), one solve
    phase per solve phase of the border."""
    prob = _border_case(k, block)
    assert mask_changes(prob, "Full", 2) > 0
    _against_oracle(pgf, prob, BORDER_POLICIES, n_neg=prob.num_cons)
    stats = []
    _border_trajectory(pgf, prob, BORDER_POLICIES, stats)
    for (red, sol, pan), (_, bfac, bsol) in stats:
        assert bfac >= 1 and bsol >= 2
        assert (red, pan, sol) == (bfac, bfac, bsol), (k, block, stats)
    assert stats[1][1][1] == 1  # Simplified: one factor phase


def test_border_columns_one_by_one_agree(pgf, tmp_path):
    """PGF_BORDER_MULTI=0 (read once per process: a fresh child) forms Y column by column through the
    single right-hand side solve phase; the child meets the oracle on its own and agrees with the
    panel route within TOL."""
    out = str(tmp_path / "columns.npz")
    env = dict(os.environ, PGF_BORDER_MULTI="0")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=REPO,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    theirs = np.load(out)
    ours = _border_trajectory(pgf, _border_case(17, 32), BORDER_POLICIES)
    assert len(ours) == len(theirs.files) == 14
    for i, v in enumerate(ours):
        assert G.rel_err(v, theirs[f"a{i}"]) <= TOL, i


def _child(out):
    import pygradflow_amd as pgf

    assert os.environ.get("PGF_BORDER_MULTI") == "0"
    prob = _border_case(17, 32)
    _against_oracle(pgf, prob, BORDER_POLICIES, n_neg=prob.num_cons)
    stats = []
    traj = _border_trajectory(pgf, _border_case(17, 32), BORDER_POLICIES, stats)
    for (red, sol, pan), (_, bfac, bsol) in stats:  # k + 1 solve phases per factor phase, no panel
        assert (red, pan, sol) == (bfac, 0, bsol + 17 * bfac), stats
    np.savez(out, **{f"a{i}": v for i, v in enumerate(traj)})


# ------------------------------------------------------------------ 6: the guard through the kept factors
@pytest.mark.parametrize("block", [16, 64])
def test_guard_refines_through_the_kept_factors(pgf, block):
    """The construction of test_wide_unstable_pivot_is_refined: K[v, v] = 1e-9 at the head of
    block 1.  The solve after the step refines -- its corrections are solve phases, the matrix is
    not reduced again."""
    n, eps = 300, 1e-9
    rng = np.random.default_rng(7)
    d = 2.5 + rng.uniform(0.0, 0.5, n)
    v = head_of_first_eliminated(wide_band_problem(n, d, 1, block), block)
    d[v] = -1.0 + eps  # lambda = 1: K[v, v] = eps
    prob = wide_band_problem(n, d, 1, block)
    K = prob.hess_sparse().toarray() + np.eye(n)
    assert abs(K[v, v]) < 1e-8 and np.linalg.cond(K) < 1e5
    sv, it = _step_solver(pgf, prob, mask=np.zeros(n, dtype=bool))
    b0 = sv.band_stats()
    sv.solve(it)
    assert sv._hd.plan.block_size == block
    before = sv.refinement_stats()
    b1 = sv.band_stats()
    rhs = np.arange(1.0, n + 1.0)
    sol = sv.solver.solve(rhs)
    after = sv.refinement_stats()
    assert after[0] > before[0], "the guard did not refine"
    assert after[2] <= 1e-11
    assert G.rel_err(sol, np.linalg.solve(K, rhs)) <= 1e-9
    assert _delta(sv.band_stats(), b0)[0] == 1
    red, solves, _ = _delta(sv.band_stats(), b1)
    assert red == 0 and solves == 1 + (after[0] - before[0])
    sv.close()


# ------------------------------------------------------------------ 7: exact zero pivot
@pytest.mark.parametrize("block", [16, 64])
def test_zero_pivot_leaves_no_kept_factor(pgf, block):
    """The construction of test_not_quasi_definite_is_a_step_solver_error: K[v, v] = 0 at the head
    of block 1.  Every attempt is an error and a reduction of its own, never a solve phase."""
    from pygradflow_amd.errors import StepSolverError

    n = 300
    rng = np.random.default_rng(8)
    d = 2.5 + rng.uniform(0.0, 0.5, n)
    v = head_of_first_eliminated(wide_band_problem(n, d, 2, block), block)
    d[v] = -1.0
    prob = wide_band_problem(n, d, 2, block)
    K = prob.hess_sparse().toarray() + np.eye(n)
    assert K[v, v] == 0.0 and np.linalg.cond(K) < 1e6
    sv, it = _step_solver(pgf, prob, mask=np.zeros(n, dtype=bool))
    b0 = sv.band_stats()
    for attempt in (1, 2):
        with pytest.raises(StepSolverError):
            sv.solve(it)
        assert _delta(sv.band_stats(), b0) == (attempt, 0, 0)
    sv.close()


if __name__ == "__main__":
    _child(sys.argv[1])
