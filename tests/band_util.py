"""Helpers shared by the banded-path GPU tests (test_band_wide_gpu.py, test_band_narrow_gpu.py,
test_border_gpu.py, test_border_edges_gpu.py).

Bars as in test_gpu_parity.py: masks bit-identical, x and y within 1e-10 relative."""

import numpy as np
import scipy.sparse as sps

from oracle import newton_oracle as O
from tests import golden_util as G

TOL = 1e-10

# sizes of the 8 x 8 cyclic reduction's edge sweep (test_band_narrow_gpu.py has the table of launch
# plan branches they hit; check_band.py --sweep runs them under the schedule switches)
SWEEP_BOX = (1, 7, 8, 9, 255, 256, 257, 263, 264, 265, 511, 512, 513, 520, 1024, 1025, 1031, 1033)  # box_qp(n)
SWEEP_OCP = (1, 2, 3, 11, 85, 86, 171, 172, 342, 343)  # sparse_ocp(m): N = 3 m


def bcr_launch_plan(nb, pair_max=4096, pairs=True, fused=True, tail=32):
    """Launch plan of the 8 x 8 cyclic reduction for nb blocks, the arithmetic of
    sp_launch_bcr_solve restated on the host: ([("single" | "pair", stride), ...] before the tail,
    blocks the LDS tail starts with).  pair_max, pairs, fused: PGF_BCR_PAIR_MAX, PGF_BCR_PAIRS,
    PGF_BCR_FUSED (pairs need fused levels)."""
    st, levels = 1, []
    while st < nb:
        left = (nb + st - 1) // st
        if left <= tail:
            break
        left2 = (nb + 2 * st - 1) // (2 * st)
        if fused and pairs and left <= pair_max and left2 > tail and 2 * st < nb:
            levels.append(("pair", st))
            st *= 4
        else:
            levels.append(("single", st))
            st *= 2
    return levels, (nb + st - 1) // st


def bcr_launch_plan_from_env(nb, env):
    """bcr_launch_plan under the switches in ``env`` (a mapping like os.environ)."""
    off = lambda name: name in env and int(env[name]) == 0  # noqa: E731
    return bcr_launch_plan(nb, pair_max=int(env.get("PGF_BCR_PAIR_MAX", 4096)),
                           pairs=not off("PGF_BCR_PAIRS"), fused=not off("PGF_BCR_FUSED"))


def _as_sparse_lq(problem, block=None):
    from pygradflow_amd import problems

    sp = problems.LinearQuadraticProblem(
        sps.csr_matrix(problem.hess_dense()), problem.q,
        sps.csr_matrix(problem.jac_dense().reshape(problem.num_cons, problem.num_vars)),
        problem.b, problem.var_lb, problem.var_ub)
    sp.pgf_force_band = True
    if block:
        sp.pgf_band_block = block
    return sp


def _against_oracle(pgf, prob, policies, dt=1.0, rho=1.0, step_solver=True, n_neg=None, x0=None):
    """DeviceNewton (and, with step_solver, HipStepSolver through newton_steps) against the
    oracle: masks identical, x and y within TOL; n_neg of every device step if given.  Starts
    from x0 (zero if not given), y0 = 0; returns the largest active-set size met."""
    n, m = prob.num_vars, prob.num_cons
    x0 = np.zeros(n) if x0 is None else np.asarray(x0, dtype=np.float64)
    y0 = np.zeros(m)
    churn = 0
    for pol, steps in policies:
        recs = O.NewtonOracle(prob, pol, x0, y0, dt, rho).run(x0, y0, steps)
        dn = pgf.DeviceNewton(prob, pol, x0, y0, dt, rho)
        assert dn.sparse
        for k, rec in enumerate(recs):
            _, nn = dn.step()
            x, y = dn.point()
            assert np.array_equal(dn.mask(), rec["mask"]), (pol, k)
            assert G.rel_err(x, rec["xn"]) <= TOL, (pol, k)
            assert G.rel_err(y, rec["yn"]) <= TOL, (pol, k)
            if n_neg is not None:
                assert nn == n_neg, (pol, k)
            churn = max(churn, int(np.count_nonzero(rec["mask"])))
        dn.close()
        if step_solver:
            params = pgf.Params(newton_type=pol, step_solver=pgf.HipStepSolver)
            gen = pgf.newton_steps(prob, params, pgf.Iterate(prob, params, x0, y0), dt, rho)
            for k, rec in enumerate(recs):
                step = next(gen)
                assert np.array_equal(step.active_set, rec["mask"]), (pol, k)
                assert G.rel_err(step.iterate.x, rec["xn"]) <= TOL, (pol, k)
                assert G.rel_err(step.iterate.y, rec["yn"]) <= TOL, (pol, k)
    return churn


def mask_changes(prob, pol, steps, dt=1.0, rho=1.0):
    """Number of oracle steps of the policy whose active set differs from the step before."""
    n, m = prob.num_vars, prob.num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    recs = O.NewtonOracle(prob, pol, x0, y0, dt, rho).run(x0, y0, steps)
    return sum(int(not np.array_equal(a["mask"], b["mask"])) for a, b in zip(recs, recs[1:]))


def simplified_mask_goes_stale(prob, dt=1.0, rho=1.0):
    """True if, after the first Simplified step from zero, the active set at the new point differs
    from the one the Simplified policy keeps: a second step that refactorised with the current
    mask would then not reproduce the oracle's back-solve step."""
    n, m = prob.num_vars, prob.num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    first = O.NewtonOracle(prob, "Simplified", x0, y0, dt, rho).run(x0, y0, 1)[0]
    fresh = O.NewtonOracle(prob, "Full", x0, y0, dt, rho).run(first["xn"], first["yn"], 1)[0]
    return not np.array_equal(first["mask"], fresh["mask"])


def band_problem(n, d, seed, bw, lb=None, ub=None):
    """H = diag(d) + a symmetric band of half-width bw with small entries, m = 0; no bounds
    unless given."""
    from pygradflow_amd import problems

    rng = np.random.default_rng(seed)
    offs = [k for k in range(-bw, bw + 1) if k != 0]
    vals = {k: 0.04 * rng.uniform(0.5, 1.0, n - abs(k)) for k in range(1, bw + 1)}
    diags = [vals[abs(k)] for k in offs]
    H = (sps.diags(diags, offs, shape=(n, n)) + sps.diags(d)).tocsr()
    lb = np.full(n, -np.inf) if lb is None else lb
    ub = np.full(n, np.inf) if ub is None else ub
    return problems.LinearQuadraticProblem(H, rng.standard_normal(n), sps.csr_matrix((0, n)), np.zeros(0),
                                           lb, ub)


def bordered_lq(n0, bw, mloc, kv, kc, seed, block=None, bound=0.5):
    """A band plus an explicit border of k = kv + kc nodes, every size exact (host only):

      n0    band variables: H banded with half-width bw, diagonal in [1, 2], off-diagonals
            0.04 U(0.5, 1) (band_problem);
      mloc  local constraints x[a] - c x[a + 1] = b, c in U(0.5, 1), a spread evenly: B gets
            negative pivots of its own (mloc <= n0 - 1);
      kv    global variables behind the band ones, coupled to every band variable through H with
            U(-1, 1) 0.3 / sqrt(n0), diagonal in [1, 2];
      kc    dense constraint rows over all n = n0 + kv variables, N(0, 1) / sqrt(n);
      box   [-bound, bound] on every variable, q ~ N(0, 1), b ~ 0.1 N(0, 1).

    prob.pgf_border lists the kv variables and the kc dense rows, so k = kv + kc and
    Nb = n0 + mloc whatever select_border would find; block: a forced pgf_band_block."""
    from pygradflow_amd import problems

    assert n0 >= 1 and 0 <= mloc <= max(n0 - 1, 0) and kv >= 0 and kc >= 0 and kv + kc >= 1
    rng = np.random.default_rng(seed)
    n, m = n0 + kv, mloc + kc
    wb = min(bw, n0 - 1)
    offs = [k for k in range(-wb, wb + 1) if k != 0]
    vals = {k: 0.04 * rng.uniform(0.5, 1.0, n0 - k) for k in range(1, wb + 1)}
    Hb = sps.diags(rng.uniform(1.0, 2.0, n0))
    if offs:
        Hb = Hb + sps.diags([vals[abs(k)] for k in offs], offs, shape=(n0, n0))
    G = sps.csr_matrix(rng.uniform(-1.0, 1.0, (n0, kv)) * 0.3 / np.sqrt(n0))
    H = sps.bmat([[Hb, G], [G.T, sps.diags(rng.uniform(1.0, 2.0, kv))]], format="csr")
    a = (np.arange(mloc) * (n0 - 1)) // max(mloc, 1)
    loc = sps.csr_matrix((np.concatenate([np.ones(mloc), -rng.uniform(0.5, 1.0, mloc)]),
                          (np.concatenate([np.arange(mloc)] * 2), np.concatenate([a, a + 1]))), shape=(mloc, n))
    A = sps.vstack([loc, sps.csr_matrix(rng.standard_normal((kc, n)) / np.sqrt(n))], format="csr")
    prob = problems.LinearQuadraticProblem(H, rng.standard_normal(n), A, 0.1 * rng.standard_normal(m),
                                           np.full(n, -bound), np.full(n, bound))
    prob.pgf_border = [n0 + j for j in range(kv)] + [n + mloc + r for r in range(kc)]
    if block:
        prob.pgf_band_block = block
    return prob


def plan_of(prob, border=None):
    """The band plan the solvers build for the problem (automatic or forced block size; border:
    the problem's own pgf_border unless given)."""
    from pygradflow_amd.sparse import BandPlan

    return BandPlan(prob.hess_sparse(), prob.jac_sparse(), prob.num_vars, prob.num_cons,
                    block=getattr(prob, "pgf_band_block", None),
                    border=getattr(prob, "pgf_border", None) if border is None else border)


def head_of_first_eliminated(prob, block):
    """Variable that the plan puts first in block 1 of a reduction with blocks of ``block`` rows
    (inverted as it stands by level one)."""
    plan = plan_of(prob)
    assert plan.bw <= block
    return int(np.nonzero(plan.pos[: prob.num_vars] == block)[0][0])


def refined_solve(K, rhs):
    """float64 solve followed by two refinement steps whose residual is accumulated in
    np.longdouble; returns (refined, plain float64) solutions.  rhs: a vector, or right-hand sides
    in columns."""
    plain = np.linalg.solve(K, rhs)
    Kl, bl = K.astype(np.longdouble), rhs.astype(np.longdouble)
    x = plain.astype(np.longdouble)
    for _ in range(2):
        r = bl - Kl @ x
        x = x + np.linalg.solve(K, np.asarray(r, dtype=np.float64)).astype(np.longdouble)
    return np.asarray(x, dtype=np.float64), plain
