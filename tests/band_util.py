"""Problem builders and CPU references shared by the banded-path tests (test_band*.py,
test_border*.py; band_batch_util.py has the batch harness).

Bars as in test_gpu_parity.py: masks bit-identical, x and y within 1e-10 relative."""

import numpy as np
import scipy.sparse as sps

from oracle import newton_oracle as O
from tests import golden_util as G

TOL = 1e-10
COND_MAX = 1e4  # cond(K) asserted on the host where eps cond is to leave TOL two orders of headroom

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


def forced(prob, block=None, split=None):
    """``prob`` sent down the banded path (pgf_force_band), with a forced block size and the
    factor / solve split of the wide reduction switched on or off if given."""
    prob.pgf_force_band = True
    if block is not None:
        prob.pgf_band_block = block
    if split is not None:
        prob.pgf_band_split = split
    return prob


def multistate_ocp(T, nx, nu, seed, block=None, split=None):
    """problems.multistate_ocp(T, nx, nu, seed=seed), forced."""
    from pygradflow_amd import problems

    return forced(problems.multistate_ocp(T, nx, nu, seed=seed), block, split)


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


def mask_change_steps(prob, pol, steps, dt=1.0, rho=1.0):
    """Per oracle step of the policy from zero after the first: its active set differs from that of
    the step before."""
    n, m = prob.num_vars, prob.num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    recs = O.NewtonOracle(prob, pol, x0, y0, dt, rho).run(x0, y0, steps)
    return [not np.array_equal(a["mask"], b["mask"]) for a, b in zip(recs, recs[1:])]


def mask_changes(prob, pol, steps, dt=1.0, rho=1.0):
    """Number of oracle steps of the policy whose active set differs from the step before."""
    return sum(mask_change_steps(prob, pol, steps, dt, rho))


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


def wide_band_problem(n, d, seed, block=None):
    """band_problem of half-width 12 (block size 16 by the plan), m = 0, no bounds; forced."""
    return forced(band_problem(n, d, seed, 12), block)


def _decoupled_hess(prob, v):
    H = sps.csr_matrix(prob.hess_sparse(), copy=True)
    rows = np.repeat(np.arange(H.shape[0]), np.diff(H.indptr))
    H.data[(rows == v) | (H.indices == v)] = 0.0
    H.data[(rows == v) & (H.indices == v)] = -1.0
    return H


def decoupled(good, v):
    """``good`` with variable v decoupled and H[v, v] = -1 (K[v, v] = 0 at dt = 1) ON THE SAME
    PATTERN: the entries of row and column v stay stored, as zeros."""
    from pygradflow_amd import problems

    return problems.LinearQuadraticProblem(_decoupled_hess(good, v), good.q, good.jac_sparse(), good.b,
                                           good.var_lb, good.var_ub)


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


def case(k, Nb, bw=2, block=None, mloc=None, seed=None, bound=0.5):
    """bordered_lq with k border nodes (a third of them variables) and Nb band rows (a quarter of
    them local constraints unless mloc is given)."""
    mloc = Nb // 4 if mloc is None else mloc
    kv = k // 3
    return bordered_lq(Nb - mloc, bw, mloc, kv, k - kv, 1000 * k + Nb if seed is None else seed,
                       block=block, bound=bound)


def reduced_kkt(prob, mask, lamb=1.0, rho=1.0):
    return O.kkt_matrix(O.shifted_hess_rows(prob.hess_sparse(), lamb, mask), prob.jac_sparse().tocsc(), mask,
                        lamb, rho).toarray()


def with_hess_diagonal(prob, v, value):
    """The same problem with H[v, v] = value; border and block settings kept."""
    from pygradflow_amd import problems

    H = sps.lil_matrix(prob.hess_sparse())
    H[v, v] = value
    new = problems.LinearQuadraticProblem(sps.csr_matrix(H), prob.q, prob.jac_sparse(),
                                          prob.b, prob.var_lb, prob.var_ub)
    new.pgf_border = list(prob.pgf_border)
    if getattr(prob, "pgf_band_block", None):
        new.pgf_band_block = prob.pgf_band_block
    return new


def guard_case(k, block, pivot):
    """Nb = 300 band variables with a full band of half-width 8 and no local constraints, the
    layout of the narrow test one bandwidth down.  The variable v at the head of block 1 of B
    (inverted as it stands by level one of either reduction) gets K[v, v] = pivot at lambda = 1;
    the box is +-1e6, so no variable is active and v keeps its in-block couplings c = 0.04 U(0.5, 1).
    With pivot = 1e-9 the unpivoted inverse of that block adds c^2 / pivot, about 1e6, to entries
    of order one: a relative error near 1e6 u = 1e-10, ten times refine_tol, before the reduction
    has done anything else."""
    kv = k // 3
    base = bordered_lq(300, 8, 0, kv, k - kv, 77 + k + block, block=None if block == 8 else block, bound=1e6)
    v = head_of_first_eliminated(base, block)
    assert v < 300  # a band variable
    prob = with_hess_diagonal(base, v, -1.0 + pivot)
    assert plan_of(prob).block_size == block and head_of_first_eliminated(prob, block) == v
    return prob, v


def singular_schur(base):
    """The construction of test_border_edges_gpu.py::test_singular_schur_complement_is_an_error ON THE
    PATTERN of ``base``: the last border variable v decoupled (its row and column of H and its
    column of J stay stored, as zeros), H[v, v] = -1 = -lambda at dt = 1, q[v] = 0."""
    from pygradflow_amd import problems

    v = base.num_vars - 1
    A = sps.csr_matrix(base.jac_sparse(), copy=True)
    A.data[A.indices == v] = 0.0
    q = np.array(base.q)
    q[v] = 0.0
    prob = problems.LinearQuadraticProblem(_decoupled_hess(base, v), q, A, base.b, base.var_lb, base.var_ub)
    prob.pgf_border = list(base.pgf_border)
    return prob, v


def singular_schur_wide(base):
    """singular_schur with the forced block size carried over."""
    prob, v = singular_schur(base)
    prob.pgf_band_block = base.pgf_band_block
    return prob, v


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


def normwise(K, x, b):
    """The guard's measure (band_residual_rel_of): max |b - K x| / max (|K| |x| + |b|)."""
    return np.abs(b - K @ x).max() / (np.abs(K) @ np.abs(x) + np.abs(b)).max()


def gj_inverse(M):
    """Unpivoted Gauss-Jordan inverse in float64 (gj_inverse8 of pgf_bcr_dev.h, bw_gj_inverse of
    pgf_band_wide_dev.h)."""
    M = M.copy()
    for k in range(M.shape[0]):
        d = 1.0 / M[k, k]
        row, col = M[k, :].copy(), M[:, k].copy()
        M -= np.outer(col * d, row)
        M[k, :] = row * d
        M[:, k] = -col * d
        M[k, k] = d
    return M


def level_one_solve(Kp, f, block=8):
    """The first level of the cyclic reduction with blocks of ``block`` rows on the permuted matrix,
    in float64: the odd blocks are inverted unpivoted as they stand and eliminated; what is left is
    solved by LAPACK."""
    N = Kp.shape[0]
    blk = np.arange(N) // block
    o, e = np.nonzero(blk % 2 == 1)[0], np.nonzero(blk % 2 == 0)[0]
    Dinv = np.zeros((o.size, o.size))
    for b in np.unique(blk[o]):
        idx = np.nonzero(blk[o] == b)[0]
        Dinv[np.ix_(idx, idx)] = gj_inverse(Kp[np.ix_(o[idx], o[idx])])
    Keo, Koe = Kp[np.ix_(e, o)], Kp[np.ix_(o, e)]
    xe = np.linalg.solve(Kp[np.ix_(e, e)] - Keo @ Dinv @ Koe, f[e] - Keo @ (Dinv @ f[o]))
    x = np.zeros(N)
    x[e] = xe
    x[o] = Dinv @ (f[o] - Koe @ xe)
    return x
