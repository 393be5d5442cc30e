"""Bordered band (csrc/pgf_border.hip): the device's linear solve against a host solve of the same
reduced KKT matrix, at the small shapes where each kernel takes another branch.

test_border_gpu.py follows whole Newton trajectories on four problems (k = 1, 2, 17, 64; Nb = 1003,
520, about 500, 70 000).  Here the solve itself is isolated -- view.solve(rhs) against
band_util.refined_solve (float64, two refinement steps with an np.longdouble residual) -- on
band_util.bordered_lq problems whose k and Nb are exact:

  kp = 16, 32, 48, 64   k at, one under and one over every multiple of 16: k_border_gram with 1, 4,
                        9, 16 outputs per thread, k_border_ctv with 16, 8, 5 (16 idle threads), 4
                        row groups, k_mbcr_level / _back with 2, 4, 6, 8 panel columns per lane, the
                        padding of C, D and brb appearing and vanishing
  Nb                    1 .. 1025: nb = 1 (k_mbcr_back with s == 0 is the whole reduction), 2, 3
                        blocks; the 16-row tile remainder of k_border_gram; 255 / 256 / 257 rows
                        around the workgroup of k_border_residual and k_border_update; 511 / 512 /
                        513 around SP_BORDER_CHUNK (one chunk, one full chunk, a second chunk of
                        one row); 1023 / 1025 (two chunks, a third of one row)
  routes                B = 8 panel reduction; B = 8 repeated solves (PGF_BORDER_MULTI=0, a child
                        process); forced B = 16, 32, 64, also with Nb smaller than the block; a band
                        of half-width 22 on the automatic B = 32
  masks                 nothing / every band variable / every border variable / only border
                        variables inactive / random
  guard                 a 1e-9 pivot at the head of block 1 of B: refined, or an error
  singular S            a decoupled border variable with H[v, v] = -lambda: an error, not a step

Bars: cond(K) <= 1e4 is asserted on the host first, so eps cond <= 1e-12 leaves the project's
1e-10 (band_util.TOL) two orders of headroom; the guard cases keep the bars of
test_narrow_unstable_pivot_is_refined (cond < 1e5, residual <= 1e-11, error <= 1e-9).
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
from tests.band_util import (COND_MAX, TOL, _against_oracle, case, guard_case, plan_of,  # noqa: E402
                             reduced_kkt, refined_solve)

pytestmark = pytest.mark.gpu

WIDTHS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
ROWS = (1, 7, 8, 9, 16, 17, 24, 255, 256, 257, 511, 512, 513, 1023, 1025)
ROUTE_SHAPES = ((1, 9), (33, 513), (64, 257))
REPEATED_SHAPES = ((1, 9), (33, 513), (48, 203), (64, 257))


def random_mask(prob, seed=0):
    return np.random.default_rng([seed, prob.num_vars, prob.num_cons]).uniform(size=prob.num_vars) < 0.4


def right_hand_sides(K):
    """Columns: random; the unit vector of the last border node (the last dense constraint row: the
    last row of the reduced K under any mask); K @ ones."""
    N = K.shape[0]
    e = np.zeros(N)
    e[-1] = 1.0
    return np.stack([np.random.default_rng(N).standard_normal(N), e, K @ np.ones(N)], axis=1)


def step_solver(pgf, prob, mask):
    n, m = prob.num_vars, prob.num_cons
    params = pgf.Params()
    it = pgf.Iterate(prob, params, np.zeros(n), np.zeros(m))
    sv = pgf.HipStepSolver(prob, params, it, 1.0, 1.0)
    assert sv.sparse
    sv.update_active_set(mask)
    sv.update_derivs(it)
    return sv, it


def device_solves(pgf, prob, mask, rhs, k, kp, Nb, block):
    """The three solves on the device and everything the handle reports about them: (solutions in
    columns, negative pivots).  One factor phase serves the three solves; the guard measures each,
    and refines none."""
    sv, _ = step_solver(pgf, prob, mask)
    view = sv.solver_for_tests()
    plan = sv._hd.plan
    assert (plan.k, plan.kp, plan.Nb, plan.block_size) == (k, kp, Nb, block), \
        (plan.k, plan.kp, plan.Nb, plan.block_size)
    k0, f0, s0 = sv.border_stats()
    refined0 = sv.refinement_stats()[0]
    assert k0 == k
    sols = []
    for j in range(rhs.shape[1]):
        sols.append(view.solve(rhs[:, j]))
        refined, _, rel = sv.refinement_stats()
        assert rel <= 1e-11, (j, rel)
        assert refined == refined0, (j, refined - refined0)
    assert sv.border_stats() == (k, f0 + 1, s0 + rhs.shape[1])
    n_neg = view.num_neg_eigvals()
    sv.close()
    return np.stack(sols, axis=1), n_neg


def host_reference(prob, mask):
    """(K, right-hand sides, refined solutions, plain float64 solutions); cond(K) <= 1e4 asserted."""
    K = reduced_kkt(prob, mask)
    cond = np.linalg.cond(K)
    assert cond <= COND_MAX, cond
    rhs = right_hand_sides(K)
    ref, plain = refined_solve(K, rhs)
    return K, rhs, ref, plain


def errors(sols, ref, plain):
    """Largest of the three device errors and of the three float64 host errors, both against the
    refined reference (golden_util.rel_err per right-hand side)."""
    dev = max(G.rel_err(sols[:, j], ref[:, j]) for j in range(ref.shape[1]))
    host = max(G.rel_err(plain[:, j], ref[:, j]) for j in range(ref.shape[1]))
    return dev, host


def check_linear_solve(pgf, prob, mask, k, Nb, block, tag):
    kp = (k + 15) // 16 * 16
    _, rhs, ref, plain = host_reference(prob, mask)
    sols, n_neg = device_solves(pgf, prob, mask, rhs, k, kp, Nb, block)
    dev, host = errors(sols, ref, plain)
    print(f"border-edge {tag}: k {k} kp {kp} Nb {Nb} B {block} device error {dev:.3e} float64 host "
          f"{host:.3e} ratio {dev / max(host, 1e-300):.2f}")
    assert dev <= TOL, dev
    assert n_neg == prob.num_cons
    return sols


# ------------------------------------------------------------------ 1: border width
@pytest.mark.parametrize("k", WIDTHS)
def test_border_width(pgf, k):
    """Nb = 203: 26 blocks of 8, a padded last block, no power of two; random 40 % mask."""
    prob = case(k, 203)
    check_linear_solve(pgf, prob, random_mask(prob), k, 203, 8, "width")


# ------------------------------------------------------------------ 2: row count
@pytest.mark.parametrize("Nb", ROWS)
@pytest.mark.parametrize("k", [17, 48])
def test_row_count(pgf, k, Nb):
    """Random 40 % mask; the first band variable stays inactive, so that a band of a single row is
    not an identity row."""
    prob = case(k, Nb)
    mask = random_mask(prob)
    mask[0] = False
    check_linear_solve(pgf, prob, mask, k, Nb, 8, "rows")


# ------------------------------------------------------------------ 3: other routes
@pytest.mark.parametrize("k,Nb", ROUTE_SHAPES)
@pytest.mark.parametrize("block", [16, 32, 64])
def test_forced_block(pgf, block, k, Nb):
    """Y by k single solves through the wide reduction; (1, 9): Nb smaller than the block."""
    prob = case(k, Nb, block=block)
    check_linear_solve(pgf, prob, random_mask(prob), k, Nb, block, "forced")


def wide_case():
    """H of half-width 22, no local constraints (they would widen the band): automatic B = 32."""
    return case(48, 300, bw=22, mloc=0)


def test_half_width_22_on_the_automatic_block_32(pgf):
    prob = wide_case()
    plan = plan_of(prob)
    assert plan.bw == 22 and plan.block is None
    check_linear_solve(pgf, prob, random_mask(prob), 48, 300, 32, "bw22")


def test_repeated_solves_at_block_8(pgf, tmp_path):
    """PGF_BORDER_MULTI=0 is read once per process: a child solves the four shapes column by column
    at B = 8 and writes its solutions; they meet the host reference on their own, and the panel
    reduction of this process to 1e-12 (the bar of test_multi_rhs_against_repeated_solves)."""
    out = str(tmp_path / "repeated.npz")
    env = dict(os.environ, PGF_BORDER_MULTI="0")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=REPO,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    theirs = np.load(out)
    for k, Nb in REPEATED_SHAPES:
        prob = case(k, Nb)
        mask = random_mask(prob)
        _, _, ref, plain = host_reference(prob, mask)
        rep = theirs[f"s_{k}_{Nb}"]
        dev, host = errors(rep, ref, plain)
        print(f"border-edge repeated: k {k} Nb {Nb} B 8 device error {dev:.3e} float64 host {host:.3e} "
              f"ratio {dev / max(host, 1e-300):.2f}")
        assert dev <= TOL, (k, Nb, dev)
        assert int(theirs[f"neg_{k}_{Nb}"]) == prob.num_cons
        ours = check_linear_solve(pgf, prob, mask, k, Nb, 8, "panel")
        for j in range(3):
            err = G.rel_err(ours[:, j], rep[:, j])
            assert err <= 1e-12, (k, Nb, j, err)


def _child(out):
    import pygradflow_amd as pgf

    assert os.environ.get("PGF_BORDER_MULTI") == "0"
    res = {}
    for k, Nb in REPEATED_SHAPES:
        prob = case(k, Nb)
        mask = random_mask(prob)
        rhs = right_hand_sides(reduced_kkt(prob, mask))
        sols, n_neg = device_solves(pgf, prob, mask, rhs, k, (k + 15) // 16 * 16, Nb, 8)
        res[f"s_{k}_{Nb}"] = sols
        res[f"neg_{k}_{Nb}"] = n_neg
    np.savez(out, **res)


# ------------------------------------------------------------------ 4: masks
@pytest.mark.parametrize("which", ["none", "band", "border", "only_border_inactive", "random"])
def test_masks(pgf, which):
    """k = 17 (5 variables, 12 constraints), Nb = 257.  "border": C's variable columns are zero and D
    has unit rows; "band": B's variable rows are identity rows."""
    prob = case(17, 257)
    n, kv = prob.num_vars, 5
    mask = np.zeros(n, dtype=bool)
    if which in ("band", "only_border_inactive"):
        mask[: n - kv] = True
    elif which == "border":
        mask[n - kv:] = True
    elif which == "random":
        mask = random_mask(prob, 1)
        assert mask[n - kv:].any() and not mask[n - kv:].all()
    assert sorted(prob.pgf_border[:kv]) == list(range(n - kv, n))
    check_linear_solve(pgf, prob, mask, 17, 257, 8, "mask " + which)


# ------------------------------------------------------------------ 5: the guard with a border
@pytest.mark.parametrize("block", [8, 16])
@pytest.mark.parametrize("k", [1, 17])
def test_bordered_unstable_pivot_is_refined(pgf, k, block):
    """A 1e-9 pivot inside B makes Y = inv(B) C, hence S, inaccurate: band_refine then iterates the
    whole bordered solve on the residual.  It must repair the step or raise; the bars are those of
    test_narrow_unstable_pivot_is_refined."""
    prob, v = guard_case(k, block, 1e-9)
    n, m = prob.num_vars, prob.num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    rec = O.NewtonOracle(prob, "Full", x0, y0, 1.0, 1.0).run(x0, y0, 1)[0]
    mask = rec["mask"]
    assert not mask.any()
    K = reduced_kkt(prob, mask)
    assert abs(K[v, v]) < 1e-8 and np.linalg.cond(K) < 1e5
    sv, it = step_solver(pgf, prob, mask)
    before = sv.refinement_stats()
    res = sv.solve(it)
    after = sv.refinement_stats()
    plan = sv._hd.plan
    assert (plan.k, plan.Nb, plan.block_size) == (k, 300, block)
    err = max(G.rel_err(res.dx, rec["dx"]), G.rel_err(res.dy, rec["dy"]))
    print(f"border-guard k {k} block {block} v {v}: refined {before[0]} -> {after[0]}, last_rel_residual "
          f"{after[2]:.3e}, step error {err:.3e}")
    assert after[0] > before[0], "the guard did not refine"
    assert after[2] <= 1e-11
    assert err <= 1e-9
    rhs = np.arange(1.0, K.shape[0] + 1.0)
    assert G.rel_err(sv.solver.solve(rhs), refined_solve(K, rhs)[0]) <= 1e-9
    sv.close()
    dn = pgf.DeviceNewton(prob, "Full", x0, y0, 1.0, 1.0)
    dn.step()
    x, y = dn.point()
    assert np.array_equal(dn.mask(), mask)
    assert G.rel_err(x, rec["xn"]) <= 1e-9 and G.rel_err(y, rec["yn"]) <= 1e-9
    dn.close()


@pytest.mark.parametrize("block", [8, 16])
@pytest.mark.parametrize("k", [1, 17])
def test_bordered_not_quasi_definite_is_a_step_solver_error(pgf, k, block):
    """K[v, v] = 0 exactly where B is pivoted as it stands: K is regular but not quasi-definite."""
    from pygradflow_amd.errors import StepSolverError

    prob, v = guard_case(k, block, 0.0)
    mask = np.zeros(prob.num_vars, dtype=bool)
    K = reduced_kkt(prob, mask)
    assert K[v, v] == 0.0 and np.linalg.cond(K) < 1e6
    sv, it = step_solver(pgf, prob, mask)
    with pytest.raises(StepSolverError):
        sv.solve(it)
    sv.close()


# ------------------------------------------------------------------ 6: singular Schur complement
def test_singular_schur_complement_is_an_error(pgf):
    """The second of two border variables is decoupled (an empty column in C and in the dense rows)
    with H[v, v] = -lambda: B is as regular as ever, K is singular through S alone
    (k_border_factor_S meets an exact zero pivot).  Neither front end may return a step."""
    from pygradflow_amd import problems
    from pygradflow_amd.errors import StepSolverError

    base = case(6, 203)
    n, m = base.num_vars, base.num_cons
    v = n - 1
    H, A = sps.lil_matrix(base.hess_sparse()), sps.lil_matrix(base.jac_sparse())
    H[v, :] = 0.0
    H[:, v] = 0.0
    H[v, v] = -1.0
    A[:, v] = 0.0
    q = np.array(base.q)
    q[v] = 0.0  # the gradient vanishes at v: inactive
    prob = problems.LinearQuadraticProblem(sps.csr_matrix(H), q, sps.csr_matrix(A), base.b, base.var_lb,
                                           base.var_ub)
    prob.pgf_border = list(base.pgf_border)
    plan = plan_of(prob)
    assert (plan.k, plan.Nb, plan.block_size) == (6, 203, 8) and plan.pos[v] == 203 + 1
    x0, y0 = np.zeros(n), np.zeros(m)
    mask = O.NewtonOracle(prob, "Full", x0, y0, 1.0, 1.0).solver.compute_active_set(O.PointData(prob, x0, y0))
    assert not mask[v] and not mask[v - 1]
    K = reduced_kkt(prob, mask)
    iv = int(np.count_nonzero(~mask[:v]))
    assert not K[iv].any()
    keep = np.arange(K.shape[0]) != iv
    assert np.linalg.cond(K[np.ix_(keep, keep)]) <= COND_MAX  # singular through that row alone
    sv, it = step_solver(pgf, prob, mask)
    with pytest.raises(StepSolverError):
        res = sv.solve(it)
        print("returned dx", np.max(np.abs(res.dx)))
    sv.close()
    dn = pgf.DeviceNewton(prob, "Full", x0, y0, 1.0, 1.0)
    with pytest.raises(StepSolverError):
        dn.step()
    dn.close()


# ------------------------------------------------------------------ 7: trajectories at the new widths
TRAJECTORIES = {
    "kp48_B8": lambda: case(48, 203, seed=3),
    "kp48_B32": lambda: case(48, 300, bw=22, mloc=0, seed=4),
    "Nb9": lambda: case(17, 9, seed=5),
    "Nb513": lambda: case(17, 513, seed=6),
}


@pytest.mark.parametrize("name", sorted(TRAJECTORIES))
def test_trajectory(pgf, name):
    """Evaluation, scatter and step update at these layouts: Full x 3 and Simplified x 2 against the
    oracle, on problems where a border variable changes activity during the Full run."""
    prob = TRAJECTORIES[name]()
    n, m = prob.num_vars, prob.num_cons
    kv = sum(1 for i in prob.pgf_border if i < n)
    x0, y0 = np.zeros(n), np.zeros(m)
    masks = [r["mask"][n - kv:] for r in O.NewtonOracle(prob, "Full", x0, y0, 1.0, 1.0).run(x0, y0, 3)]
    assert any(not np.array_equal(a, b) for a, b in zip(masks, masks[1:]))
    plan = plan_of(prob)
    assert (plan.kp, plan.Nb, plan.block_size) == {"kp48_B8": (48, 203, 8), "kp48_B32": (48, 300, 32),
                                                   "Nb9": (32, 9, 8), "Nb513": (32, 513, 8)}[name]
    churn = _against_oracle(pgf, prob, (("Full", 3), ("Simplified", 2)), n_neg=m)
    assert churn > 0


if __name__ == "__main__":
    _child(sys.argv[1])
