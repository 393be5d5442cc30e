"""Large border (65 .. 1024 border nodes on one banded handle: csrc/pgf_border_large.hip,
``problem.pgf_border_limit``) against the CPU oracle.

Bars as in test_gpu_parity.py: masks bit-identical, x and y within 1e-10 relative, inertia m.
Shapes, the smallest at which each branch can go wrong:

  case(65, 333, bw=2, block=16)   the first size past the small border: kp = 128, the second
                                  64-column slice holds one real column, S has 63 identity rows of
                                  padding; 21 blocks of 16 (no power of two, a padded last block);
                                  the Gram kernel runs 3 tiles x 6 chunks of 64 rows, the last of 13
  case(128, 1003, bw=2)           two exact slices; a narrow band (bw 5) lifted to block 16, 63 blocks
  case(257, 1003, bw=12)          kp = 320: five slices, 15 tiles x 16 chunks (the last of 43 rows);
                                  S spans two outer blocks of the dense LDL^T (256); block 64
  case(1024, 1003, bw=2)          the limit: kp = 1024, sixteen slices, 136 tiles, four outer blocks
  multistate_ocp(300, 24, 8)      the automatic border, k = 299
"""

import ctypes as C
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
from tests.band_util import (TOL, _against_oracle, case, guard_case, reduced_kkt, refined_solve,  # noqa: E402
                             singular_schur_wide)

pytestmark = pytest.mark.gpu

CASE1_POLICIES = (("Full", 3), ("ActiveSet", 3), ("Simplified", 3))


def large(prob):
    prob.pgf_border_limit = 1024
    return prob


def case1():
    return large(case(65, 333, bw=2, block=16))


def oracle_run(prob, pol, steps, dt=1.0, rho=1.0):
    x0, y0 = np.zeros(prob.num_vars), np.zeros(prob.num_cons)
    return O.NewtonOracle(prob, pol, x0, y0, dt, rho).run(x0, y0, steps)


def border_activity(prob, recs):
    """(a border variable is active in some step, one is inactive in some step)"""
    bv = [i for i in prob.pgf_border if i < prob.num_vars]
    return any(r["mask"][bv].any() for r in recs), any(not r["mask"][bv].all() for r in recs)


def device_trajectory(pgf, prob, policies):
    x0, y0 = np.zeros(prob.num_vars), np.zeros(prob.num_cons)
    out = []
    for pol, steps in policies:
        dn = pgf.DeviceNewton(prob, pol, x0, y0, 1.0, 1.0)
        for _ in range(steps):
            dn.step()
            out.extend(dn.point())
        dn.close()
    return out


def gram_plan(dn):
    """(rows per chunk, chunks, tiles) of the Gram kernel as the handle launches it."""
    from pygradflow_amd import _lib

    r, c, t = C.c_int(0), C.c_int(0), C.c_int(0)
    _lib.check(dn._lib.pgf_debug_border_gram_plan(dn._hd.h, C.byref(r), C.byref(c), C.byref(t)), dn._hd.h,
               "pgf_debug_border_gram_plan")
    return r.value, c.value, t.value


# ------------------------------------------------------------------ 1: k = 65
def test_k65_against_oracle(pgf):
    prob = case1()
    n, m = prob.num_vars, prob.num_cons
    recs = oracle_run(prob, "Full", 3)
    counts = [int(np.count_nonzero(r["mask"])) for r in recs]
    print("active counts", counts)
    assert len(set(counts)) > 1  # the mask churns
    assert border_activity(prob, recs) == (True, True)
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(n), np.zeros(m), 1.0, 1.0)
    plan = dn._hd.plan
    assert (plan.k, plan.kp, plan.Nb, plan.block_size, plan.large) == (65, 128, 333, 16, True)
    assert dn.border_stats() == (65, 0, 0)
    dn.close()
    _against_oracle(pgf, prob, CASE1_POLICIES, n_neg=m)


def test_k65_simplified_keeps_the_factor(pgf):
    prob = case1()  # a new problem object: the pattern (and the border) are uploaded anew
    n, m = prob.num_vars, prob.num_cons
    recs = oracle_run(prob, "Simplified", 3)
    dn = pgf.DeviceNewton(prob, "Simplified", np.zeros(n), np.zeros(m), 1.0, 1.0)
    for rec in recs:
        dn.step()
        x, y = dn.point()
        assert G.rel_err(x, rec["xn"]) <= TOL and G.rel_err(y, rec["yn"]) <= TOL
    k, factorisations, solves = dn.border_stats()
    dn.close()
    assert k == 65 and factorisations == 1 and solves >= 3, (k, factorisations, solves)


# ------------------------------------------------------------------ 2, 3: two and five slices
def test_k128_two_exact_slices(pgf):
    prob = large(case(128, 1003, bw=2))
    recs = oracle_run(prob, "Full", 2)
    assert border_activity(prob, recs) == (True, True)
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(prob.num_vars), np.zeros(prob.num_cons), 1.0, 1.0)
    plan = dn._hd.plan
    dn.close()
    assert (plan.k, plan.kp, plan.Nb, plan.bw, plan.block_size) == (128, 128, 1003, 5, 16)
    churn = _against_oracle(pgf, prob, (("Full", 2), ("Simplified", 2)), n_neg=prob.num_cons)
    assert churn > 0


def test_k257_five_slices_two_outer_blocks(pgf):
    prob = large(case(257, 1003, bw=12))
    recs = oracle_run(prob, "Full", 2)
    assert border_activity(prob, recs) == (True, True)
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(prob.num_vars), np.zeros(prob.num_cons), 1.0, 1.0)
    plan = dn._hd.plan
    dn.close()
    assert (plan.k, plan.kp, plan.Nb, plan.bw, plan.block_size) == (257, 320, 1003, 41, 64)
    _against_oracle(pgf, prob, (("Full", 2),), n_neg=prob.num_cons)


def test_k1024_the_limit(pgf):
    """k = 1024 = kp: sixteen slices, 136 Gram tiles, S spans four outer blocks of the dense LDL^T,
    z fills the 8 KB of LDS in the update and residual kernels.  cond(K) = 7 at the first step."""
    prob = large(case(1024, 1003, bw=2))
    n, m = prob.num_vars, prob.num_cons
    recs = oracle_run(prob, "Full", 2)
    assert border_activity(prob, recs) == (True, True)
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(n), np.zeros(m), 1.0, 1.0)
    plan = dn._hd.plan
    assert (plan.k, plan.kp, plan.Nb, plan.bw, plan.block_size) == (1024, 1024, 1003, 5, 16)
    assert dn.border_stats()[0] == 1024 and gram_plan(dn)[2] == 136
    dn.close()
    churn = _against_oracle(pgf, prob, (("Full", 2), ("Simplified", 2)), n_neg=m)
    assert churn > 0


# ------------------------------------------------------------------ 4: the Gram kernel alone
def read_gram(dn):
    from pygradflow_amd import _lib

    plan = dn._hd.plan
    Cm, Y, Gm = np.empty((plan.Nb, plan.kp)), np.empty((plan.Nb, plan.kp)), np.empty((plan.kp, plan.kp))
    rc = dn._lib.pgf_debug_border_gram(dn._hd.h, _lib.dptr(Cm), _lib.dptr(Y), _lib.dptr(Gm))
    _lib.check(rc, dn._hd.h, "pgf_debug_border_gram")
    return Cm, Y, Gm


@pytest.mark.parametrize("shape", [(65, 333, 2, 16), (257, 1003, 12, None)])
def test_gram_kernel_against_extended_precision(pgf, shape):
    """Every entry of the lower triangle of G = C' Y within gamma (|C|' |Y|)_ij of the product in
    np.longdouble, gamma = Nb u / (1 - Nb u): the bound of an Nb-term dot product in ANY order of
    summation, so it covers the MFMA's four-row steps and the chunking.  Padding zero.  Two factor
    phases on the same matrix: the same bits."""
    from pygradflow_amd import _lib

    k, Nb, bw, block = shape
    make = lambda: large(case(k, Nb, bw=bw, block=block))  # noqa: E731
    prob = make()
    n, m = prob.num_vars, prob.num_cons
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(n), np.zeros(m), 1.0, 1.0)
    plan = dn._hd.plan
    kp = plan.kp
    rows, chunks, tiles = gram_plan(dn)  # the handle's own launch plan
    assert tiles == (kp // 64) * (kp // 64 + 1) // 2 and (chunks - 1) * rows < Nb <= chunks * rows
    assert chunks >= 3 and Nb % rows != 0, (rows, chunks)  # at least three chunks, the last ragged
    assert dn._lib.pgf_debug_border_gram(dn._hd.h, None, None, None) == _lib.PGF_NOT_READY
    dn.step()
    Cm, Y, Gm = read_gram(dn)
    dn.close()
    assert np.count_nonzero(Cm) > 0 and np.isfinite(Y).all()
    assert not Cm[:, k:].any() and not Y[:, k:].any()
    assert not Gm[k:, :].any() and not Gm[:, k:].any()  # padding rows and columns
    assert not np.triu(Gm, 1).any()                     # (only the lower triangle is formed)
    ref = Cm.T.astype(np.longdouble) @ Y.astype(np.longdouble)
    mag = np.abs(Cm).T.astype(np.longdouble) @ np.abs(Y).astype(np.longdouble)
    u = np.longdouble(2.0) ** -53
    gamma = Nb * u / (1 - Nb * u)
    low = np.tril(np.ones((kp, kp), dtype=bool))
    err = np.abs(Gm.astype(np.longdouble) - ref)  # (bound and error both in extended precision)
    live = low & (mag > 0)
    worst = float(np.max(err[live] / (gamma * mag[live])))
    print(f"gram k {k} Nb {Nb}: {rows} rows x {chunks} chunks, worst error / bound {worst:.3f}")
    assert np.all(err[low] <= gamma * mag[low])
    # the product is not trivially zero where it should not be
    assert np.count_nonzero(Gm[:k, :k]) > k * k // 8
    dn2 = pgf.DeviceNewton(make(), "Full", np.zeros(n), np.zeros(m), 1.0, 1.0)
    dn2.step()
    C2, Y2, G2 = read_gram(dn2)
    dn2.close()
    assert np.array_equal(Cm, C2) and np.array_equal(Y, Y2) and np.array_equal(Gm, G2)


# ------------------------------------------------------------------ 5: panel slices against single solves
def test_panel_slices_against_repeated_solves(pgf, tmp_path):
    """Y = inv(B) C as 64-column slices of one panel solve (this process) and by k single solves
    (PGF_BORDER_MULTI=0, read once per process: a fresh child): the child meets the oracle on its
    own, and the two routes agree to 1e-12."""
    out = str(tmp_path / "repeated.npz")
    env = dict(os.environ, PGF_BORDER_MULTI="0")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=env, cwd=REPO,
                         capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    theirs = np.load(out)
    ours = device_trajectory(pgf, case1(), CASE1_POLICIES)
    assert len(ours) == len(theirs.files) == 18
    for i, v in enumerate(ours):
        err = G.rel_err(v, theirs[f"a{i}"])
        assert err <= 1e-12, (i, err)


def _child(out):
    import pygradflow_amd as pgf

    assert os.environ.get("PGF_BORDER_MULTI") == "0"
    prob = case1()
    _against_oracle(pgf, prob, CASE1_POLICIES, n_neg=prob.num_cons)
    traj = device_trajectory(pgf, case1(), CASE1_POLICIES)
    np.savez(out, **{f"a{i}": v for i, v in enumerate(traj)})


# ------------------------------------------------------------------ 6: the automatic border, k = 299
def test_multistate_ocp_automatic_border(pgf):
    from pygradflow_amd import problems

    prob = problems.multistate_ocp(300, 24, 8)
    prob.pgf_border = "auto"
    prob.pgf_border_limit = 1024
    n, m = prob.num_vars, prob.num_cons
    recs = oracle_run(prob, "Full", 2)
    assert [int(np.count_nonzero(r["mask"])) for r in recs] == [1855, 1439]
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(n), np.zeros(m), 1.0, 1.0)
    plan = dn._hd.plan
    assert dn.border_stats()[0] == 299 and plan.kp == 320 and plan.bw <= 64
    dn.close()
    _against_oracle(pgf, prob, (("Full", 2),), n_neg=m)


# ------------------------------------------------------------------ 7: the guard
@pytest.mark.parametrize("block", [16, 32])
def test_unstable_pivot_in_B_is_refined(pgf, block, monkeypatch):
    """test_border_edges_gpu.py's guard test at k = 80: a 1e-9 pivot inside B makes Y, hence S,
    inaccurate; band_refine iterates the whole large-border solve on the residual."""
    from pygradflow_amd import sparse

    # band_util.guard_case plans without a limit (plan_of): for the construction alone the small
    # border's cap is lifted -- the band rows' permutation, all it reads, does not depend on kp
    with monkeypatch.context() as mp:
        mp.setattr(sparse, "MAX_BORDER", 1024)
        prob, v = guard_case(80, block, 1e-9)
    large(prob)
    n, m = prob.num_vars, prob.num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    rec = oracle_run(prob, "Full", 1)[0]
    mask = rec["mask"]
    assert not mask.any()
    K = reduced_kkt(prob, mask)
    assert abs(K[v, v]) < 1e-8 and np.linalg.cond(K) < 1e5
    params = pgf.Params()
    it = pgf.Iterate(prob, params, x0, y0)
    sv = pgf.HipStepSolver(prob, params, it, 1.0, 1.0)
    assert sv.sparse
    sv.update_active_set(mask)
    sv.update_derivs(it)
    before = sv.refinement_stats()
    res = sv.solve(it)
    after = sv.refinement_stats()
    plan = sv._hd.plan
    assert (plan.k, plan.kp, plan.Nb, plan.block_size, plan.large) == (80, 128, 300, block, True)
    err = max(G.rel_err(res.dx, rec["dx"]), G.rel_err(res.dy, rec["dy"]))
    print(f"large-border guard block {block} v {v}: refined {before[0]} -> {after[0]}, last_rel_residual "
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


# ------------------------------------------------------------------ 8: singular S
def test_singular_schur_complement_is_an_error(pgf):
    """The last border variable decoupled with H[v, v] = -lambda: B is as regular as ever, K is
    singular through S alone (the dense LDL^T of S meets an exact zero pivot).  Neither front end
    may return a step, and the point has not moved."""
    from pygradflow_amd.errors import StepSolverError

    prob, v = singular_schur_wide(case(65, 333, bw=2, block=16))
    large(prob)
    n, m = prob.num_vars, prob.num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    mask = O.NewtonOracle(prob, "Full", x0, y0, 1.0, 1.0).solver.compute_active_set(O.PointData(prob, x0, y0))
    assert not mask[v]
    K = reduced_kkt(prob, mask)
    iv = int(np.count_nonzero(~mask[:v]))
    assert not K[iv].any()
    params = pgf.Params()
    it = pgf.Iterate(prob, params, x0, y0)
    sv = pgf.HipStepSolver(prob, params, it, 1.0, 1.0)
    sv.update_active_set(mask)
    sv.update_derivs(it)
    assert sv._hd.plan.large and sv._hd.plan.k == 65
    with pytest.raises(StepSolverError):
        sv.solve(it)
    sv.close()
    dn = pgf.DeviceNewton(prob, "Full", x0, y0, 1.0, 1.0)
    with pytest.raises(StepSolverError):
        dn.step()
    x, y = dn.point()
    dn.close()
    assert np.array_equal(x, x0) and np.array_equal(y, y0)


# ------------------------------------------------------------------ 9: against the dense route
def without_border(prob):
    from pygradflow_amd import problems

    return problems.LinearQuadraticProblem(prob.hess_sparse(), prob.q, prob.jac_sparse(), prob.b, prob.var_lb,
                                           prob.var_ub)


def test_linear_solves_agree_with_the_dense_route(pgf):
    prob, dense = case1(), without_border(case1())
    n, m = prob.num_vars, prob.num_cons
    mask = np.random.default_rng(9).uniform(size=n) < 0.4
    rng = np.random.default_rng(10)
    sols = []
    for p in (prob, dense):
        params = pgf.Params()
        it = pgf.Iterate(p, params, np.zeros(n), np.zeros(m))
        sv = pgf.HipStepSolver(p, params, it, 1.0, 1.0)
        assert sv.sparse == (p is prob)
        sv.update_active_set(mask)
        sv.update_derivs(it)
        view = sv.solver_for_tests()
        N = n - int(np.count_nonzero(mask)) + m
        if not sols:
            one, three = rng.standard_normal(N), rng.standard_normal((N, 3))
        sols.append((view.solve(one), view.solve(three), view.num_neg_eigvals()))
        if p is prob:
            assert sv.border_stats()[0] == 65
        sv.close()
    (a1, a3, an), (b1, b3, bn) = sols
    assert an == bn == m
    assert a3.shape == b3.shape == (N, 3)
    assert G.rel_err(a1, b1) <= TOL
    for j in range(3):
        assert G.rel_err(a3[:, j], b3[:, j]) <= TOL, j


def test_globalized_step_agrees_with_the_dense_route(pgf):
    prob, dense = case1(), without_border(case1())
    n, m = prob.num_vars, prob.num_cons
    out = []
    for p in (prob, dense):
        dn = pgf.DeviceNewton(p, "Globalized", np.zeros(n), np.zeros(m), 10.0, 1.0)
        assert dn.sparse == (p is prob)
        dn.step()
        out.append((dn.line_search(), dn.point(), dn.mask()))
        dn.close()
    (la, (xa, ya), ma), (lb, (xb, yb), mb) = out
    print("line search: large border", la["alpha"], la["trials"], "dense", lb["alpha"], lb["trials"])
    assert la["alpha"] == lb["alpha"] and la["trials"] == lb["trials"]
    assert np.array_equal(ma, mb)
    assert G.rel_err(xa, xb) <= TOL and G.rel_err(ya, yb) <= TOL


# ------------------------------------------------------------------ 10: refusals
def test_what_the_large_border_refuses(pgf):
    from pygradflow_amd import _lib, problems

    lib = _lib.load()
    INVALID = _lib.PGF_INVALID
    err = lambda h: lib.pgf_last_error(h)  # noqa: E731

    def newton(prob):
        return pgf.DeviceNewton(prob, "Full", np.zeros(prob.num_vars), np.zeros(prob.num_cons), 1.0, 1.0)

    # a wide handle (block 16, the split on) with a small border: sizes outside 65 .. 1024
    dn = newton(case(6, 333, bw=2, block=16))
    h = dn._hd.h
    for k in (64, 1025, 0, -1):
        assert lib.pgf_sparse_set_border_large(h, k) == INVALID and err(h) == b"large border size must be 65..1024"
    assert dn.border_stats()[0] == 6  # (refused: nothing changed)
    assert lib.pgf_debug_border_gram(h, None, None, None) == INVALID
    assert lib.pgf_sparse_set_border(h, 65) == INVALID  # the small entry point keeps its limit
    # ... with the split off
    assert lib.pgf_sparse_set_factor_split(h, 0) == _lib.PGF_OK
    assert lib.pgf_sparse_set_border_large(h, 65) == INVALID
    assert err(h) == b"a large border needs the factor / solve split"
    assert lib.pgf_sparse_set_factor_split(h, 1) == _lib.PGF_OK
    dn.close()
    # a block-8 handle
    dn = newton(case(6, 333, bw=2))
    assert dn._hd.plan.block_size == 8
    assert lib.pgf_sparse_set_border_large(dn._hd.h, 65) == INVALID
    assert err(dn._hd.h) == b"a large border needs a wide remainder (block size 16, 32 or 64)"
    dn.close()
    # a dense handle
    dense = newton(problems.dense_qp(8, 2, seed=0))
    assert lib.pgf_sparse_set_border_large(dense._hd.h, 65) == INVALID
    assert lib.pgf_debug_border_gram(dense._hd.h, None, None, None) == INVALID
    dense.close()
    # with a large border: no way back to the narrow route or to the fused reduction
    a, b = newton(case1()), newton(case1())
    for dn in (a, b):
        h = dn._hd.h
        assert dn.border_stats()[0] == 65
        assert lib.pgf_sparse_set_factor_split(h, 0) == INVALID
        assert err(h) == b"a large border needs the factor / solve split"
        assert lib.pgf_sparse_set_block_size(h, 8) == INVALID
        assert err(h) == b"a large border needs a wide remainder (block size 16, 32 or 64)"
        assert lib.pgf_sparse_set_block_size(h, 16) == _lib.PGF_OK
    # a batch of such handles, under every flag a bordered wide batch could ask for
    arr = (C.c_void_p * 2)(a._hd.h, b._hd.h)
    out = C.c_void_p()
    flags = _lib.BATCH_WIDE_BAND | _lib.BATCH_BORDER | _lib.BATCH_WIDE_BORDER
    assert lib.pgf_batch_create_ex(arr, 2, flags, C.byref(out)) == INVALID and not out.value
    assert err(a._hd.h) == b"batch: a large border (more than 64 nodes) cannot join a device batch"
    assert lib.pgf_batch_create(arr, 2, C.byref(out)) == INVALID and not out.value
    # the refusals left the handles as they were
    rec = oracle_run(case1(), "Full", 1)[0]
    for dn in (a, b):
        dn.step()
        x, y = dn.point()
        assert G.rel_err(x, rec["xn"]) <= TOL and G.rel_err(y, rec["yn"]) <= TOL
        dn.close()
    # the Python front end
    prob = case1()
    prob.pgf_band_split = False
    with pytest.raises(ValueError, match="pgf_band_split"):
        newton(prob)
    prob = large(case(65, 333, bw=2, block=8))
    with pytest.raises(ValueError, match="pgf_band_block"):
        newton(prob)
    with pytest.raises(ValueError, match="at most 64"):  # no limit: as ever
        newton(case(65, 333, bw=2, block=16))


if __name__ == "__main__":
    _child(sys.argv[1])
