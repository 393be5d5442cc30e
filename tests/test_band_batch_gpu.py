"""Banded device batch (csrc/pgf_sparse.hip, csrc/pgf_api_band_batch.hip): many banded instances
of one sparsity pattern advanced by one launch sequence per Newton step.

Two references, with the bars of band_batch_util.py: ``sequential=True``, which drives the same
instances one by one through their own handles (both routes run the same device functions in the
same order), and the CPU oracle.  Shapes are the smallest that reach each kernel branch.
"""

import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps

from tests import golden_util as G
from tests.band_batch_util import against_oracle, make_batch, same_as_sequential, same_step
from tests.band_util import (TOL, band_problem, bordered_lq, decoupled, forced, head_of_first_eliminated,
                             level_one_solve, mask_changes, multistate_ocp, normwise, plan_of, refined_solve)

pytestmark = pytest.mark.gpu

POLICIES = ("Simplified", "Full", "ActiveSet")
ORACLE_STEPS = tuple((p, 3) for p in POLICIES)

_batch = make_batch


# ------------------------------------------------------------------ 1: the batch exists
def test_banded_instances_form_a_device_batch_and_take_the_batched_route(pgf):
    from pygradflow_amd import problems

    probs = [forced(problems.box_qp(264, seed=i)) for i in range(3)]
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
    return [forced(make(size, seed=size + 7 * i)) for i in range(B)]


@pytest.mark.parametrize("kind,size", [("box", n) for n in (7, 9, 256, 257, 513, 1033)]
                         + [("ocp", m) for m in (3, 85, 86, 171, 343)])
def test_same_as_one_by_one_on_every_branch_of_the_launch_plan(pgf, kind, size):
    """Block counts 1 (ragged), 2, 32 (the most the tail takes), 33 (single level, odd), 65 (pair),
    130 (pair whose last workgroup lies beyond nb, plus single s = 4) and 2, 32, 33, 65, 129: the
    table of test_band_narrow_gpu.py::test_block_counts_on_every_branch_of_the_launch_plan."""
    probs = _sweep_problems(kind, size)
    plan = plan_of(probs[0])
    assert plan.block_size == 8 and plan.bw <= 8
    same_as_sequential(_batch, probs)


# ------------------------------------------------------------------ 3, 4: against the oracle
def _ocp(i):
    return multistate_ocp(60, 3, 1, i)  # bw 7, N = 420, boxed controls


def test_against_the_oracle_constrained(pgf):
    probs = [_ocp(i) for i in range(5)]
    assert plan_of(probs[0]).bw == 7 and probs[0].num_vars + probs[0].num_cons == 420
    for pol in ("Full", "ActiveSet"):  # (Simplified keeps its mask by definition)
        assert any(mask_changes(p, pol, 3) > 0 for p in probs)
    assert against_oracle(_batch, probs, ORACLE_STEPS) > 0


def test_against_the_oracle_box_qp(pgf):
    from pygradflow_amd import problems

    probs = [forced(problems.box_qp(600, seed=i)) for i in range(5)]
    for pol in ("Full", "ActiveSet"):
        assert any(mask_changes(p, pol, 3) > 0 for p in probs)
    assert against_oracle(_batch, probs, ORACLE_STEPS) > 0


def test_values_differ_per_instance_not_only_vectors(pgf):
    """H_i = (1 + i / 4) H and J_i = (1 - i / 8) J on one pattern."""
    from pygradflow_amd import problems

    base = _ocp(0)
    H, J = base.hess_sparse(), base.jac_sparse()
    probs = [forced(problems.LinearQuadraticProblem(sps.csr_matrix(H * (1 + i / 4)), base.q,
                                                     sps.csr_matrix(J * (1 - i / 8)), base.b,
                                                     base.var_lb, base.var_ub)) for i in range(4)]
    assert against_oracle(_batch, probs, ORACLE_STEPS) > 0


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
    probs = [forced(_bandwidth_case(bw, k)) for k in range(2)]
    plan = plan_of(probs[0])
    assert plan.bw == bw and plan.block_size == 8
    same_as_sequential(_batch, probs)


# ------------------------------------------------------------------ 6: B edge cases
def test_batch_of_one_equals_the_single_handle(pgf):
    from pygradflow_amd import problems

    prob = forced(problems.box_qp(264, seed=5))
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

    probs = [forced(problems.box_qp(40, seed=i, bound={3: 0.0, 5: np.inf}.get(i, 0.5))) for i in range(70)]
    bd, ref = _batch(probs, "Full"), _batch(probs, "Full", sequential=True)
    for k in range(2):
        same_step(bd, ref, k)
    mk = bd.masks()
    assert mk[3].all() and not mk[5].any() and mk[0].any() and not mk[0].all()
    bd.close()
    ref.close()
    assert against_oracle(_batch, probs[:8], (("Full", 2), ("Simplified", 1))) > 0


# ------------------------------------------------------------------ 7: per-instance outer steps
def test_per_instance_outer_steps_rejection_and_freezing(pgf):
    from pygradflow_amd import problems

    probs = [forced(problems.box_qp(264, seed=20 + i)) for i in range(3)]
    dt = np.array([0.5, 1.0, 2.0])
    bd, ref, free = _batch(probs, "Full"), _batch(probs, "Full", sequential=True), _batch(probs, "Full")
    for run in (bd, ref, free):
        run.step_local()
        run.advance_outer_each(dt, 1.0)
    outer = bd.points()
    for k in range(2):
        same_step(bd, ref, ("dt", k))
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
def test_one_singular_instance_does_not_spoil_the_batch(pgf):
    from pygradflow_amd import _lib

    n, v = 600, 333
    goods = [forced(band_problem(n, 2.5 + np.random.default_rng(9 + i).uniform(0.0, 0.5, n), 3 + i, 5))
             for i in range(3)]
    bad = forced(decoupled(goods[1], v))
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
def test_an_unstable_pivot_in_one_instance_is_repaired_on_its_handle(pgf):
    """The recipe of test_band_narrow_gpu.py::test_narrow_unstable_pivot_is_refined at bw 5 and block
    size 8: a tiny K[v, v] at the head of block 1, which level one inverts as it stands.  The pivot
    is 1e-11 and not that test's 1e-9: at 1e-9 the emulated plain solve below misses refine_tol by a
    factor of 3 only (3.0e-11), at 1e-11 by 250 (2.5e-9), and one refinement step still brings it
    to 5e-17."""
    n, bw, eps = 300, 5, 1e-11
    rng = np.random.default_rng(7)
    ds = [2.5 + rng.uniform(0.0, 0.5, n) for _ in range(3)]
    v = head_of_first_eliminated(forced(band_problem(n, ds[1], 1, bw)), 8)
    ds[1][v] = -1.0 + eps  # lambda = 1: K[v, v] = eps
    probs = [forced(band_problem(n, ds[i], 1 + i, bw)) for i in range(3)]
    plan = plan_of(probs[1])
    assert plan.bw == bw and plan.block_size == 8
    K = probs[1].hess_sparse().toarray() + np.eye(n)
    assert abs(K[v, v]) < 1e-8 and np.linalg.cond(K) < 1e5
    # on the CPU first: the plain float64 solve in the reduction's order misses refine_tol, one
    # refinement step with the same solve brings it below
    refine_tol = 1e-11
    perm = np.argsort(plan.pos)
    Kp, f = K[np.ix_(perm, perm)], probs[1].q[perm]
    s0 = level_one_solve(Kp, f)
    assert normwise(Kp, s0, f) > refine_tol
    s1 = s0 + level_one_solve(Kp, f - Kp @ s0)
    assert normwise(Kp, s1, f) <= refine_tol
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
        _batch([forced(problems.box_qp(n, seed=1)), problems.box_qp(n, seed=2, dense=True)], "Full")
    with pytest.raises(ValueError, match="dense and banded"):
        _batch([problems.box_qp(n, seed=2, dense=True), forced(problems.box_qp(n, seed=1))], "Full")
    with pytest.raises(ValueError, match="one sparsity pattern"):
        _batch([forced(problems.box_qp(n, seed=1)), forced(band_problem(n, d, 1, 3))], "Full")
    wide = [forced(problems.multistate_ocp(50, 8, 4, seed=i)) for i in range(2)]
    assert plan_of(wide[0]).block_size > 8
    with pytest.raises(ValueError, match="wide band"):
        _batch(wide, "Full")
    with pytest.raises(ValueError, match="bordered band"):
        _batch([bordered_lq(100, 3, 10, 1, 1, seed=i) for i in range(2)], "Full")
    with pytest.raises(ValueError, match=r"one \(n, m\)"):
        _batch([forced(problems.box_qp(n, seed=1)), forced(problems.box_qp(n + 1, seed=1))], "Full")
    bd = _batch([forced(problems.box_qp(n, seed=i)) for i in range(2)], "Full")
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
        same_step(bd, ref, k)
    assert close(bd.measures(), ref.measures()) and close(bd.residual_norms_local(), ref.residual_norms_local())
    assert bd.measures()[:, 3].max() > 0.0  # (multipliers have moved: the measures are not all zero)
    # the stream the launches went to is the batch's own
    s = C.c_void_p()
    assert bd._lib.load().pgf_batch_stream(bd._b, C.byref(s)) == 0 and s.value
    bd.close()
    ref.close()
