"""Wide bands (block sizes 16, 32, 64) in the banded device batch (csrc/pgf_band_wide.hip,
csrc/pgf_api_band_batch.hip): instances of one pattern on the wide route share every launch of the
Newton step, each in the phase its own state asks for -- the reduction, or with the factor / solve
split on the solve phase against the factors it kept.

The references are ``sequential=True`` (the same instances one by one through their own handles) and
the CPU oracle, with the bars of band_batch_util.py.  Every batch here is created
with ``wide_band=True`` (pgf_batch_create_ex with PGF_BATCH_WIDE_BAND).  The per-instance phase is read
from ``band_wide_stats()``: (reductions, solve phases) each instance's workgroups ran, and the steps
enqueued without inversion launches.
"""

import functools

import numpy as np
import pytest

from tests import golden_util as G
from tests.band_batch_util import against_oracle, handle_stats, make_batch, same_as_sequential, same_step
from tests.band_util import (TOL, forced, head_of_first_eliminated, level_one_solve, mask_change_steps,
                             mask_changes, multistate_ocp, normwise, plan_of, refined_solve, wide_band_problem)

pytestmark = pytest.mark.gpu

POLICIES = ("Simplified", "Full", "ActiveSet")
NEW_REFUSAL = "must share the block size and the factor / solve split"

_batch = functools.partial(make_batch, wide_band=True)


# ------------------------------------------------------------------ 1: block-count edges
EDGE_CASES = [((T, 4, 2, T), 16) for T in (1, 3, 4, 5, 47, 48, 52)] + [
    ((2, 6, 3, 0), 32), ((2, 6, 3, 0), 64), ((30, 6, 3, 0), 32), ((30, 6, 3, 0), 64)]


@pytest.mark.parametrize("args,block", EDGE_CASES)
def test_block_count_edges(pgf, args, block):
    """multistate_ocp(T, 4, 2) at B = 16: 1, 2, 3, 4, 30, 30, 33 blocks -- the single block, a missing
    right neighbour at every level, both sides of 32; (2, 6, 3) and (30, 6, 3) at B = 32, 64.  Three
    instances with their own seeds.  Full for 2 steps, then fresh instances with Simplified for 3: one
    reduction, two solve phases per instance, and the last two steps enqueue no inversion."""
    T, nx, nu, seed = args
    probs = [multistate_ocp(T, nx, nu, seed + 7 * i, block) for i in range(3)]
    assert plan_of(probs[0]).block_size == block

    def opened(bd):
        assert bd.band_block == block

    def after(bd, pol, steps):
        red, sol, lean = bd.band_wide_stats()
        if pol == "Full":
            assert list(red) == [2] * 3 and not sol.any() and lean == 0, (red, sol, lean)
        else:
            assert list(red) == [1] * 3 and list(sol) == [2] * 3 and lean == 2, (red, sol, lean)

    same_as_sequential(_batch, probs, (("Full", 2), ("Simplified", 3)), opened, after)


# ------------------------------------------------------------------ 2: the oracle
def test_against_the_oracle(pgf):
    """5 instances of multistate_ocp(12, 8, 4): N = 240, half-bandwidth 22, block 32 by the plan."""
    probs = [multistate_ocp(12, 8, 4, i) for i in range(5)]
    plan = plan_of(probs[0])
    n, m = probs[0].num_vars, probs[0].num_cons
    assert (plan.bw, plan.block_size, n + m) == (22, 32, 240)
    for pol in ("Full", "ActiveSet"):  # (Simplified keeps its mask by definition)
        assert any(mask_changes(p, pol, 3) > 0 for p in probs)

    def opened(bd):
        assert bd.band_block == 32

    against_oracle(_batch, probs, tuple((p, 3) for p in POLICIES), opened=opened)


# ------------------------------------------------------------------ 3: per-instance phase
def test_each_instance_takes_its_own_phase(pgf):
    """Instances whose masks settle at different steps.  Under Full every instance refactorises every
    step by definition (PGF_STEP_REFACTOR), so its counters are the number of steps; the phases
    differ between instances under ActiveSet, which reduces exactly when the instance's mask changed.
    Seeds 0, 1, 2 of multistate_ocp(12, 4, 2): at step 2 the oracle's mask of instance 0 stays while
    those of instances 1 and 2 change -- one instance solves while the others reduce, in ONE launch
    sequence.  After every step the batch's per-instance counters equal the difference of the single
    handles' band_stats() in the sequential run."""
    steps = 4
    probs = [multistate_ocp(12, 4, 2, s) for s in (0, 1, 2)]
    assert plan_of(probs[0]).block_size == 16
    # [instance][step]: the step reduces
    changed = np.array([[True] + mask_change_steps(p, "ActiveSet", steps) for p in probs])
    assert any(changed[:, k].any() and not changed[:, k].all() for k in range(1, steps)), changed
    for pol in ("ActiveSet", "Full"):
        bd, ref = _batch(probs, pol), _batch(probs, pol, sequential=True)
        h0 = handle_stats(ref, ("band", "refined"))
        for k in range(steps):
            same_step(bd, ref, (pol, k))
            red, sol, lean = bd.band_wide_stats()
            hred, hsol, hrefined = dh = handle_stats(ref, ("band", "refined")) - h0
            # (a refinement step of the guard is one more solve phase on the handle; the batch runs
            # its corrections on the handle too, outside its own counters)
            assert np.array_equal(red, hred) and np.array_equal(sol, hsol - hrefined), (pol, k, red, sol, dh)
            want = changed[:, : k + 1].sum(axis=1) if pol == "ActiveSet" else np.full(3, k + 1)
            assert np.array_equal(red, want) and np.array_equal(red + sol, np.full(3, k + 1)), (pol, k, red, sol)
            assert lean == 0  # (a step that recomputes the mask may reduce: the inversions are enqueued)
        bd.close()
        ref.close()


# ------------------------------------------------------------------ 4: split off
@pytest.mark.parametrize("args,block", [((5, 4, 2), 16), ((30, 6, 3), 32)])
def test_split_off_gives_the_same_bits_and_no_solve_phase(pgf, args, block):
    out = {}
    for split in (True, False):
        probs = [multistate_ocp(*args, 3 + i, block, split=split) for i in range(3)]
        bd, ref = _batch(probs, "Simplified"), _batch(probs, "Simplified", sequential=True)
        for k in range(3):
            same_step(bd, ref, (split, k))
        red, sol, lean = bd.band_wide_stats()
        if split:
            assert list(red) == [1] * 3 and list(sol) == [2] * 3 and lean == 2, (red, sol, lean)
        else:
            assert list(red) == [3] * 3 and not sol.any() and lean == 0, (red, sol, lean)
        out[split] = bd.points() + (bd.masks(),)
        bd.close()
        ref.close()
    for a, b in zip(out[True], out[False]):
        assert np.array_equal(a, b)


def test_mixed_split_or_block_size_is_refused(pgf):
    on, off = multistate_ocp(5, 4, 2, 0, 16, split=True), multistate_ocp(5, 4, 2, 1, 16, split=False)
    with pytest.raises(ValueError, match=NEW_REFUSAL):
        _batch([on, off], "Full")
    with pytest.raises(ValueError, match=NEW_REFUSAL):
        _batch([off, on], "Full")
    b16, b32 = multistate_ocp(5, 4, 2, 0, 16), multistate_ocp(5, 4, 2, 1, 32)
    assert plan_of(b16).pattern_hash() == plan_of(b32).pattern_hash()
    assert (plan_of(b16).block_size, plan_of(b32).block_size) == (16, 32)
    with pytest.raises(ValueError, match=NEW_REFUSAL):
        _batch([b16, b32], "Full")
    # and the handles are none the worse for it
    pair = [b16, multistate_ocp(5, 4, 2, 1, 16)]
    bd, ref = _batch(pair, "Full"), _batch(pair, "Full", sequential=True)
    same_step(bd, ref, "after the refusals")
    bd.close()
    ref.close()


# ------------------------------------------------------------------ 5: per-instance outer steps
@pytest.mark.parametrize("pol", ["Full", "ActiveSet"])
def test_per_instance_outer_steps_rejection_and_freezing(pgf, pol):
    """The scenario of test_band_batch_gpu.py's test of the same name on multistate_ocp(12, 4, 2).
    A frozen instance's counters do not move; after advance_outer_each (a new lambda: a new matrix)
    every instance reduces once, whatever the policy."""
    probs = [multistate_ocp(12, 4, 2, 20 + i) for i in range(3)]
    dt = np.array([0.5, 1.0, 2.0])
    bd, ref, free = _batch(probs, pol), _batch(probs, pol, sequential=True), _batch(probs, pol)
    assert bd.band_block == 16
    for run in (bd, ref, free):
        run.step_local()
        run.advance_outer_each(dt, 1.0)
    outer = bd.points()
    c0 = bd.band_wide_stats()
    for k in range(2):
        same_step(bd, ref, ("dt", k))
        free.step_local()
        if k == 0:  # the first step behind the new outer step
            c1 = bd.band_wide_stats()
            assert list(c1[0] - c0[0]) == [1] * 3 and list(c1[1] - c0[1]) == [0] * 3, (c0, c1)
    # instance 1 is rejected: back to its outer point, bit for bit; the others go on
    moved, m0 = bd.points(), bd.masks()
    for run in (bd, ref, free):
        run.advance_outer_each(dt / 2, 1.0, accepted=[True, False, True])
    x, y = bd.points()
    assert np.array_equal(x[1], outer[0][1]) and np.array_equal(y[1], outer[1][1])
    assert np.array_equal(x[0], moved[0][0]) and np.array_equal(x[2], moved[0][2])
    assert not np.array_equal(x[1], moved[0][1])
    # instance 1 frozen: its point, mask and counters stay, the others step as if nothing were frozen
    bd.set_frozen([0, 1, 0])
    ref.set_frozen([0, 1, 0])
    c0 = bd.band_wide_stats()
    for k in range(2):
        st, _, df = bd.step_local()
        ref.step_local()
        free.step_local()
        assert not st.any() and df[1] == 0.0
        c1 = bd.band_wide_stats()
        assert c1[0][1] == c0[0][1] and c1[1][1] == c0[1][1], (k, c0, c1)
        for i in (0, 2):
            assert (c1[0][i] - c0[0][i]) + (c1[1][i] - c0[1][i]) == k + 1, (k, i, c0, c1)
            assert c1[0][i] - c0[0][i] >= 1  # (the first step behind the new outer step reduced)
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


# ------------------------------------------------------------------ 6: singular instance
@pytest.mark.parametrize("pol", ["Full", "Simplified"])
@pytest.mark.parametrize("block", [16, 64])
def test_one_singular_instance_does_not_spoil_the_batch(pgf, block, pol):
    """The construction of test_band_split_gpu.py::test_zero_pivot_leaves_no_kept_factor in the middle
    instance of three: K[v, v] = 0 at the head of block 1, on the pattern of the good ones.  The bad
    instance reports PGF_SINGULAR step after step, keeps its point and reduces again every step (a bad
    pivot never leaves a kept factor); the neighbours are those of a batch of the two good ones --
    under Simplified they solve against their kept factors in the step in which the bad one reduces."""
    from pygradflow_amd import _lib

    n = 300
    rng = np.random.default_rng(8)
    ds = [2.5 + rng.uniform(0.0, 0.5, n) for _ in range(3)]
    v = head_of_first_eliminated(wide_band_problem(n, ds[1], 2, block), block)
    good = wide_band_problem(n, ds[1].copy(), 2, block)
    ds[1][v] = -1.0  # lambda = 1: K[v, v] = 0
    probs = [wide_band_problem(n, ds[i], 1 + i, block) for i in range(3)]
    K = probs[1].hess_sparse().toarray() + np.eye(n)
    assert K[v, v] == 0.0 and np.linalg.cond(K) < 1e6
    assert plan_of(probs[1]).pattern_hash() == plan_of(good).pattern_hash() == plan_of(probs[0]).pattern_hash()
    assert plan_of(probs[1]).block_size == block
    bd, two = _batch(probs, pol), _batch([probs[0], probs[2]], pol)
    for k in range(2):
        st, _, _ = bd.step_local()
        st2, _, _ = two.step_local()
        assert list(st) == [0, _lib.PGF_SINGULAR, 0] and not st2.any(), (k, st, st2)
        (x, _), (x2, _) = bd.points(), two.points()
        assert not x[1].any()  # the point it started from
        assert np.array_equal(x[0], x2[0]) and np.array_equal(x[2], x2[1]), k
    red, sol, lean = bd.band_wide_stats()
    assert red[1] == 2 and sol[1] == 0 and lean == 0, (red, sol, lean)
    if pol == "Simplified":
        assert list(red[[0, 2]]) == [1, 1] and list(sol[[0, 2]]) == [1, 1], (red, sol)
        assert two.band_wide_stats()[2] == 1
    else:
        assert list(red[[0, 2]]) == [2, 2] and not sol.any(), (red, sol)
    bd.close()
    two.close()


# ------------------------------------------------------------------ 7: unstable pivot
def test_an_unstable_pivot_in_one_instance_is_repaired_on_its_handle(pgf):
    """The construction of test_band_split_gpu.py::test_guard_refines_through_the_kept_factors in one
    instance of three at block size 16: a tiny K[v, v] at the head of block 1, which level one inverts
    as it stands.  The pivot is 1e-10 and not that test's 1e-9: at 1e-9 the emulated plain solve below
    misses refine_tol by a factor of 4 only (4.1e-11), at 1e-10 by 70 (7.0e-10), and one refinement
    step still brings it to 1.4e-16.

    Measured: the plain solve on the device misses refine_tol, the guard repairs the instance on its
    handle with solve phases against the factors the batch's reduction left (no reduction there), and
    the batch's own reductions counter of the instance stays 1."""
    n, bw, block, eps = 300, 12, 16, 1e-10
    rng = np.random.default_rng(7)
    ds = [2.5 + rng.uniform(0.0, 0.5, n) for _ in range(3)]
    v = head_of_first_eliminated(wide_band_problem(n, ds[1], 1, block), block)
    ds[1][v] = -1.0 + eps  # lambda = 1: K[v, v] = eps
    probs = [wide_band_problem(n, ds[i], 1 + i, block) for i in range(3)]
    plan = plan_of(probs[1])
    assert plan.bw == bw and plan.block_size == block
    K = probs[1].hess_sparse().toarray() + np.eye(n)
    assert abs(K[v, v]) < 1e-9 and np.linalg.cond(K) < 1e5
    # on the CPU first: the plain float64 solve in the reduction's order misses refine_tol by at least
    # 10 x, one refinement step with the same solve brings it below
    refine_tol = 1e-11
    perm = np.argsort(plan.pos)
    Kp, f = K[np.ix_(perm, perm)], probs[1].q[perm]
    s0 = level_one_solve(Kp, f, block)
    assert normwise(Kp, s0, f) >= 10 * refine_tol
    s1 = s0 + level_one_solve(Kp, f - Kp @ s0, block)
    assert normwise(Kp, s1, f) <= refine_tol
    ref, plain = refined_solve(K, probs[1].q)
    assert G.rel_err(plain, ref) < 1e-11
    bd = _batch(probs, "Full")
    assert bd.repaired() == 0 and bd.band_block == block
    h0 = bd.solvers[1].band_stats()
    st, nn, df = bd.step_local()
    x, _ = bd.points()
    red, sol, _ = bd.band_wide_stats()
    h1 = bd.solvers[1].band_stats()
    print(f"status {st}, repaired {bd.repaired()}, x error {G.rel_err(x[1], -ref):.3e}, batch counters "
          f"{red} {sol}, handle {tuple(a - b for a, b in zip(h1, h0))}")
    neg = int((np.linalg.eigvalsh(K) < 0).sum())
    assert neg == 1 and not st.any() and list(nn) == [0, neg, 0]
    assert bd.repaired() >= 1
    assert G.rel_err(x[1], -ref) <= TOL
    assert abs(df[1] - np.linalg.norm(ref)) <= 1e-9 * np.linalg.norm(ref)
    for i in (0, 2):
        Ki = probs[i].hess_sparse().toarray() + np.eye(n)
        assert G.rel_err(x[i], -np.linalg.solve(Ki, probs[i].q)) <= TOL
    # the corrections were solve phases on the handle, against the factors of the batch's one reduction
    assert list(red) == [1, 1, 1] and not sol.any()
    assert h1[0] - h0[0] == 0 and h1[1] - h0[1] >= 1, (h0, h1)
    # the step after a repair: from the repaired point, evaluated afresh
    st, _, _ = bd.step_local()
    x2, _ = bd.points()
    assert not st.any() and G.rel_err(x2[1], -ref) <= TOL
    bd.close()


# ------------------------------------------------------------------ 8: narrow and default behaviour
def test_the_flag_changes_nothing_for_a_narrow_batch_and_wide_needs_it(pgf):
    from pygradflow_amd import problems

    def narrow():
        return [forced(problems.box_qp(264, seed=30 + i)) for i in range(3)]

    probs = narrow()
    assert plan_of(probs[0]).block_size == 8
    for pol, steps in (("Full", 2), ("Simplified", 2)):
        a, b = _batch(probs, pol, wide_band=True), _batch(probs, pol, wide_band=False)
        assert a.band and b.band and a.band_block == b.band_block == 8
        for k in range(steps):
            sa, sb = a.step_local(), b.step_local()
            for u, w in zip(sa, sb):
                assert np.array_equal(u, w), (pol, k)
            assert np.array_equal(a.masks(), b.masks())
            for u, w in zip(a.points(), b.points()):
                assert np.array_equal(u, w), (pol, k)
        assert a.band_stats() == b.band_stats()
        for run in (a, b):
            red, sol, lean = run.band_wide_stats()
            assert not red.any() and not sol.any() and lean == 0
            run.close()
    # the split is a matter of the wide route: narrow instances may differ in it, as before
    mixed = narrow()
    mixed[1].pgf_band_split = False
    for flag in (False, True):
        a, b = _batch(mixed, "Full", wide_band=flag), _batch(probs, "Full", wide_band=False)
        st, _, _ = a.step_local()
        b.step_local()
        assert not st.any() and np.array_equal(a.points()[0], b.points()[0]), flag
        a.close()
        b.close()
    wide = [multistate_ocp(12, 4, 2, i) for i in range(2)]
    with pytest.raises(ValueError, match="wide band"):
        _batch(wide, "Full", wide_band=False)


# ------------------------------------------------------------------ 9: batch of one, and 70 instances
@pytest.mark.parametrize("pol,steps", [("Full", 2), ("Simplified", 3)])
def test_batch_of_one_equals_the_single_handle(pgf, pol, steps):
    prob = multistate_ocp(12, 4, 2, 5)
    n, m = prob.num_vars, prob.num_cons
    bd = _batch([prob], pol)
    dn = pgf.DeviceNewton(prob, pol, np.zeros(n), np.zeros(m), 1.0, 1.0)
    assert bd.band and dn.sparse and bd.band_block == 16
    for k in range(steps):
        st, nn, df = bd.step_local()
        d1, n1 = dn.step()
        x, y = bd.points()
        x1, y1 = dn.point()
        assert st[0] == 0 and nn[0] == n1 and abs(df[0] - d1) <= 1e-14 * abs(d1), k
        assert np.array_equal(x[0], x1) and np.array_equal(y[0], y1), k
        assert np.array_equal(bd.masks()[0], dn.mask()), k
    bd.close()
    dn.close()


def test_seventy_tiny_instances(pgf):
    """More instances than any grid.x of the sequence, several per CU: multistate_ocp(3, 4, 2), N = 30,
    two blocks of 16."""
    probs = [multistate_ocp(3, 4, 2, i) for i in range(70)]
    assert plan_of(probs[0]).block_size == 16
    for pol, steps in (("Full", 2), ("Simplified", 2)):
        bd, ref = _batch(probs, pol), _batch(probs, pol, sequential=True)
        for k in range(steps):
            same_step(bd, ref, (pol, k))
        red, sol, _ = bd.band_wide_stats()
        assert np.all(red + sol == steps)
        bd.close()
        ref.close()
