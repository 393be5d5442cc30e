"""Refinement inside the device-resident controller's loop on band batches (PGF_BATCH_CTL_REFINE
with PGF_BATCH_BAND_CTL; band_batch_enqueue_refine in csrc/pgf_api_batch_ctl.hip): an instance whose
solve misses its handle's refine_tol is refined on the device, by the device functions and in the
order of band_refine on its handle, instead of rejected with 2 lambda.

The reference is the host-driven ``BatchedDistanceRatioController`` on a twin batch, which repairs
such an instance on its handle (``repaired() >= 1``).  Bars, with the helpers of
test_band_batch_ctl_gpu.py: accept flags equal, lambda used and lambda next within rtol 1e-12, points
within 1e-10; after ONE iteration from the same lambda the points are ``np.array_equal`` (lambda used
is lamb_init exactly, the point does not depend on lambda next, and the refinement is the handle's
kernel for kernel).  Every unstable construction is checked on the CPU first: the plain solve in the
reduction's order misses refine_tol = 1e-11 by at least 10 x and one round brings it below."""

import numpy as np
import pytest

from tests.band_batch_util import make_batch, phases
from tests.band_util import (band_problem, bordered_lq, decoupled, forced, guard_case, head_of_first_eliminated,
                             level_one_solve, normwise, plan_of, reduced_kkt, wide_band_problem)
from tests.test_band_batch_ctl_gpu import SLOW_RED, _host_run, _same_log, _same_points, _unstable

from pygradflow_amd import step_control as SC
from pygradflow_amd.params import Params

pytestmark = pytest.mark.gpu

REFINE_TOL = 1e-11


def _one_round_cures(Kp, f, block, factor=10.0):
    """The premise of the module docstring on the permuted matrix (of B, under a border)."""
    s0 = level_one_solve(Kp, f, block)
    first = normwise(Kp, s0, f)
    s1 = s0 + level_one_solve(Kp, f - Kp @ s0, block)
    assert first >= factor * REFINE_TOL and normwise(Kp, s1, f) <= REFINE_TOL, (first, normwise(Kp, s1, f))


def _premise(prob, block):
    """An unbordered instance with m = 0 at lambda = 1 from zero: K = H + I, rhs = -q."""
    plan = plan_of(prob)
    assert plan.block_size == block and plan.k == 0
    K = prob.hess_sparse().toarray() + np.eye(prob.num_vars)
    assert np.linalg.cond(K) < 1e5
    perm = np.argsort(plan.pos)
    _one_round_cures(K[np.ix_(perm, perm)], prob.q[perm], block)


def _premise_bordered(prob, v, block):
    """guard_case: the band part B of K in the plan's order, whose block 1 level one inverts as it
    stands, with the band part of the right-hand side.  The emulated solve with B alone misses
    refine_tol by 2.7 x, 5.1 x and 6.1 x at block 8, 16 and 64 (2.7e-11, 5.1e-11, 6.1e-11; one round:
    below 2e-16), not by 10 x as the unbordered constructions do: the bar here is 2 x.  That the
    device's bordered solve misses it too is what ``repaired() >= 1`` on the host-driven twin and
    the refinement counters assert."""
    plan = plan_of(prob)
    assert plan.block_size == block and plan.k == 1 and plan.Nb == 300
    K = reduced_kkt(prob, np.zeros(prob.num_vars, dtype=bool))
    assert abs(K[v, v]) < 1e-8 and np.linalg.cond(K) < 1e5
    perm = np.argsort(plan.pos)[: plan.Nb]
    f = np.concatenate([-prob.q, prob.b])[perm]
    _one_round_cures(K[np.ix_(perm, perm)], f, block, factor=2.0)


def _dev(probs, par, iters, pol="Full", before_init=None, **flags):
    flags.setdefault("ctl_refine", True)
    bd = make_batch(probs, pol, band_ctl=True, **flags)
    if before_init is not None:
        before_init(bd)
    dev = SC.DeviceResidentDistanceRatioController(bd, par, rho=1.0, max_iterations=iters)
    dev.run(iters)
    return bd, dev


def _refined(bd, which, count):
    """Instance ``which`` refined at least one step, by one or two rounds each; the others none."""
    ref, rnd = bd.ctl_refine_stats()
    others = [i for i in range(count) if i != which]
    assert ref[which] >= 1 and 1 <= rnd[which] <= 2 * ref[which], (ref, rnd)
    assert not ref[others].any() and not rnd[others].any(), (ref, rnd)
    return int(ref[which]), int(rnd[which])


def _against_host(probs, iters, which, pol="Full", host_flags=None, **dev_flags):
    """The comparison of the module docstring from lambda = 1: the log and the points after ``iters``
    iterations, and bit for bit after one iteration on fresh batches.  Returns (device batch -- still
    open, host batch -- still open, rounds of instance ``which``, live)."""
    par = Params(newton_type=pol, lamb_init=1.0, lamb_red=0.9)
    host_flags = host_flags or {}
    for n_it in (1, iters):
        host_b = make_batch(probs, pol, **host_flags)
        host, rec, live = _host_run(host_b, par, n_it)
        bd, dev = _dev(probs, par, n_it, pol, **dev_flags)
        assert host_b.repaired() >= 1
        piv, grd = bd.ctl_stats()
        assert not piv.any() and not grd.any(), (piv, grd)
        _, rounds = _refined(bd, which, len(probs))
        # accepted at lambda = 1 in iteration 0
        assert dev.history[0, which, 0] == 1.0 and dev.history[0, which, 2] != 0.0, dev.history[0, which]
        _same_log(dev.history, rec)
        if n_it == 1:
            for a, b in zip(bd.points(), host_b.points()):
                assert np.array_equal(a, b)
            bd.close()
            host_b.close()
    _same_points(bd, dev, host_b, host)
    return bd, host_b, rounds, live


# ------------------------------------------------------------------ 1: the narrow route
def test_a_miss_of_the_guard_is_refined_inside_the_loop(pgf):
    probs = _unstable()
    _premise(probs[1], 8)
    bd, host_b, _, _ = _against_host(probs, 3, 1)
    bd.close()
    host_b.close()


# ------------------------------------------------------------------ 2: the wide route, block 16
def _wide_unstable(split=None):
    """test_band_batch_wide_gpu.py's unstable pivot: n = 300, bw 12, block 16, K[v, v] = 1e-10."""
    n, block, eps = 300, 16, 1e-10
    rng = np.random.default_rng(7)
    ds = [2.5 + rng.uniform(0.0, 0.5, n) for _ in range(3)]
    v = head_of_first_eliminated(wide_band_problem(n, ds[1], 1, block), block)
    ds[1][v] = -1.0 + eps
    return [forced(band_problem(n, ds[i], 1 + i, 12), block, split) for i in range(3)]


def test_wide_route_refines_against_the_kept_factors(pgf):
    iters = 3
    probs = _wide_unstable()
    assert plan_of(probs[1]).bw == 12
    _premise(probs[1], 16)
    bd, host_b, rounds, live = _against_host(probs, iters, 1, host_flags=dict(wide_band=True), wide_band=True)
    host_b.close()
    steps = iters + live.sum(axis=0)
    red, sol, _ = bd.band_wide_stats()
    bd.close()
    # split on: one reduction per iteration (lambda changed; no bounds, so the mask never does and a
    # second step solves against the kept factors), and the rounds are solve phases
    extra = np.array([0, rounds, 0])
    assert list(red) == [iters] * 3 and np.array_equal(sol, live.sum(axis=0) + extra), (red, sol, live, rounds)
    # split off: the rounds reduce again; the same history
    par = Params(newton_type="Full", lamb_init=1.0, lamb_red=0.9)
    on, dev_on = _dev(probs, par, iters, wide_band=True)
    off, dev_off = _dev(_wide_unstable(split=False), par, iters, wide_band=True)
    red, sol, _ = off.band_wide_stats()
    assert np.array_equal(red, steps + extra) and not sol.any(), (red, sol)
    assert np.array_equal(dev_off.history, dev_on.history)
    on.close()
    off.close()


# ------------------------------------------------------------------ 3, 4: bordered, narrow and wide
@pytest.mark.parametrize("block", [8, 16, 64])
def test_bordered_routes_refine_against_y_and_the_factor_of_s(pgf, block):
    iters = 2
    prob, v = guard_case(1, block, 1e-9)
    _premise_bordered(prob, v, block)
    others = [bordered_lq(300, 8, 0, 0, 1, 186 + 100 * i, block=None if block == 8 else block, bound=1e6)
              for i in range(2)]
    probs = [others[0], prob, others[1]]
    assert len({plan_of(p).pattern_hash() for p in probs}) == 1
    route = dict(border=True) if block == 8 else dict(wide_border=True)
    bd, host_b, rounds, live = _against_host(probs, iters, 1, host_flags=route, border_ctl=True, **route)
    assert bd.band_block == block and bd.band_border == 1
    # the factor phases are those of the host-driven twin, whose repair ran on the handle; the
    # rounds are solve phases of the batch
    (fac, sol), (hfac, hsol) = bd.border_stats(), host_b.border_stats()
    assert np.array_equal(fac, hfac) and np.array_equal(sol, hsol + np.array([0, rounds, 0])), (fac, hfac, sol, hsol)
    if block > 8:
        assert all(np.array_equal(a, b) for a, b in zip(phases(bd), (fac, sol)))
    bd.close()
    host_b.close()


# ------------------------------------------------------------------ 5: a miss refinement does not cure
def test_a_miss_that_refinement_does_not_cure_stays_a_rejected_step(pgf):
    from pygradflow_amd import _lib

    lib, iters = _lib.load(), 3
    probs = _unstable()
    handle = []

    def strict(bd):  # (refine_fail far below what a round reaches)
        handle.append(bd.solvers[1]._hd.h)
        _lib.check(lib.pgf_set_refinement(handle[0], 1, 1e-11, 1e-30))

    try:
        bd, dev = _dev(probs, SLOW_RED, iters, before_init=strict)
        assert list(dev.history[0, 1]) == [1.0, 2.0, 0.0]
        piv, grd = bd.ctl_stats()
        ref, rnd = bd.ctl_refine_stats()
        assert list(grd) == [0, 1, 0] and not piv.any() and list(ref) == [0, 1, 0], (piv, grd, ref, rnd)
        plain, dev2 = _dev(probs, SLOW_RED, iters, ctl_refine=False)
        assert np.array_equal(dev.history[:, [0, 2]], dev2.history[:, [0, 2]])
        for a, b in zip(bd.points(), plain.points()):
            assert np.array_equal(a[[0, 2]], b[[0, 2]])
        plain.close()
        bd.close()
    finally:  # (handles are pooled)
        if handle:
            _lib.check(lib.pgf_set_refinement(handle[0], 1, 1e-11, 1e-7))


# ------------------------------------------------------------------ 6: refinement off on the handle
def test_no_refinement_when_the_handle_has_refinement_off(pgf):
    from pygradflow_amd import _lib

    lib = _lib.load()
    handle = []

    def off(bd):
        handle.append(bd.solvers[1]._hd.h)
        _lib.check(lib.pgf_set_refinement(handle[0], 0, 0.0, 0.0))

    try:
        bd, dev = _dev(_unstable(), Params(newton_type="Full", lamb_init=1.0), 2, before_init=off)
        piv, grd = bd.ctl_stats()
        ref, rnd = bd.ctl_refine_stats()
        assert not piv.any() and not grd.any() and not ref.any() and not rnd.any(), (piv, grd, ref, rnd)
        bd.close()
    finally:
        if handle:
            _lib.check(lib.pgf_set_refinement(handle[0], 1, 0.0, 0.0))


# ------------------------------------------------------------------ 7: singular beside refining
def test_a_singular_instance_is_never_refined(pgf):
    probs = _unstable()
    n, v = probs[0].num_vars, 150
    bad = forced(decoupled(probs[0], v))
    assert not (bad.hess_sparse().toarray() + np.eye(n))[v].any()
    bd, dev = _dev([bad, probs[1], probs[2]], SLOW_RED, 3)
    assert list(dev.history[0, 0]) == [1.0, 2.0, 0.0]
    assert dev.history[0, 1, 0] == 1.0 and dev.history[0, 1, 2] != 0.0
    piv, grd = bd.ctl_stats()
    assert list(piv) == [1, 0, 0] and not grd.any()
    _refined(bd, 1, 3)
    bd.close()


# ------------------------------------------------------------------ 8: Simplified
def test_simplified_with_a_refined_instance(pgf):
    iters = 3
    bd, host_b, _, _ = _against_host(_unstable(), iters, 1, pol="Simplified")
    # (two steps enqueued per iteration, the second without the assembly)
    assert tuple(bd.band_stats()[:2]) == (2 * iters, iters)
    bd.close()
    host_b.close()


# ------------------------------------------------------------------ 9: the inert pass, batch sizes
def test_seventy_instances_the_unstable_one_last(pgf):
    n, bw, count, iters = 300, 5, 70, 2
    rng = np.random.default_rng(11)
    ds = [2.5 + rng.uniform(0.0, 0.5, n) for _ in range(count)]
    v = head_of_first_eliminated(forced(band_problem(n, ds[-1], count, bw)), 8)
    ds[-1][v] = -1.0 + 1e-11
    probs = [forced(band_problem(n, ds[i], 1 + i, bw)) for i in range(count)]
    _premise(probs[-1], 8)
    bd, dev = _dev(probs, SLOW_RED, iters)
    plain, dev2 = _dev(probs, SLOW_RED, iters, ctl_refine=False)
    assert np.array_equal(dev.history[:, :-1], dev2.history[:, :-1])
    for a, b in zip(bd.points(), plain.points()):
        assert np.array_equal(a[:-1], b[:-1])
    assert dev.history[0, -1, 0] == 1.0 and dev.history[0, -1, 2] != 0.0 and dev2.history[0, -1, 2] == 0.0
    _refined(bd, count - 1, count)
    assert not bd.ctl_stats()[1].any() and plain.ctl_stats()[1][-1] >= 1
    bd.close()
    plain.close()


def test_batch_of_one(pgf):
    bd, dev = _dev([_unstable()[1]], SLOW_RED, 2)
    assert dev.history[0, 0, 0] == 1.0 and dev.history[0, 0, 2] != 0.0
    _refined(bd, 0, 1)
    assert not bd.ctl_stats()[1].any()
    bd.close()
