"""The device-resident step controller on band batches (PGF_BATCH_BAND_CTL; kbb_step_final in
csrc/pgf_sparse.hip, the loop in csrc/pgf_api_batch_ctl.hip): k outer iterations of every instance
enqueued back to back, the banded step finished per instance on the device.

The reference is the host-driven ``BatchedDistanceRatioController`` on a twin batch without the flag,
which test_step_control.py pins to the reference's controller.  Both run the same kernels in the same
order, and kbb_step_final sums the step length in the host's order, so the only difference is device
``log`` / ``exp`` against libm in the PI law.  The bars are those of the dense test
(test_step_control.py::test_device_resident_controller_matches_host_controller): accept flags equal,
lambda used and lambda next within rtol 1e-12, points within 1e-10 after one more
``advance_outer_each`` has put rejected instances back.  The comparison with the host twin means
something only when no guard fired on either side, so it asserts ``ctl_stats()`` all zero and
``repaired() == 0``.  Shapes are the smallest that reach each branch.
"""

import ctypes as C

import numpy as np
import pytest

from tests import golden_util as G
from tests.band_batch_util import make_batch
from tests.band_util import band_problem, decoupled, forced, head_of_first_eliminated, multistate_ocp, plan_of
from tests.oracle_step_solver import OracleStepSolver

from pygradflow_amd import step_control as SC
from pygradflow_amd.iterate import Iterate
from pygradflow_amd.params import Params

pytestmark = pytest.mark.gpu

_batch = make_batch


def _host_run(host_b, par, iters, lamb=None):
    """``iters`` iterations of the host-driven controller; returns (controller, record, live) with
    record[it] = (lambda used, lambda next, accepted) and live[it][i]: instance i took step two."""
    host = SC.BatchedDistanceRatioController(host_b, par, rho=1.0)
    if lamb is not None:
        host.lamb = np.array(lamb, dtype=np.float64)
    frozen, set_frozen = [], host_b.set_frozen

    def spy(done=None):
        frozen.append(np.array(done, dtype=bool))
        return set_frozen(done)

    host_b.set_frozen = spy
    rec, live = [], []
    for _ in range(iters):
        k = len(frozen)
        rec.append(host.step())
        # (no call: every instance was done after step one, and no second step was taken)
        live.append(~frozen[k] if len(frozen) > k else np.zeros(host_b.count, dtype=bool))
    host_b.set_frozen = set_frozen
    return host, rec, np.array(live)


def _same_log(history, rec, rows=None, cols=slice(None), shift=0):
    for it, (used, nxt, acc) in enumerate(rec[:rows]):
        h = history[it + shift][cols]
        assert np.array_equal(h[:, 2] != 0.0, acc[cols]), (it, h[:, 2], acc)
        assert np.allclose(h[:, 0], used[cols], rtol=1e-12, atol=0), (it, h[:, 0], used)
        assert np.allclose(h[:, 1], nxt[cols], rtol=1e-12, atol=0), (it, h[:, 1], nxt)


def _same_points(dev_b, dev, host_b, host, cols=slice(None)):
    """One more outer step puts rejected instances back on both sides; then the points."""
    host_b.advance_outer_each(1.0 / host.lamb, host.rho, host.accepted)
    dev_b.advance_outer_each(1.0 / dev.lamb, np.ones(dev_b.count), dev.accepted)
    (xh, yh), (xd, yd) = host_b.points(), dev_b.points()
    assert G.rel_err(xd[cols], xh[cols]) <= 1e-10 and G.rel_err(yd[cols], yh[cols]) <= 1e-10


def _no_guard_fired(dev_b, host_b):
    piv, grd = dev_b.ctl_stats()
    assert not piv.any() and not grd.any() and host_b.repaired() == 0, (piv, grd, host_b.repaired())


def _against_host(probs, pol, lamb_init, iters, wide=False):
    """The comparison of the module docstring; returns (device history, host record, live, device
    batch -- still open, for the counters of the caller)."""
    par = Params(newton_type=pol, lamb_init=lamb_init)
    host_b, dev_b = _batch(probs, pol, wide_band=wide), _batch(probs, pol, wide_band=wide, band_ctl=True)
    assert dev_b.band and host_b.band
    host, rec, live = _host_run(host_b, par, iters)
    dev = SC.DeviceResidentDistanceRatioController(dev_b, par, rho=1.0, max_iterations=iters)
    dev.run(iters)  # one ctl_iterate, one host synchronisation
    _same_log(dev.history, rec)
    assert np.allclose(dev.lamb, host.lamb, rtol=1e-12, atol=0)
    _no_guard_fired(dev_b, host_b)
    _same_points(dev_b, dev, host_b, host)
    host_b.close()
    return dev.history, rec, live, dev_b


def _cpu_kinds(prob, pol, lamb_init, iters):
    """The reference's controller over the CPU oracle, one instance: per iteration "rej", "conv"
    (accepted after step one with lambda * lamb_red: the converged early exit) or "acc"."""
    par = Params(newton_type=pol, step_solver=OracleStepSolver, lamb_init=lamb_init)
    ctl = SC.DistanceRatioController(prob, par)
    recs = SC.gradient_flow(ctl, lambda x, y: Iterate(prob, par, x, y), np.zeros(prob.num_vars),
                            np.zeros(prob.num_cons), 1.0, iters)
    return ["rej" if not r["accepted"] else
            "conv" if r["lamb_next"] == max(r["lamb"] * par.lamb_red, par.lamb_min) else "acc" for r in recs]


# ------------------------------------------------------------------ 1: narrow route
def _narrow(kind, i):
    from pygradflow_amd import problems

    return forced(problems.box_qp(264, seed=i) if kind == "box" else problems.sparse_ocp(30, seed=i))


# (problem, lamb_init, what the CPU controller shows somewhere in the case).  box_qp(264) from
# lambda = 1: the first step overshoots its bounds and is rejected; from lambda = 16 the first two
# iterations converge after one Newton step; sparse_ocp(30) (constrained, N = 90) converges after one
# step in every iteration.
NARROW = [("box", 1.0, "rej"), ("box", 16.0, "conv"), ("ocp", 1.0, "conv")]


@pytest.mark.parametrize("pol", ["Full", "Simplified", "ActiveSet"])
@pytest.mark.parametrize("kind,lamb_init,want", NARROW)
def test_narrow_route_against_the_host_driven_controller(pgf, kind, lamb_init, want, pol):
    iters = 6
    probs = [_narrow(kind, i) for i in range(4)]
    assert plan_of(probs[0]).block_size == 8
    cpu = [_cpu_kinds(p, pol, lamb_init, iters) for p in probs]
    assert any(want in k for k in cpu), cpu
    hist, rec, live, dev_b = _against_host(probs, pol, lamb_init, iters)
    dev_b.close()
    # the host record on the device shows what the case was chosen for: a rejection, or the
    # converged early exit (accepted with lambda * lamb_red, no second step)
    par = Params()
    if want == "rej":
        assert any(not r[2].all() for r in rec)
    else:
        assert any(r[2][i] and not live[it][i] and r[1][i] == max(r[0][i] * par.lamb_red, par.lamb_min)
                   for it, r in enumerate(rec) for i in range(4))


# ------------------------------------------------------------------ 2: wide route
# T = 5: N = 50, 100, 200, four blocks of 16, 32, 64 rows (a left and a right neighbour missing at
# level one, one level with a single kept block: the edges of test_band_split_gpu.py's (5, 4, 2)).
# lamb_init: one at which the CPU controller keeps lambda above 0.2 over four iterations.
WIDE = [((5, 4, 2), 16, 4.0), ((5, 8, 4), 32, 1.0), ((5, 16, 8), 64, 1.0)]


@pytest.mark.parametrize("pol", ["Full", "Simplified"])
@pytest.mark.parametrize("args,block,lamb_init", WIDE)
def test_wide_route_against_the_host_driven_controller(pgf, args, block, lamb_init, pol):
    iters = 4
    probs = [multistate_ocp(*args, i) for i in range(3)]
    assert plan_of(probs[0]).block_size == block
    hist, rec, live, dev_b = _against_host(probs, pol, lamb_init, iters, wide=True)
    assert dev_b.band_block == block
    red, sol, lean = dev_b.band_wide_stats()
    dev_b.close()
    if pol == "Full":
        return
    # Simplified, split on: step one of an iteration reduces (lambda changed), step two is a solve
    # phase for the instances still live, enqueued without assembly and inversion launches
    assert list(red) == [iters] * 3 and lean == iters, (red, lean)
    assert np.array_equal(sol, live.sum(axis=0)), (sol, live)
    assert live.any()
    # split off: the second steps reduce again, nothing is lean, the trajectory is the same
    off = [multistate_ocp(*args, i, split=False) for i in range(3)]
    off_b = _batch(off, pol, wide_band=True, band_ctl=True)
    dev = SC.DeviceResidentDistanceRatioController(off_b, Params(newton_type=pol, lamb_init=lamb_init),
                                                   rho=1.0, max_iterations=iters)
    dev.run(iters)
    red, sol, lean = off_b.band_wide_stats()
    assert np.array_equal(red, iters + live.sum(axis=0)) and not sol.any() and lean == 0, (red, sol, lean)
    assert np.array_equal(dev.history, hist)
    off_b.close()


# ------------------------------------------------------------------ 3: a singular instance
def _ctl_run(probs, par, iters):
    bd = _batch(probs, "Full", band_ctl=True)
    dev = SC.DeviceResidentDistanceRatioController(bd, par, rho=1.0, max_iterations=iters)
    dev.run(iters)
    return bd, dev


# The problems of tests 3 and 4 have no bounds, so a Full step solves the outer step exactly and every
# iteration that is not rejected takes the converged early exit, lambda <- lamb_red lambda.  With the
# default lamb_red = 0.5 an instance rejected at lambda = 1 would come back to lambda = 1 from
# 2 lambda, and be rejected there again, every other iteration; 0.9 keeps it away (2, 1.8, 1.62, ...).
SLOW_RED = Params(newton_type="Full", lamb_init=1.0, lamb_red=0.9)


def test_one_singular_instance_is_rejected_and_goes_on(pgf):
    n, v, iters = 600, 333, 3
    goods = [forced(band_problem(n, 2.5 + np.random.default_rng(9 + i).uniform(0.0, 0.5, n), 3 + i, 5))
             for i in range(3)]
    bad = forced(decoupled(goods[1], v))
    assert not (bad.hess_sparse().toarray() + np.eye(n))[v].any()
    bd, dev = _ctl_run([goods[0], bad, goods[2]], SLOW_RED, iters)
    two, dev2 = _ctl_run([goods[0], goods[2]], SLOW_RED, iters)
    assert list(dev.history[0, 1]) == [1.0, 2.0, 0.0]
    piv, grd = bd.ctl_stats()
    assert list(piv) == [0, 1, 0] and not grd.any()
    # from iteration 1 on it runs with lambda = 2, K[v, v] = 1: no further failure, and it moves
    assert dev.history[1, 1, 0] == 2.0 and dev.history[1:, 1, 2].all()
    bd.advance_outer_each(1.0 / dev.lamb, np.ones(3), dev.accepted)
    two.advance_outer_each(1.0 / dev2.lamb, np.ones(2), dev2.accepted)
    (x, _), (x2, _) = bd.points(), two.points()
    assert x[1].any()
    # the others: bit for bit the batch of two
    assert np.array_equal(dev.history[:, [0, 2]], dev2.history)
    assert np.array_equal(x[[0, 2]], x2)
    bd.close()
    two.close()


# ------------------------------------------------------------------ 4: a miss of the guard
def _unstable(eps=1e-11):
    """test_band_batch_gpu.py::test_an_unstable_pivot_in_one_instance_is_repaired_on_its_handle:
    n = 300, bw 5, K[v, v] = eps at lambda = 1 at the head of block 1, which level one inverts as it
    stands.  That test shows on the CPU that the plain solve in the reduction's order misses
    refine_tol = 1e-11 (2.5e-9)."""
    n, bw = 300, 5
    rng = np.random.default_rng(7)
    ds = [2.5 + rng.uniform(0.0, 0.5, n) for _ in range(3)]
    v = head_of_first_eliminated(forced(band_problem(n, ds[1], 1, bw)), 8)
    ds[1][v] = -1.0 + eps
    return [forced(band_problem(n, ds[i], 1 + i, bw)) for i in range(3)]


def test_a_miss_of_the_guard_is_a_rejected_step(pgf):
    iters = 3
    probs = _unstable()
    par = SLOW_RED
    bd, dev = _ctl_run(probs, par, iters + 1)
    piv, grd = bd.ctl_stats()
    print(f"log of instance 1: {dev.history[:, 1]}, guard rejects {grd}")
    assert list(dev.history[0, 1]) == [1.0, 2.0, 0.0]
    assert grd[1] >= 1 and grd[0] == 0 and grd[2] == 0 and not piv.any()
    # the host-driven twin, instance 1 starting at lambda = 2 (K[v, v] = 1 + eps: nothing to repair)
    host_b = _batch(probs, "Full")
    host, rec, _ = _host_run(host_b, par, iters, lamb=[1.0, 2.0, 1.0])
    assert host_b.repaired() == 0
    _same_log(dev.history, rec, cols=[1], shift=1)
    _same_log(dev.history, rec, cols=[0, 2])
    assert grd[1] == 1  # (so rows 1.. of instance 1 are undisturbed)
    _same_points(bd, dev, host_b, host, cols=[1])
    bd.close()
    host_b.close()


def test_no_guard_reject_when_the_handle_has_refinement_off(pgf):
    from pygradflow_amd import _lib

    probs = _unstable()
    bd = _batch(probs, "Full", band_ctl=True)
    lib, h = _lib.load(), bd.solvers[1]._hd.h
    _lib.check(lib.pgf_set_refinement(h, 0, 0.0, 0.0))  # (tolerances as they are)
    try:
        dev = SC.DeviceResidentDistanceRatioController(bd, Params(newton_type="Full", lamb_init=1.0), rho=1.0,
                                                       max_iterations=2)
        dev.run(2)
        piv, grd = bd.ctl_stats()
        assert not grd.any() and not piv.any(), (piv, grd)
    finally:  # (handles are pooled: the next owner finds the guard as a new handle has it)
        _lib.check(lib.pgf_set_refinement(h, 1, 0.0, 0.0))
        bd.close()


# ------------------------------------------------------------------ 5: B edge cases
def test_batch_of_one(pgf):
    from pygradflow_amd import problems

    _against_host([forced(problems.box_qp(264, seed=5))], "Full", 1.0, 3)[3].close()


def test_seventy_tiny_instances(pgf):
    """Eighteen workgroups of kbb_step_final, the last with two instances; N = 40."""
    from pygradflow_amd import problems

    probs = [forced(problems.box_qp(40, seed=i, bound={3: 0.0, 5: np.inf}.get(i, 0.5))) for i in range(70)]
    _against_host(probs, "Full", 1.0, 3)[3].close()


# ------------------------------------------------------------------ 6: order of calls, mixing
def test_order_of_calls_and_mixing_with_host_driven_steps(pgf):
    from pygradflow_amd import _lib, problems

    lib = _lib.load()
    probs = [forced(problems.box_qp(264, seed=i)) for i in range(3)]
    par = Params(newton_type="Full", lamb_init=100.0)  # (a short step: converged after step one)
    nan = float("nan")
    dev_b, host_b = _batch(probs, "Full", band_ctl=True), _batch(probs, "Full")
    assert lib.pgf_batch_ctl_iterate(dev_b._b, 3, nan, 1) == _lib.PGF_NOT_READY
    assert lib.pgf_batch_ctl_read(dev_b._b, None, None, None, 0) == _lib.PGF_NOT_READY
    dev = SC.DeviceResidentDistanceRatioController(dev_b, par, rho=1.0, max_iterations=2)
    _lib.check(lib.pgf_batch_step_async(dev_b._b, 3, nan), batch=dev_b._b)
    assert lib.pgf_batch_ctl_iterate(dev_b._b, 3, nan, 1) == _lib.PGF_NOT_READY  # a step is pending
    _lib.check(lib.pgf_batch_sync(dev_b._b, None, None, None), batch=dev_b._b)
    host_b.step_local()
    assert lib.pgf_batch_ctl_iterate(dev_b._b, 3, nan, 3) == _lib.PGF_INVALID  # beyond the log
    host, rec, live = _host_run(host_b, par, 1)
    dev.run(1)
    _same_log(dev.history, rec)
    frozen = ~live[0]  # decided after step one: the controller froze them for step two
    assert frozen.any() and rec[0][2][frozen].all()
    # a host-driven step right behind ctl_read: the device still has them frozen, and the host
    # knows (the twin is told: its controller freezes only in front of a second step)
    before = dev_b.points()
    st, _, df = dev_b.step_local()
    host_b.set_frozen(frozen)
    host_b.step_local()
    assert not st.any() and not df[frozen].any() and df[~frozen].all()
    assert all(np.array_equal(a[frozen], b[frozen]) for a, b in zip(before, dev_b.points()))
    # and from the next outer step on the batch is driven by the host like its twin
    for bd, lamb, acc in ((dev_b, dev.lamb, dev.accepted), (host_b, host.lamb, host.accepted)):
        bd.advance_outer_each(1.0 / lamb, np.ones(3), acc)
    (st, nn, df), (st2, nn2, df2) = dev_b.step_local(), host_b.step_local()
    assert not st.any() and not st2.any() and np.array_equal(nn, nn2) and df.all()
    assert np.allclose(df, df2, rtol=1e-10, atol=0)
    (x, y), (x2, y2) = dev_b.points(), host_b.points()
    assert G.rel_err(x, x2) <= 1e-10 and G.rel_err(y, y2) <= 1e-10
    # a band batch without the flag still refuses (test_band_batch_gpu.py has the full list)
    with pytest.raises(NotImplementedError, match="dense batch only"):
        host_b.ctl_init(par)
    assert lib.pgf_batch_ctl_iterate(host_b._b, 3, nan, 1) == _lib.PGF_INVALID
    piv = np.full(3, 5, dtype=np.int32)
    assert lib.pgf_batch_debug_ctl_stats(host_b._b, piv.ctypes.data_as(C.POINTER(C.c_int)), None) == 0
    assert not piv.any()
    dev_b.close()
    host_b.close()
