"""Bordered band batches under the device-resident step controller (PGF_BATCH_BORDER_CTL with
PGF_BATCH_BORDER | PGF_BATCH_BAND_CTL; on a wide remainder PGF_BATCH_WIDE_BAND | PGF_BATCH_WIDE_BORDER
besides): the loop of csrc/pgf_api_batch_ctl.hip around the bordered step of csrc/pgf_border.hip, finished
per instance by kbb_step_final.

The reference and the bars are those of test_band_batch_ctl_gpu.py, whose helpers are used: the
host-driven ``BatchedDistanceRatioController`` on a twin batch without the controller's flags --
accept flags equal, lambda used and lambda next within rtol 1e-12, points within 1e-10 -- and
``np.array_equal`` where both sides run the same device functions in the same order.  Shapes are
the smallest that reach each branch."""

import numpy as np
import pytest

from tests.band_batch_util import make_batch, phases
from tests.band_util import band_problem, bordered_lq, case, forced, plan_of, singular_schur
from tests.test_band_batch_ctl_gpu import _cpu_kinds, _host_run, _no_guard_fired, _same_log, _same_points

from pygradflow_amd import step_control as SC
from pygradflow_amd.params import Params

pytestmark = pytest.mark.gpu

CTL = dict(border=True, band_ctl=True, border_ctl=True)


def _flags(wide):
    return dict(wide_border=True) if wide else dict(border=True)


def _dev_run(probs, pol, lamb_init, iters, wide=False, par=None, **extra):
    par = par or Params(newton_type=pol, lamb_init=lamb_init)
    dev_b = make_batch(probs, pol, band_ctl=True, border_ctl=True, **_flags(wide), **extra)
    dev = SC.DeviceResidentDistanceRatioController(dev_b, par, rho=1.0, max_iterations=iters)
    dev.run(iters)
    return dev_b, dev


def _against_host(probs, pol, lamb_init, iters, wide=False):
    """(device history, host record, live, device batch -- still open)."""
    par = Params(newton_type=pol, lamb_init=lamb_init)
    host_b = make_batch(probs, pol, **_flags(wide))
    assert host_b.band and host_b.band_border == plan_of(probs[0]).k
    host, rec, live = _host_run(host_b, par, iters)
    dev_b, dev = _dev_run(probs, pol, lamb_init, iters, wide)
    assert dev_b.band and dev_b.band_border == host_b.band_border
    _same_log(dev.history, rec)
    assert np.allclose(dev.lamb, host.lamb, rtol=1e-12, atol=0)
    _no_guard_fired(dev_b, host_b)
    _same_points(dev_b, dev, host_b, host)
    host_b.close()
    return dev.history, rec, live, dev_b


# ------------------------------------------------------------------ 1: narrow route
# bordered_lq(100, 2, 10, 1, 1): k = 2, Nb = 110, block 8.  On the CPU, from lambda = 1 the first
# iteration of instances 0 and 1 is rejected under every policy; from lambda = 16 iteration 0 of every
# instance takes the converged early exit.
@pytest.mark.parametrize("pol", ["Full", "Simplified", "ActiveSet"])
@pytest.mark.parametrize("lamb_init,want", [(1.0, "rej"), (16.0, "conv")])
def test_narrow_route_against_the_host_driven_controller(pgf, lamb_init, want, pol):
    iters = 6
    probs = [bordered_lq(100, 2, 10, 1, 1, seed=i) for i in range(3)]
    plan = plan_of(probs[0])
    assert plan.block_size == 8 and plan.k == 2 and plan.Nb == 110
    cpu = [_cpu_kinds(p, pol, lamb_init, iters) for p in probs]
    assert any(want in k for k in cpu), cpu
    hist, rec, live, dev_b = _against_host(probs, pol, lamb_init, iters)
    dev_b.close()
    par = Params()
    if want == "rej":
        assert any(not r[2].all() for r in rec)
    else:
        assert any(r[2][i] and not live[it][i] and r[1][i] == max(r[0][i] * par.lamb_red, par.lamb_min)
                   for it, r in enumerate(rec) for i in range(3))


# ------------------------------------------------------------------ 2: wide route
# Five blocks of B (a right neighbour missing at level one, a level with a single kept block):
# Nb = 70, 140, 280 band rows at block 16, 32, 64, k = 2, 2, 3.  lamb_init = 4: the CPU controller
# accepts every iteration.
WIDE = [((2, 70), 16), ((2, 140), 32), ((3, 280), 64)]


@pytest.mark.parametrize("pol", ["Full", "Simplified"])
@pytest.mark.parametrize("args,block", WIDE)
def test_wide_route_against_the_host_driven_controller(pgf, args, block, pol):
    iters, lamb_init = 4, 4.0
    probs = [case(*args, block=block, seed=i) for i in range(3)]
    plan = plan_of(probs[0])
    assert plan.block_size == block and plan.k == args[0] and plan.Nb == args[1]
    assert -(-plan.Nb // block) == 5
    hist, rec, live, dev_b = _against_host(probs, pol, lamb_init, iters, wide=True)
    assert dev_b.band_block == block
    fac, sol = dev_b.border_stats()
    wide_fac, wide_sol = phases(dev_b)
    lean = dev_b.band_wide_stats()[2]
    dev_b.close()
    if pol == "Full":
        return
    # Simplified: step one of an iteration runs the factor phase (lambda changed), step two is a
    # solve phase for the instances still live, enqueued without factor-phase launches
    assert list(fac) == [iters] * 3 and lean == iters, (fac, lean)
    assert np.array_equal(sol, iters + live.sum(axis=0)), (sol, live)
    assert np.array_equal(wide_fac, fac) and np.array_equal(wide_sol, sol)
    assert live.any()


# ------------------------------------------------------------------ 3: a singular Schur complement
def test_a_singular_schur_complement_in_one_instance(pgf):
    """singular_schur: S has a zero pivot at lambda = 1 (the flag reaches the status block through
    kbd_border_small_solve); from lambda = 2 the instance moves."""
    iters = 3
    goods = [case(6, 203, seed=6203 + i) for i in range(3)]
    bad, v = singular_schur(goods[1])
    assert plan_of(bad).k == 6 and plan_of(bad).block_size == 8
    par = Params(newton_type="Full", lamb_init=1.0, lamb_red=0.9)
    bd, dev = _dev_run([goods[0], bad, goods[2]], "Full", 1.0, iters, par=par)
    two, dev2 = _dev_run([goods[0], goods[2]], "Full", 1.0, iters, par=par)
    assert list(dev.history[0, 1]) == [1.0, 2.0, 0.0]
    piv, grd = bd.ctl_stats()
    assert list(piv) == [0, 1, 0] and not grd.any()
    assert dev.history[1, 1, 0] == 2.0 and dev.history[1:, 1, 2].all()
    bd.advance_outer_each(1.0 / dev.lamb, np.ones(3), dev.accepted)
    two.advance_outer_each(1.0 / dev2.lamb, np.ones(2), dev2.accepted)
    (x, y), (x2, y2) = bd.points(), two.points()
    assert x[1].any()
    assert np.array_equal(dev.history[:, [0, 2]], dev2.history)
    assert np.array_equal(x[[0, 2]], x2) and np.array_equal(y[[0, 2]], y2)
    bd.close()
    two.close()


# ------------------------------------------------------------------ 4: refusals, inert cases
def test_refusals_and_inert_cases(pgf):
    import ctypes as C

    from pygradflow_amd import _lib, problems

    lib = _lib.load()
    out = C.c_void_p()
    text = "does not drive a bordered band batch"
    narrow = [bordered_lq(100, 2, 10, 1, 1, seed=i) for i in range(2)]
    # The bit without its companions, on handles that 16 | 4 | 2 would admit: PGF_INVALID, and no
    # handle was read -- a refusal of band_batch_create would have left its reason on handle 0.
    seq = make_batch(narrow, "Full", sequential=True)
    hs = (C.c_void_p * 2)(*[s._hd.h for s in seq.solvers])
    before = lib.pgf_last_error(hs[0])
    for flags in (16, 16 | 4, 16 | 2, 16 | 8 | 1, 32, 32 | 4, 32 | 4 | 1):
        assert lib.pgf_batch_create_ex(hs, 2, flags, C.byref(out)) == _lib.PGF_INVALID, flags
        assert lib.pgf_last_error(hs[0]) == before and not out.value, flags
    seq.close()
    with pytest.raises(ValueError, match=text):
        make_batch(narrow, "Full", border=True, band_ctl=True)
    wide = [case(2, 70, block=16, seed=i) for i in range(2)]
    with pytest.raises(ValueError, match=text):
        make_batch(wide, "Full", wide_border=True, band_ctl=True)
    # handles without a border: the bit changes nothing
    probs = [forced(problems.box_qp(264, seed=i)) for i in range(3)]
    par = Params(newton_type="Full", lamb_init=1.0)
    hist = []
    for extra in (dict(band_ctl=True), CTL):
        bd = make_batch(probs, "Full", **extra)
        assert bd.band and bd.band_border == 0
        dev = SC.DeviceResidentDistanceRatioController(bd, par, rho=1.0, max_iterations=3)
        dev.run(3)
        hist.append((np.array(dev.history), bd.points()))
        bd.close()
    assert np.array_equal(hist[0][0], hist[1][0])
    assert all(np.array_equal(a, b) for a, b in zip(hist[0][1], hist[1][1]))


# ------------------------------------------------------------------ 5: batch sizes
def test_batch_of_one(pgf):
    _against_host([bordered_lq(100, 2, 10, 1, 1, seed=5)], "Full", 1.0, 3)[3].close()


def test_seventy_tiny_instances(pgf):
    """Eighteen workgroups of kbb_step_final, the last with two instances."""
    probs = [bordered_lq(60, 2, 8, 1, 1, seed=i) for i in range(70)]
    assert plan_of(probs[0]).k == 2 and plan_of(probs[0]).block_size == 8
    _against_host(probs, "Full", 4.0, 3)[3].close()
