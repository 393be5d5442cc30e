"""Bordered instances in the banded device batch (csrc/pgf_border.hip, PGF_BATCH_BORDER): a
band of block size 8 plus 1 <= k <= 64 border nodes per instance, one launch sequence per Newton
step, factor phase per instance only where its matrix changed.

Two references, with the bars of band_batch_util.py: ``sequential=True``, which drives the same
instances one by one through their own handles (both routes run the same device functions of
pgf_border_dev.h and pgf_band_dev.h in the same order), and the CPU oracle.

Shapes, each checked on the host with ``plan_of`` (block size 8, plan supported) before it was put
here, as (k, Nb, bw, block):

  border widths   bordered_lq(200, 3, 65, kv, kc): (1 | 15 | 16 | 17 | 33 | 64, 265, 6, 8), each with
                  two thirds of the border variables (kv-heavy) and two thirds constraints (kc-heavy)
  row counts      bordered_lq(Nb - Nb // 4, 2, Nb // 4, 5, 12): (17, 1, 0, 8), (17, 7, 2, 8),
                  (17, 8, 3, 8), (17, 9, 3, 8), (17, 257, 3, 8), (17, 511, 5, 8), (17, 512, 6, 8),
                  (17, 513, 6, 8), (17, 1033, 6, 8): 1, 1, 1, 2, 33, 64, 64, 65, 130 blocks
  first / oracle  bordered_lq(100, 2, 10, 1, 1): (2, 110, 6, 8); bordered_lq(200, 2, 40, 2, 2):
                  (4, 240, 6, 8); budget_box_qp(1003) with the automatic border: (1, 1003, 1, 8)
  edges           bordered_lq(60, 2, 8, 1, 1): (2, 68, 3, 8)

bordered_lq(100, 3, 10, 1, 1) and bordered_lq(200, 3, 40, 2, 2) -- half-width 3 in H -- come out of
the plan's ordering with half-bandwidth 9, block size 16: the wide route, which a bordered batch
refuses.  They serve as the refusal's case below; the batches step their half-width 2 neighbours.
"""

import functools

import numpy as np
import pytest

from oracle import newton_oracle as O
from tests import golden_util as G
from tests.band_batch_util import against_oracle, churn_of, handle_stats, make_batch, same_as_sequential, same_step
from tests.band_util import (TOL, bordered_lq, case, forced, guard_case, mask_change_steps, plan_of,
                             singular_schur)

pytestmark = pytest.mark.gpu

POLICIES = ("Simplified", "Full", "ActiveSet")

_batch = functools.partial(make_batch, border=True)


def _narrow(probs, k=None):
    """The host-side check of the module docstring; every instance on one pattern."""
    plans = [plan_of(p) for p in probs]
    assert all(pl.supported and pl.block_size == 8 and pl.bw <= 8 for pl in plans)
    assert len({pl.pattern_hash() for pl in plans}) == 1
    if k is not None:
        assert plans[0].k == k
    return plans[0]


def _as_one_by_one(probs):
    """same_as_sequential with the border's width, block size and phase counters."""
    k = plan_of(probs[0]).k

    def opened(bd):
        assert bd.band_border == k and bd.band_block == 8

    def after(bd, pol, steps):
        fac, sol = bd.border_stats()
        assert np.all(sol == steps) and np.all(fac == (steps if pol == "Full" else 1)), (pol, fac, sol)

    same_as_sequential(_batch, probs, opened=opened, after=after)


# ------------------------------------------------------------------ 1: the batch exists
def test_bordered_instances_form_a_device_batch(pgf):
    probs = [bordered_lq(100, 2, 10, 1, 1, seed=i) for i in range(3)]
    _narrow(probs, k=2)
    bd = _batch(probs, "Full")
    assert bd.band and bd._b is not None and bd.band_border == 2 and bd.band_block == 8
    for _ in range(2):
        st, nn, _ = bd.step_local()
        assert not st.any() and np.all(nn == probs[0].num_cons)
    fac, sol = bd.border_stats()
    assert list(fac) == [2, 2, 2] and list(sol) == [2, 2, 2]
    assert bd.band_stats() == (2, 2)
    bd.close()


# ------------------------------------------------------------------ 2: border widths
@pytest.mark.parametrize("heavy", ["kv", "kc"])
@pytest.mark.parametrize("k", [1, 15, 16, 17, 33, 64])
def test_border_widths_as_one_by_one(pgf, k, heavy):
    """kp = 16 | 16 | 16 | 32 | 48 | 64: either side of every padding boundary, and MB_MAXQ = 8 panel
    columns per lane at k = 64."""
    big, small = k - k // 3, k // 3
    kv, kc = (big, small) if heavy == "kv" else (small, big)
    probs = [bordered_lq(200, 3, 65, kv, kc, seed=100 * k + i) for i in range(3)]
    plan = _narrow(probs, k=k)
    assert plan.Nb == 265 and plan.kp == (k + 15) // 16 * 16
    _as_one_by_one(probs)


# ------------------------------------------------------------------ 3: row counts
@pytest.mark.parametrize("Nb", [1, 7, 8, 9, 257, 511, 512, 513, 1033])
def test_row_counts_as_one_by_one(pgf, Nb):
    """One ragged block; block counts 1, 2, 33, 64 / 65, 130 -- the launch-plan branches of
    sp_bcr_plan that test_band_batch_gpu.py lists -- and SP_BORDER_CHUNK = 512 on either side."""
    mloc = Nb // 4
    probs = [bordered_lq(Nb - mloc, 2, mloc, 5, 12, seed=17000 + Nb + i) for i in range(3)]
    plan = _narrow(probs, k=17)
    assert plan.Nb == Nb
    _as_one_by_one(probs)


# ------------------------------------------------------------------ 4: against the oracle
def _oracle_run(probs):
    def check_recs(pol, recs):
        if pol != "Simplified":  # (which keeps its mask by definition)
            assert churn_of(recs) > 0, pol

    def opened(bd):
        assert bd.band_border

    return against_oracle(_batch, probs, tuple((p, 3) for p in POLICIES), check_recs=check_recs, opened=opened)


def test_against_the_oracle_bordered_lq(pgf):
    probs = [bordered_lq(200, 2, 40, 2, 2, seed=i) for i in range(3)]
    _narrow(probs, k=4)
    assert _oracle_run(probs) > 0


def test_against_the_oracle_budget_box_qp(pgf):
    from pygradflow_amd import problems

    probs = [problems.budget_box_qp(1003, seed=i) for i in range(3)]
    for p in probs:
        p.pgf_force_band = True
        p.pgf_border = "auto"
    assert _narrow(probs, k=1).Nb == 1003
    assert _oracle_run(probs) > 0


# ------------------------------------------------------------------ 5: phases per instance
def test_factor_phase_only_where_the_matrix_changed(pgf):
    """One pattern, three boxes: +-0.5 (the mask changes at every step), +-1 (at the second step
    only), +-3 (never active).  Under ActiveSet each instance factors where its own mask changed."""
    probs = [bordered_lq(200, 2, 40, 2, 2, seed=s, bound=b) for s, b in ((0, 0.5), (1, 1.0), (2, 3.0))]
    _narrow(probs, k=4)
    ch = [mask_change_steps(p, "ActiveSet", 4) for p in probs]
    assert ch == [[True, True, True], [True, False, False], [False, False, False]]
    bd, ref = _batch(probs, "ActiveSet"), _batch(probs, "ActiveSet", sequential=True)
    base = handle_stats(ref, ("border",))
    for k in range(4):
        same_step(bd, ref, k)
        fac, sol = bd.border_stats()
        hf, hs = handle_stats(ref, ("border",)) - base
        assert np.array_equal(fac, hf) and np.array_equal(sol, hs), (k, fac, hf, sol, hs)
    fac, sol = bd.border_stats()
    assert list(sol) == [4, 4, 4] and list(fac) == [4, 2, 1]
    assert bd.band_wide_stats()[2] == 0  # (the policy may change the mask: never lean)
    bd.close()
    ref.close()
    # Simplified: one factor phase, then two steps without a factor-phase launch
    bd, ref = _batch(probs, "Simplified"), _batch(probs, "Simplified", sequential=True)
    for k in range(3):
        same_step(bd, ref, ("Simplified", k))
    fac, sol = bd.border_stats()
    assert list(fac) == [1, 1, 1] and list(sol) == [3, 3, 3]
    assert bd.band_wide_stats()[2] == 2 and bd.band_stats() == (3, 1)
    bd.close()
    ref.close()


# ------------------------------------------------------------------ 6: per-instance outer steps
def test_per_instance_outer_steps_rejection_and_freezing(pgf):
    probs = [bordered_lq(200, 2, 40, 2, 2, seed=20 + i) for i in range(3)]
    _narrow(probs, k=4)
    dt = np.array([0.5, 1.0, 2.0])
    bd, ref = _batch(probs, "Full"), _batch(probs, "Full", sequential=True)
    for run in (bd, ref):
        run.step_local()
        run.advance_outer_each(dt, 1.0)
    outer = bd.points()
    for k in range(2):
        same_step(bd, ref, ("dt", k))
    # instance 1 is rejected: back to its outer point, bit for bit; the others go on
    moved, m0 = bd.points(), bd.masks()
    for run in (bd, ref):
        run.advance_outer_each(dt / 2, 1.0, accepted=[True, False, True])
    x, y = bd.points()
    assert np.array_equal(x[1], outer[0][1]) and np.array_equal(y[1], outer[1][1])
    assert np.array_equal(x[0], moved[0][0]) and np.array_equal(x[2], moved[0][2])
    assert not np.array_equal(x[1], moved[0][1])
    # instance 1 frozen: its point, its mask and both its counters stay
    fac0, sol0 = bd.border_stats()
    assert list(fac0) == [3, 3, 3] and list(sol0) == [3, 3, 3]
    bd.set_frozen([0, 1, 0])
    ref.set_frozen([0, 1, 0])
    for k in range(2):  # (the inertia reported for a frozen instance is the batch's alone)
        st, _, df = bd.step_local()
        ref.step_local()
        assert not st.any() and df[1] == 0.0
    x, y = bd.points()
    xr, yr = ref.points()
    assert np.array_equal(x, xr) and np.array_equal(y, yr)
    for i in (0, 2):  # (the frozen handle of the sequential loop has adopted no mask since its outer step)
        assert np.array_equal(bd.masks()[i], ref.solvers[i].mask()), i
    assert np.array_equal(x[1], outer[0][1]) and np.array_equal(y[1], outer[1][1])
    assert np.array_equal(bd.masks()[1], m0[1])
    fac, sol = bd.border_stats()
    assert list(fac - fac0) == [2, 0, 2] and list(sol - sol0) == [2, 0, 2]
    # the next outer step thaws it
    for run in (bd, ref):
        run.advance_outer_each(dt, 1.0)
    ref.set_frozen(None)  # (the sequential loop keeps its own list until told otherwise)
    same_step(bd, ref, "thawed")
    fac, sol = bd.border_stats()
    assert list(fac - fac0) == [3, 1, 3] and list(sol - sol0) == [3, 1, 3]
    bd.close()
    ref.close()


def test_measures_and_norms_as_one_by_one(pgf):
    probs = [bordered_lq(200, 2, 40, 2, 2, seed=30 + i) for i in range(3)]
    bd, ref = _batch(probs, "Full"), _batch(probs, "Full", sequential=True)

    def close(a, b):
        return np.all(np.abs(a - b) <= 1e-13 * np.abs(b))

    for k in range(2):
        assert close(bd.residual_norms_local(), ref.residual_norms_local()), k
        assert close(bd.measures(), ref.measures()), k
        same_step(bd, ref, k)
    assert close(bd.measures(), ref.measures()) and close(bd.residual_norms_local(), ref.residual_norms_local())
    assert bd.measures()[:, 3].max() > 0.0
    bd.close()
    ref.close()


# ------------------------------------------------------------------ 7: singular S in one instance
def test_a_singular_schur_complement_in_one_instance(pgf):
    from pygradflow_amd import _lib

    goods = [case(6, 203, seed=6203 + i) for i in range(3)]
    bad, v = singular_schur(goods[1])
    probs = [goods[0], bad, goods[2]]
    plan = _narrow(probs, k=6)
    assert plan.Nb == 203 and plan.pos[v] == 203 + 1  # a border node: B is as regular as ever
    n, m = bad.num_vars, bad.num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    mask = O.NewtonOracle(bad, "Full", x0, y0, 1.0, 1.0).solver.compute_active_set(O.PointData(bad, x0, y0))
    assert not mask[v]
    bd, ref = _batch(probs, "Full"), _batch(probs, "Full", sequential=True)
    st, nn, _ = bd.step_local()
    st2, nn2, _ = ref.step_local()
    assert list(st) == list(st2) == [0, _lib.PGF_SINGULAR, 0]
    (x, y), (x2, y2) = bd.points(), ref.points()
    assert not x[1].any() and not y[1].any()  # the point it started from
    for i in (0, 2):
        assert np.array_equal(x[i], x2[i]) and np.array_equal(y[i], y2[i]) and nn[i] == nn2[i] == m, i
        assert np.array_equal(bd.masks()[i], ref.solvers[i].mask()), i
    fac, sol = bd.border_stats()
    assert list(fac) == [1, 1, 1] and list(sol) == [1, 1, 1]
    # lambda = 2 makes S regular: the instance factors again (its bad factor is never solved
    # against a second time) and steps cleanly
    for run in (bd, ref):
        run.advance_outer_each(np.array([1.0, 0.5, 1.0]), 1.0, accepted=[True, False, True])
    st, nn = same_step(bd, ref, "regular")
    assert np.all(nn == m)
    x, _ = bd.points()
    assert x[1].any()
    fac, sol = bd.border_stats()
    assert list(fac) == [2, 2, 2] and list(sol) == [2, 2, 2]
    bd.close()
    ref.close()


def test_a_bad_factor_phase_is_repeated_before_the_next_solve(pgf):
    """Simplified keeps the mask, so only ctl[1] == 0 can make the singular instance factor again:
    it does, at every step, while the good ones factor once."""
    from pygradflow_amd import _lib

    goods = [case(6, 203, seed=6203 + i) for i in range(3)]
    bad, _ = singular_schur(goods[1])
    bd = _batch([goods[0], bad, goods[2]], "Simplified")
    for k in range(3):
        st, _, _ = bd.step_local()
        assert list(st) == [0, _lib.PGF_SINGULAR, 0], k
    fac, sol = bd.border_stats()
    assert list(fac) == [1, 3, 1] and list(sol) == [3, 3, 3]
    assert bd.band_wide_stats()[2] == 0  # (never lean while an instance is bad)
    bd.close()


# ------------------------------------------------------------------ 8: guard repair
def test_an_unstable_pivot_in_one_instance_is_repaired_on_its_handle(pgf):
    """band_util.guard_case(1, 8, 1e-9) as instance 1 of three: a 1e-9 pivot at the
    head of block 1 of B, an instability chosen on the CPU (K is regular, cond < 1e5)."""
    prob, v = guard_case(1, 8, 1e-9)
    others = [bordered_lq(300, 8, 0, 0, 1, 186 + 100 * i, bound=1e6) for i in range(2)]
    probs = [others[0], prob, others[1]]
    _narrow(probs, k=1)
    n, m = prob.num_vars, prob.num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    rec = O.NewtonOracle(prob, "Full", x0, y0, 1.0, 1.0).run(x0, y0, 1)[0]
    assert not rec["mask"].any()
    bd, ref = _batch(probs, "Full"), _batch(probs, "Full", sequential=True)
    before = bd.repaired()
    st, nn, _ = bd.step_local()
    ref.step_local()
    x, y = bd.points()
    xr, yr = ref.points()
    print(f"status {st}, repaired {bd.repaired() - before}, x error {G.rel_err(x[1], rec['xn']):.3e}, "
          f"y error {G.rel_err(y[1], rec['yn']):.3e}")
    assert not st.any()
    assert bd.repaired() == before + 1
    assert G.rel_err(x[1], rec["xn"]) <= TOL and G.rel_err(y[1], rec["yn"]) <= TOL
    for i in (0, 2):
        assert np.array_equal(x[i], xr[i]) and np.array_equal(y[i], yr[i]), i
    bd.close()
    ref.close()


# ------------------------------------------------------------------ 9: edges
def test_batch_of_one_equals_the_single_handle(pgf):
    prob = bordered_lq(100, 2, 10, 1, 1, seed=5)
    n, m = prob.num_vars, prob.num_cons
    bd = _batch([prob], "Full")
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(n), np.zeros(m), 1.0, 1.0)
    assert bd.band and bd.band_border == 2 and dn.sparse
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


def test_seventy_tiny_instances(pgf):
    probs = [bordered_lq(60, 2, 8, 1, 1, seed=i) for i in range(70)]
    _narrow(probs, k=2)
    bd, ref = _batch(probs, "Full"), _batch(probs, "Full", sequential=True)
    for k in range(2):
        same_step(bd, ref, k)
    fac, sol = bd.border_stats()
    assert np.all(fac == 2) and np.all(sol == 2) and fac.size == 70
    bd.close()
    ref.close()


def test_without_a_border_the_flag_changes_nothing(pgf):
    from pygradflow_amd import problems

    def make():
        return [forced(problems.box_qp(264, seed=i)) for i in range(3)]

    bd, plain = _batch(make(), "Full", border=True), _batch(make(), "Full", border=False)
    assert bd.band and bd.band_border == 0 and plain.band_border == 0
    for k in range(2):
        same_step(bd, plain, k)
    assert bd.band_stats() == plain.band_stats() == (2, 2)
    fac, sol = bd.border_stats()
    assert not fac.any() and not sol.any()
    bd.close()
    plain.close()
    # PGF_BATCH_BORDER | PGF_BATCH_BAND_CTL without a border means PGF_BATCH_BAND_CTL alone
    bd = _batch(make(), "Full", border=True, band_ctl=True)
    assert bd.band and bd.band_ctl and not bd.step_local()[0].any()
    bd.close()


# ------------------------------------------------------------------ 10: refusals
def test_what_a_bordered_batch_refuses(pgf):
    def steps_correctly():
        probs = [bordered_lq(100, 2, 10, 1, 1, seed=40 + i) for i in range(2)]
        bd, ref = _batch(probs, "Full"), _batch(probs, "Full", sequential=True)
        same_step(bd, ref, "after a refusal")
        bd.close()
        ref.close()

    narrow = lambda: [bordered_lq(100, 2, 10, 1, 1, seed=i) for i in range(2)]  # noqa: E731
    with pytest.raises(ValueError, match="batch: a bordered band cannot join a device batch"):
        _batch(narrow(), "Full", border=False)
    steps_correctly()
    # one (n, m) = (101, 11), borders of two nodes and of one
    mixed = [bordered_lq(100, 2, 10, 1, 1, seed=0), bordered_lq(101, 2, 10, 0, 1, seed=1)]
    assert [plan_of(p).k for p in mixed] == [2, 1] and all(plan_of(p).block_size == 8 for p in mixed)
    with pytest.raises(ValueError, match="batch: banded instances must share the border size"):
        _batch(mixed, "Full")
    steps_correctly()
    wide = [bordered_lq(100, 3, 10, 1, 1, seed=i) for i in range(2)]
    assert plan_of(wide[0]).block_size == 16 and plan_of(wide[0]).k == 2
    for kw in ({}, {"wide_band": True}):
        with pytest.raises(ValueError, match=r"narrow route only \(block size 8\)"):
            _batch(wide, "Full", **kw)
    steps_correctly()
    with pytest.raises(ValueError, match="the device-resident controller does not drive a bordered band batch"):
        _batch(narrow(), "Full", band_ctl=True)
    steps_correctly()
