"""Bordered instances on the WIDE route in the banded device batch (PGF_BATCH_WIDE_BORDER;
csrc/pgf_border.hip around the twins in csrc/pgf_band_wide.hip): a band of block size 16,
32 or 64 plus 1 <= k <= 64 border nodes per instance, one launch sequence per Newton step.  An
instance whose matrix changed factorises B once (the factor-only reduction that keeps its
multipliers) and forms Y = inv(B) C by one panel solve on the matrix pipes; every live instance
solves against the kept factors every step.

Two references, with the bars of band_batch_util.py: ``sequential=True``, which drives the same
instances one by one through their own handles (both routes run the same device functions of
pgf_band_wide_dev.h and pgf_border_dev.h in the same order), and the CPU oracle, with
cond(K) <= 1e4 (band_util.COND_MAX) asserted on the host first.

Shapes, each asserted on the host with ``plan_of`` before it is used, as (k, Nb, bw, block):

  border widths   case(k, 203, block=B), k = 1 | 16 | 17 | 64, B = 16 | 32 | 64: kp = 16 | 16 | 32 |
                  64, so 1, 2, 4 column tiles per tile row of the panel kernels, 16 output tiles at
                  B = 64 with k = 64; 13, 7, 4 blocks
  row counts      case(17, Nb, block=B), Nb = 1, 9, B - 1, B, B + 1, 2 B + 1, 257, 513: one ragged
                  block (the last-block launch is the whole panel solve), exactly one block, one row
                  into a second, three blocks, either side of the 256-row workgroups and of
                  SP_BORDER_CHUNK = 512
  automatic       bordered_lq(100, 3, 10, 1, 1): (2, 110, 9, 16); bordered_lq(200, 3, 40, 2, 2):
                  (4, 240, 9, 16); case(48, 300, bw=22, mloc=0): (48, 300, 22, 32);
                  case(17, 300, bw=40, mloc=0): (17, 300, 40, 64); ocp_global_parameter(12, 4, 2, 2)
                  with the automatic border: (2, 120, 10, 16)
"""

import ctypes as C
import functools

import numpy as np
import pytest

from oracle import newton_oracle as O
from tests import golden_util as G
from tests.band_batch_util import (against_oracle, churn_of, handle_stats, make_batch, phases, same_as_sequential,
                                   same_step)
from tests.band_util import (COND_MAX, bordered_lq, case, guard_case, mask_change_steps, plan_of, reduced_kkt,
                             singular_schur_wide, wide_band_problem)

pytestmark = pytest.mark.gpu

POLICIES = ("Simplified", "Full", "ActiveSet")
BLOCKS = (16, 32, 64)

_batch = functools.partial(make_batch, wide_border=True)


def _wide(probs, k=None, Nb=None, bw=None, block=None):
    """The host-side check of the module docstring; every instance on one pattern and one ordering."""
    plans = [plan_of(p) for p in probs]
    p0 = plans[0]
    assert all(pl.supported and pl.block_size in BLOCKS and pl.k >= 1 for pl in plans)
    assert len({pl.pattern_hash() for pl in plans}) == 1
    assert all(np.array_equal(pl.pos, p0.pos) for pl in plans)
    for name, want, got in (("k", k, p0.k), ("Nb", Nb, p0.Nb), ("bw", bw, p0.bw), ("block", block, p0.block_size)):
        assert want is None or want == got, (name, want, got)
    return p0


def _as_one_by_one(probs):
    """same_as_sequential with the flags the keyword derives, the plan's sizes and the phase counters."""
    plan = plan_of(probs[0])

    def opened(bd):
        assert bd.wide_band and bd.border and bd.wide_border
        assert bd.band_border == plan.k and bd.band_block == plan.block_size

    def after(bd, pol, steps):
        fac, sol = phases(bd)
        assert np.all(sol == steps) and np.all(fac == (steps if pol == "Full" else 1)), (pol, fac, sol)

    same_as_sequential(_batch, probs, opened=opened, after=after)


# ------------------------------------------------------------------ 1: the batch exists
def test_wide_bordered_instances_form_a_device_batch(pgf):
    probs = [bordered_lq(100, 3, 10, 1, 1, seed=i) for i in range(3)]
    _wide(probs, k=2, Nb=110, bw=9, block=16)
    bd = _batch(probs, "Full")
    assert bd.band and bd._b is not None and bd.band_border == 2 and bd.band_block == 16
    assert bd.wide_band and bd.border
    for _ in range(2):
        st, nn, _ = bd.step_local()
        assert not st.any() and np.all(nn == probs[0].num_cons)
    fac, sol = phases(bd)
    assert list(fac) == [2, 2, 2] and list(sol) == [2, 2, 2]
    assert bd.band_stats() == (2, 2)
    bd.close()


# ------------------------------------------------------------------ 2: border widths
@pytest.mark.parametrize("block", BLOCKS)
@pytest.mark.parametrize("k", [1, 16, 17, 64])
def test_border_widths_as_one_by_one(pgf, k, block):
    probs = [case(k, 203, block=block, seed=1000 * k + block + i) for i in range(3)]
    plan = _wide(probs, k=k, Nb=203, block=block)
    assert plan.kp == {1: 16, 16: 16, 17: 32, 64: 64}[k]
    assert (203 + block - 1) // block == {16: 13, 32: 7, 64: 4}[block]
    _as_one_by_one(probs)


# ------------------------------------------------------------------ 3: row counts
def _row_counts(block):
    return (1, 9, block - 1, block, block + 1, 2 * block + 1, 257, 513)


@pytest.mark.parametrize("block,Nb", [(b, nb) for b in BLOCKS for nb in _row_counts(b)])
def test_row_counts_as_one_by_one(pgf, block, Nb):
    probs = [case(17, Nb, block=block, seed=17000 + Nb + block + i) for i in range(3)]
    _wide(probs, k=17, Nb=Nb, block=block)
    _as_one_by_one(probs)


# ------------------------------------------------------------------ 4: automatic wide plans
def _ocp(seed):
    from pygradflow_amd import problems

    prob = problems.ocp_global_parameter(12, 4, 2, 2, seed=seed)
    prob.pgf_border = "auto"
    return prob


AUTOMATIC = {
    "lq100": (lambda i: bordered_lq(100, 3, 10, 1, 1, seed=i), (2, 110, 9, 16)),
    "lq200": (lambda i: bordered_lq(200, 3, 40, 2, 2, seed=i), (4, 240, 9, 16)),
    "bw22": (lambda i: case(48, 300, bw=22, mloc=0, seed=4 + i), (48, 300, 22, 32)),
    "bw40": (lambda i: case(17, 300, bw=40, mloc=0, seed=40 + i), (17, 300, 40, 64)),
    "ocp": (lambda i: _ocp(1 + i), (2, 120, 10, 16)),
}


@pytest.mark.parametrize("name", sorted(AUTOMATIC))
def test_automatic_wide_plans_as_one_by_one(pgf, name):
    make, (k, Nb, bw, block) = AUTOMATIC[name]
    probs = [make(i) for i in range(3)]
    assert all(getattr(p, "pgf_band_block", None) is None for p in probs)
    _wide(probs, k=k, Nb=Nb, bw=bw, block=block)
    _as_one_by_one(probs)


# ------------------------------------------------------------------ 5: against the oracle
def _oracle_run(probs):
    def check_recs(pol, recs):
        for p, r in zip(probs, recs):
            for rec in r:
                cond = np.linalg.cond(reduced_kkt(p, rec["mask"]))
                assert cond <= COND_MAX, (pol, cond)
        if pol != "Simplified":  # (which keeps its mask by definition)
            assert all(churn_of([r]) > 0 for r in recs), pol

    def opened(bd):
        assert bd.band_border and bd.band_block in BLOCKS

    against_oracle(_batch, probs, tuple((p, 3) for p in POLICIES), check_recs=check_recs, opened=opened)


@pytest.mark.parametrize("name", ["lq100", "lq200", "ocp"])
def test_against_the_oracle(pgf, name):
    """Seeds chosen on the CPU (band_util.mask_changes): every instance's active set changes between
    the three steps under Full and under ActiveSet."""
    make, (k, Nb, bw, block) = AUTOMATIC[name]
    probs = [make(i) for i in range(3)]
    _wide(probs, k=k, Nb=Nb, bw=bw, block=block)
    _oracle_run(probs)


# ------------------------------------------------------------------ 6: phases per instance
def test_factor_phase_only_where_the_matrix_changed(pgf):
    """One pattern, three boxes: +-0.5 (the mask changes at every step), +-1.5 (at the second step
    only), +-5 (never active).  Under ActiveSet each instance factors where its own mask changed; the
    batch's counters are those of the handles in the sequential twin, step by step."""
    probs = [bordered_lq(200, 3, 40, 2, 2, seed=s, bound=b) for s, b in ((0, 0.5), (1, 1.5), (2, 5.0))]
    _wide(probs, k=4, Nb=240, bw=9, block=16)
    ch = [mask_change_steps(p, "ActiveSet", 4) for p in probs]
    assert ch == [[True, True, True], [True, False, False], [False, False, False]]
    want = [4, 2, 1]  # (the first step always factors)
    bd, ref = _batch(probs, "ActiveSet"), _batch(probs, "ActiveSet", sequential=True)
    base = handle_stats(ref, ("border", "band"))
    for k in range(4):
        same_step(bd, ref, k)
        fac, sol = phases(bd)
        hf, hs, hred, hkept = handle_stats(ref, ("border", "band")) - base
        assert np.array_equal(fac, hf) and np.array_equal(sol, hs), (k, fac, hf, sol, hs)
        assert np.array_equal(fac, hred) and np.array_equal(sol, hkept), (k, fac, hred, sol, hkept)
    fac, sol = phases(bd)
    assert list(sol) == [4, 4, 4] and list(fac) == want, (fac, want)
    assert bd.band_wide_stats()[2] == 0  # (the policy may change the mask: never lean)
    bd.close()
    ref.close()
    # Simplified: one factor phase, then two lean steps without a factor-phase launch, which leave the
    # factor counters alone
    bd, ref = _batch(probs, "Simplified"), _batch(probs, "Simplified", sequential=True)
    same_step(bd, ref, ("Simplified", 0))
    fac1, _ = phases(bd)
    for k in (1, 2):
        same_step(bd, ref, ("Simplified", k))
    fac, sol = phases(bd)
    assert list(fac1) == list(fac) == [1, 1, 1] and list(sol) == [3, 3, 3]
    assert bd.band_wide_stats()[2] == 2 and bd.band_stats() == (3, 1)
    bd.close()
    ref.close()


# ------------------------------------------------------------------ 7: per-instance outer steps
def test_per_instance_outer_steps_rejection_and_freezing(pgf):
    probs = [bordered_lq(200, 3, 40, 2, 2, seed=20 + i) for i in range(3)]
    _wide(probs, k=4, Nb=240, bw=9, block=16)
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
    # instance 1 frozen: its point, its mask and all its counters stay
    fac0, sol0 = phases(bd)
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
    fac, sol = phases(bd)
    assert list(fac - fac0) == [2, 0, 2] and list(sol - sol0) == [2, 0, 2]
    # the next outer step thaws it
    for run in (bd, ref):
        run.advance_outer_each(dt, 1.0)
    ref.set_frozen(None)  # (the sequential loop keeps its own list until told otherwise)
    same_step(bd, ref, "thawed")
    fac, sol = phases(bd)
    assert list(fac - fac0) == [3, 1, 3] and list(sol - sol0) == [3, 1, 3]
    bd.close()
    ref.close()


# ------------------------------------------------------------------ 8: a bad pivot in one instance
@pytest.mark.parametrize("block", [16, 64])
def test_a_singular_schur_complement_in_one_instance(pgf, block):
    """A decoupled border variable with H[v, v] = -lambda in the middle instance: B is as regular as
    ever, S meets an exact zero pivot.  The instance reports PGF_SINGULAR and keeps its point, its
    neighbours are those of the sequential twin bit for bit, and at lambda = 2 it factors again and
    steps cleanly."""
    from pygradflow_amd import _lib

    goods = [case(6, 203, block=block, seed=6203 + i) for i in range(3)]
    bad, v = singular_schur_wide(goods[1])
    probs = [goods[0], bad, goods[2]]
    plan = _wide(probs, k=6, Nb=203, block=block)
    assert plan.pos[v] == 203 + 1  # a border node
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
    fac, sol = phases(bd)
    assert list(fac) == [1, 1, 1] and list(sol) == [1, 1, 1]
    for run in (bd, ref):
        run.advance_outer_each(np.array([1.0, 0.5, 1.0]), 1.0, accepted=[True, False, True])
    st, nn = same_step(bd, ref, "regular")
    assert np.all(nn == m)
    x, _ = bd.points()
    assert x[1].any()
    fac, sol = phases(bd)
    assert list(fac) == [2, 2, 2] and list(sol) == [2, 2, 2]
    bd.close()
    ref.close()
    # Simplified keeps the mask, so only ctl[1] == 0 can make the singular instance factor again: it
    # does, before every solve, while the good ones factor once
    bd = _batch(probs, "Simplified")
    for k in range(3):
        st, _, _ = bd.step_local()
        assert list(st) == [0, _lib.PGF_SINGULAR, 0], k
    fac, sol = phases(bd)
    assert list(fac) == [1, 3, 1] and list(sol) == [3, 3, 3]
    assert bd.band_wide_stats()[2] == 0  # (never lean while an instance is bad)
    bd.close()


def _guard_neighbours(block):
    """Two instances on the pattern of guard_case(1, block, .): k = 1, Nb = 300, half-width 8."""
    return [bordered_lq(300, 8, 0, 0, 1, 186 + 100 * i, block=block, bound=1e6) for i in range(2)]


@pytest.mark.parametrize("block", [16, 64])
def test_a_zero_pivot_in_the_band_of_one_instance(pgf, block):
    """band_util.guard_case(1, block, 0.0) in the middle: K[v, v] = 0 at the head of
    block 1 of B, which level one of the factor-only reduction inverts as it stands.  The flag is
    parked with those of S and comes back in front of the solve phase: PGF_SINGULAR, the point kept,
    a new factor phase before every further solve (Simplified keeps the mask), the neighbours bit for
    bit those of the sequential twin."""
    from pygradflow_amd import _lib

    bad, v = guard_case(1, block, 0.0)
    K = reduced_kkt(bad, np.zeros(bad.num_vars, dtype=bool))
    assert K[v, v] == 0.0 and np.linalg.cond(K) < 1e6
    others = _guard_neighbours(block)
    probs = [others[0], bad, others[1]]
    _wide(probs, k=1, Nb=300, block=block)
    bd, ref = _batch(probs, "Simplified"), _batch(probs, "Simplified", sequential=True)
    for k in range(2):
        st, nn, _ = bd.step_local()
        st2, nn2, _ = ref.step_local()
        assert list(st) == list(st2) == [0, _lib.PGF_SINGULAR, 0], (k, st, st2)
        (x, y), (x2, y2) = bd.points(), ref.points()
        assert not x[1].any() and not y[1].any()
        for i in (0, 2):
            assert np.array_equal(x[i], x2[i]) and np.array_equal(y[i], y2[i]) and nn[i] == nn2[i], (k, i)
    fac, sol = phases(bd)
    assert list(fac) == [1, 2, 1] and list(sol) == [2, 2, 2]
    bd.close()
    ref.close()


# ------------------------------------------------------------------ 9: guard repair
@pytest.mark.parametrize("block", [16, 64])
def test_an_unstable_pivot_in_one_instance_is_repaired_on_its_handle(pgf, block):
    """guard_case(1, block, 1e-9) as instance 1 of three: a 1e-9 pivot at the head of block 1 of B, an
    instability chosen on the CPU (K is regular, cond < 1e5).  The handle repairs it by solve phases
    against the factors, Y and S the batch left; bar: that of test_bordered_unstable_pivot_is_refined
    for refined solves, 1e-9, against the oracle and against the sequential twin."""
    prob, v = guard_case(1, block, 1e-9)
    others = _guard_neighbours(block)
    probs = [others[0], prob, others[1]]
    _wide(probs, k=1, Nb=300, block=block)
    n, m = prob.num_vars, prob.num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    rec = O.NewtonOracle(prob, "Full", x0, y0, 1.0, 1.0).run(x0, y0, 1)[0]
    assert not rec["mask"].any()
    K = reduced_kkt(prob, rec["mask"])
    assert abs(K[v, v]) < 1e-8 and np.linalg.cond(K) < 1e5
    bd, ref = _batch(probs, "Full"), _batch(probs, "Full", sequential=True)
    before = bd.repaired()
    h0 = bd.solvers[1].band_stats()
    st, nn, _ = bd.step_local()
    ref.step_local()
    h1 = bd.solvers[1].band_stats()
    x, y = bd.points()
    xr, yr = ref.points()
    print(f"block {block}: status {st}, repaired {bd.repaired() - before}, x error "
          f"{G.rel_err(x[1], rec['xn']):.3e}, y error {G.rel_err(y[1], rec['yn']):.3e}, against the twin "
          f"{G.rel_err(x[1], xr[1]):.3e} {G.rel_err(y[1], yr[1]):.3e}, handle {tuple(a - b for a, b in zip(h1, h0))}")
    assert not st.any()
    assert bd.repaired() > before
    assert G.rel_err(x[1], rec["xn"]) <= 1e-9 and G.rel_err(y[1], rec["yn"]) <= 1e-9
    assert G.rel_err(x[1], xr[1]) <= 1e-9 and G.rel_err(y[1], yr[1]) <= 1e-9
    # the corrections on the handle were solve phases: it never reduced B again
    assert h1[0] == h0[0] and h1[1] > h0[1], (h0, h1)
    fac, sol = phases(bd)
    assert list(fac) == [1, 1, 1] and list(sol) == [1, 1, 1]
    for i in (0, 2):
        assert np.array_equal(x[i], xr[i]) and np.array_equal(y[i], yr[i]), i
    bd.close()
    ref.close()


# ------------------------------------------------------------------ 10: batch sizes
def test_batch_of_one_equals_the_single_handle(pgf):
    prob = bordered_lq(100, 3, 10, 1, 1, seed=5)
    _wide([prob], k=2, Nb=110, bw=9, block=16)
    n, m = prob.num_vars, prob.num_cons
    bd = _batch([prob], "Full")
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(n), np.zeros(m), 1.0, 1.0)
    assert bd.band and bd.band_border == 2 and bd.band_block == 16 and dn.sparse
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
    """The smallest shape of the row counts, (17, 1, 0, 16): one band row, one ragged block."""
    probs = [case(17, 1, block=16, seed=900 + i) for i in range(70)]
    _wide(probs, k=17, Nb=1, block=16)
    bd, ref = _batch(probs, "Full"), _batch(probs, "Full", sequential=True)
    for k in range(2):
        same_step(bd, ref, k)
    fac, sol = phases(bd)
    assert np.all(fac == 2) and np.all(sol == 2) and fac.size == 70
    bd.close()
    ref.close()


def test_the_flag_changes_nothing_for_narrow_borders_and_unbordered_wide_bands(pgf):
    # a narrow bordered batch: as under PGF_BATCH_BORDER alone
    def narrow():
        return [bordered_lq(100, 2, 10, 1, 1, seed=i) for i in range(3)]

    assert plan_of(narrow()[0]).block_size == 8 and plan_of(narrow()[0]).k == 2
    bd, old = _batch(narrow(), "Full"), _batch(narrow(), "Full", wide_border=False, border=True)
    assert bd.band_block == old.band_block == 8 and bd.band_border == old.band_border == 2
    for k in range(2):
        same_step(bd, old, ("narrow", k))
    assert bd.band_stats() == old.band_stats() == (2, 2)
    for a, b in zip(bd.border_stats() + bd.band_wide_stats(), old.border_stats() + old.band_wide_stats()):
        assert np.array_equal(a, b)
    bd.close()
    old.close()

    # a wide batch without a border: as under PGF_BATCH_WIDE_BAND alone
    def wide():
        rng = np.random.default_rng(8)
        return [wide_band_problem(300, 2.5 + rng.uniform(0.0, 0.5, 300), 1 + i) for i in range(3)]

    pl = plan_of(wide()[0])
    assert pl.block_size == 16 and pl.k == 0
    for pol, steps in (("Full", 2), ("Simplified", 2)):
        bd, old = _batch(wide(), pol), _batch(wide(), pol, wide_border=False, wide_band=True)
        assert bd.band_block == old.band_block == 16 and bd.band_border == old.band_border == 0
        for k in range(steps):
            same_step(bd, old, ("wide", pol, k))
        assert bd.band_stats() == old.band_stats()
        for a, b in zip(bd.border_stats() + bd.band_wide_stats(), old.border_stats() + old.band_wide_stats()):
            assert np.array_equal(a, b)
        assert not bd.border_stats()[0].any()
        bd.close()
        old.close()


# ------------------------------------------------------------------ 11: refusals
def test_what_a_wide_bordered_batch_refuses(pgf):
    from pygradflow_amd import _lib

    def steps_correctly():
        probs = [bordered_lq(100, 3, 10, 1, 1, seed=40 + i) for i in range(2)]
        bd, ref = _batch(probs, "Full"), _batch(probs, "Full", sequential=True)
        same_step(bd, ref, "after a refusal")
        bd.close()
        ref.close()

    def wide():
        return [bordered_lq(100, 3, 10, 1, 1, seed=i) for i in range(2)]

    assert plan_of(wide()[0]).block_size == 16 and plan_of(wide()[0]).k == 2
    # the factor / solve split off
    off = wide()
    for p in off:
        p.pgf_band_split = False
    with pytest.raises(ValueError, match="batch: a bordered wide band needs the factor / solve split"):
        _batch(off, "Full")
    steps_correctly()
    # one (n, m) = (101, 11), borders of two nodes and of one
    mixed = [bordered_lq(100, 3, 10, 1, 1, seed=0), bordered_lq(101, 3, 10, 0, 1, seed=1, block=16)]
    assert [plan_of(p).k for p in mixed] == [2, 1] and all(plan_of(p).block_size == 16 for p in mixed)
    with pytest.raises(ValueError, match="batch: banded instances must share the border size"):
        _batch(mixed, "Full")
    steps_correctly()
    # one pattern, block sizes 16 and 32
    blocks = [case(17, 203, block=16, seed=1), case(17, 203, block=32, seed=2)]
    assert plan_of(blocks[0]).pattern_hash() == plan_of(blocks[1]).pattern_hash()
    assert [plan_of(p).block_size for p in blocks] == [16, 32]
    with pytest.raises(ValueError, match="batch: banded instances must share the block size"):
        _batch(blocks, "Full")
    steps_correctly()
    # the new bit without one of the other two, or without both: PGF_INVALID before any handle is read
    hold = _batch(wide(), "Full", sequential=True)
    arr = (C.c_void_p * 2)(*[s._hd.h for s in hold.solvers])
    out = C.c_void_p()
    lib = _lib.load()
    for flags in (_lib.BATCH_WIDE_BORDER, _lib.BATCH_WIDE_BORDER | _lib.BATCH_BORDER,
                  _lib.BATCH_WIDE_BORDER | _lib.BATCH_WIDE_BAND,
                  _lib.BATCH_WIDE_BORDER | _lib.BATCH_BAND_CTL | _lib.BATCH_BORDER):
        assert lib.pgf_batch_create_ex(arr, 2, flags, C.byref(out)) == _lib.PGF_INVALID, flags
        assert not out.value
    hold.close()
    steps_correctly()
    # without the new bit the refusal keeps its text
    for kw in ({"border": True}, {"border": True, "wide_band": True}):
        with pytest.raises(ValueError, match=r"narrow route only \(block size 8\)"):
            _batch(wide(), "Full", wide_border=False, **kw)
    steps_correctly()
    # a border under the device-resident controller stays refused
    with pytest.raises(ValueError, match="the device-resident controller does not drive a bordered band batch"):
        _batch(wide(), "Full", band_ctl=True)
    steps_correctly()
