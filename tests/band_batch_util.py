"""The harness of the banded device batch's GPU tests (test_band_batch*_gpu.py): one constructor
and one copy of each comparison.

The bars.  Against the sequential twin (``sequential=True``: the same instances one by one through
their own handles, the same device functions in the same order): statuses equal, masks, x and y bit
for bit (``np.array_equal``), the inertia exactly on every instance that stepped, the step length
within 1e-14 relative (its sum is taken in another order).  Against the CPU oracle: masks identical,
x and y within ``band_util.TOL`` (1e-10), n_neg = m."""

import numpy as np

from oracle import newton_oracle as O
from tests import golden_util as G
from tests.band_util import TOL


def make_batch(probs, pol, dt=1.0, rho=1.0, sequential=False, **flags):
    """BatchedDeviceNewton over ``probs``; flags: wide_band, band_ctl, border, wide_border."""
    from pygradflow_amd.batched import BatchedDeviceNewton

    return BatchedDeviceNewton(lambda i: probs[i], len(probs), pol, dt, rho, sequential=sequential, **flags)


def same_step(bd, ref, tag, ok=True):
    """One step of the batch and of its twin, under the twin's bars of the module docstring; with
    ``ok`` every status is zero besides.  Returns (statuses, n_neg) of the batch."""
    st, nn, df = bd.step_local()
    st2, nn2, df2 = ref.step_local()
    assert np.array_equal(st, st2), (tag, st, st2)
    if ok:
        assert not st.any() and not st2.any(), (tag, st, st2)
    assert np.array_equal(bd.masks(), ref.masks()), tag
    (x, y), (x2, y2) = bd.points(), ref.points()
    assert np.array_equal(x, x2), (tag, G.rel_err(x, x2))
    assert np.array_equal(y, y2), (tag, G.rel_err(y, y2))
    good = st == 0
    assert np.array_equal(nn[good], nn2[good]), (tag, nn, nn2)
    assert np.all(np.abs(df - df2) <= 1e-14 * np.abs(df2)), (tag, df, df2)
    return st, nn


def same_as_sequential(batch, probs, policies=(("Full", 2), ("Simplified", 1)), opened=None, after=None):
    """Fresh instances per policy, ``batch(probs, pol)`` against its sequential twin: same_step with
    n_neg = m at every step, one batched reduction launch per step.  ``opened(bd)`` and
    ``after(bd, pol, steps)`` hold what the route asserts of a batch just created and of its counters
    at the end."""
    m = probs[0].num_cons
    for pol, steps in policies:
        bd, ref = batch(probs, pol), batch(probs, pol, sequential=True)
        assert bd.band
        if opened is not None:
            opened(bd)
        for k in range(steps):
            _, nn = same_step(bd, ref, (pol, k))
            assert np.all(nn == m), (pol, k, nn)
        assert bd.band_stats()[0] == steps
        if after is not None:
            after(bd, pol, steps)
        bd.close()
        ref.close()


def churn_of(recs):
    """Steps whose mask differs from the step before, summed over the instances' oracle records."""
    return sum(int(not np.array_equal(a["mask"], b["mask"])) for r in recs for a, b in zip(r, r[1:]))


def against_oracle(batch, probs, policies, dt=1.0, rho=1.0, check_recs=None, opened=None):
    """Every instance of ``batch(probs, pol, dt, rho)`` against NewtonOracle from zero, under the
    oracle's bars of the module docstring; returns churn_of summed over the policies.
    ``check_recs(pol, recs)`` sees the oracle's records (recs[instance][step]) before the batch is
    created; ``opened(bd)`` as in same_as_sequential."""
    n, m = probs[0].num_vars, probs[0].num_cons
    x0, y0 = np.zeros(n), np.zeros(m)
    churn = 0
    for pol, steps in policies:
        recs = [O.NewtonOracle(p, pol, x0, y0, dt, rho).run(x0, y0, steps) for p in probs]
        if check_recs is not None:
            check_recs(pol, recs)
        bd = batch(probs, pol, dt, rho)
        assert bd.band
        if opened is not None:
            opened(bd)
        for k in range(steps):
            st, nn, _ = bd.step_local()
            assert not st.any(), (pol, k, st)
            mk = bd.masks()
            x, y = bd.points()
            for i, rec in enumerate(recs):
                assert np.array_equal(mk[i], rec[k]["mask"]), (pol, k, i)
                assert G.rel_err(x[i], rec[k]["xn"]) <= TOL, (pol, k, i)
                assert G.rel_err(y[i], rec[k]["yn"]) <= TOL, (pol, k, i)
                assert nn[i] == m, (pol, k, i, nn[i])
        bd.close()
        churn += churn_of(recs)
    return churn


_HANDLE_FIELDS = {
    "border": lambda s: s.border_stats()[1:],  # (factor phases, solve phases)
    "band": lambda s: s.band_stats()[:2],  # (reductions, solve phases)
    "refined": lambda s: s.refinement_stats()[:1],  # (refinement steps,)
}


def handle_stats(ref, fields):
    """The counters named in ``fields`` (keys of _HANDLE_FIELDS, in that order) on the handles of a
    sequential run: one row per counter, one column per instance.  Handles are pooled: use
    differences."""
    return np.array([sum((tuple(_HANDLE_FIELDS[f](s)) for f in fields), ()) for s in ref.solvers]).T


def phases(bd):
    """(factor phases, solve phases) per instance of a bordered wide batch, which the border's and
    the wide band's counters must both report."""
    fac, sol = bd.border_stats()
    red, kept, _ = bd.band_wide_stats()
    assert np.array_equal(fac, red) and np.array_equal(sol, kept), (fac, red, sol, kept)
    return fac, sol
