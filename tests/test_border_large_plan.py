"""Host plan of the LARGE border (65 .. 1024 border nodes: BandPlan(border_limit=...),
select_border(pat, limit), csrc/pgf_border_large.hip): the limit's validation, the layout with
kp = k rounded up to 64 restated in numpy against the oracle's KKT matrix (the restatement of
test_border_plan.py, which takes any kp), the block size of the remainder, and the automatic border
of multistate_ocp(300, 24, 8) with and without the limit.  CPU only."""

import numpy as np
import pytest

from pygradflow_amd import problems
from pygradflow_amd.sparse import MAX_BANDWIDTH, MAX_BORDER, MAX_LARGE_BORDER, BandPlan, border_key
from tests.band_util import case
from tests.test_border_plan import oracle_full, restate


def _plan(prob, border=None, limit=None, **kw):
    """The plan of the problem's own border (or ``border``) and forced block under ``limit``."""
    return BandPlan(prob.hess_sparse(), prob.jac_sparse(), prob.num_vars, prob.num_cons,
                    block=getattr(prob, "pgf_band_block", None),
                    border=getattr(prob, "pgf_border", None) if border is None else border,
                    border_limit=limit, **kw)


def test_limit_validation():
    assert (MAX_BORDER, MAX_LARGE_BORDER) == (64, 1024)
    prob = case(65, 99)
    for bad in (63, 1025, 0, -1, 100.0, "1024", True):
        with pytest.raises(ValueError, match="pgf_border_limit"):
            _plan(prob, limit=bad)
    with pytest.raises(ValueError, match="at most 64"):  # k = 65 without a limit: as ever
        _plan(prob)
    with pytest.raises(ValueError, match="at most 64"):
        _plan(prob, limit=64)
    with pytest.raises(ValueError, match="at most 70"):  # k > limit
        _plan(case(71, 99), limit=70)
    assert _plan(prob, limit=65).k == 65 and _plan(prob, limit=1024).k == 65
    small = case(64, 99)
    a, b = _plan(small), _plan(small, limit=1024)  # k <= 64: the limit changes nothing but the key
    assert (a.k, a.kp, a.large) == (b.k, b.kp, b.large) == (64, 64, False)
    assert np.array_equal(a.Hslot, b.Hslot) and np.array_equal(a.Jslot, b.Jslot) and np.array_equal(a.pos, b.pos)
    assert a.store_size == b.store_size and a.block_size == b.block_size


def test_plan_key_includes_the_limit():
    assert border_key(None) is None and border_key("auto") == "auto" and border_key([3, 1]) == (3, 1)
    keys = [border_key("auto"), border_key("auto", 64), border_key("auto", 1024), border_key([3, 1], 1024),
            border_key([3, 1]), border_key(None, 1024)]
    assert len(set(keys)) == len(keys)
    prob = case(64, 99)
    assert _plan(prob).border_spec != _plan(prob, limit=1024).border_spec
    assert _plan(prob, limit=1024).border_spec == border_key(prob.pgf_border, 1024)


@pytest.mark.parametrize("k,kp", [(65, 128), (128, 128), (257, 320)])
def test_layout_with_kp_a_multiple_of_64(k, kp):
    """Border variables and constraints mixed, one border variable active and one not: C (Nb x kp),
    the lower triangle of D and the identity padding land where the device reads them."""
    prob = case(k, 57, mloc=12, seed=k)
    n, m = prob.num_vars, prob.num_cons
    kv = k // 3
    plan = _plan(prob, limit=1024)
    assert (plan.k, plan.kp, plan.Nb, plan.large, plan.supported) == (k, kp, 57, True, True)
    assert list(plan.border) == list(range(45, n)) + list(range(n + 12, n + m))
    assert np.array_equal(plan.pos[plan.border], 57 + np.arange(k))
    assert plan.base_C == 58 * plan.ldb and plan.base_D == plan.base_C + 57 * kp
    assert plan.store_size == plan.base_D + kp * kp
    hv, jv = plan.values(prob.hess_sparse(), prob.jac_sparse())
    mask = np.random.default_rng(k).uniform(size=n) < 0.4
    mask[45], mask[46] = True, False
    assert kv >= 2
    lamb, rho = 0.8, 1.7
    assert np.array_equal(restate(plan, hv, jv, mask, lamb, lamb / (1.0 + lamb * rho)),
                          oracle_full(prob, mask, lamb, rho, plan.pos))


def test_block_size_under_a_large_border():
    narrow = case(128, 1003, bw=2)
    plan = _plan(narrow, limit=1024)
    assert plan.bw == 5 and plan.block_size == 16 and plan.block is None  # lifted from 8
    assert _plan(case(64, 1003, bw=2), limit=1024).block_size == 8       # a small border is not
    wide = case(257, 1003, bw=12)
    plan = _plan(wide, limit=1024)
    assert plan.bw == 41 and plan.block_size == 64
    for forced in (16, 32, 64):
        narrow.pgf_band_block = forced
        assert _plan(narrow, limit=1024).block_size == forced
    narrow.pgf_band_block = 8
    with pytest.raises(ValueError, match="pgf_band_block"):
        _plan(narrow, limit=1024)
    narrow.pgf_band_block = None
    with pytest.raises(ValueError, match="pgf_band_split"):
        _plan(narrow, limit=1024, split=False)
    assert _plan(narrow, limit=1024, split=True).block_size == 16
    assert _plan(case(64, 99), limit=1024, split=False).k == 64  # (a small border runs without the split)


def test_effective_split_includes_the_default(monkeypatch):
    """What the solvers hand to BandPlan(split=...): the problem's setting or, without one, the
    library's default -- PGF_BW_SPLIT=0 alone must already refuse a large border with a ValueError."""
    from pygradflow_amd.sparse import effective_band_split

    prob = case(128, 99)
    monkeypatch.delenv("PGF_BW_SPLIT", raising=False)
    assert effective_band_split(prob) is True
    monkeypatch.setenv("PGF_BW_SPLIT", "0")
    assert effective_band_split(prob) is False
    with pytest.raises(ValueError, match="pgf_band_split"):
        _plan(prob, limit=1024, split=effective_band_split(prob))
    prob.pgf_band_split = True  # the problem's own setting wins
    assert effective_band_split(prob) is True
    assert _plan(prob, limit=1024, split=effective_band_split(prob)).k == 128


def test_multistate_ocp_needs_the_limit():
    prob = problems.multistate_ocp(300, 24, 8)
    plan = _plan(prob, "auto")
    assert plan.supported is False and plan.k == 64 and plan.bw > MAX_BANDWIDTH  # pinned: test_border_plan.py
    plan = _plan(prob, "auto", limit=1024)
    assert plan.supported and plan.k == 299 and plan.kp == 320 and plan.bw <= 64
    assert plan.block_size in (16, 32, 64) and plan.block_size >= plan.bw
    assert plan.Nb == prob.num_vars + prob.num_cons - 299
    assert _plan(prob, "auto", limit=298).supported is False  # one node short
