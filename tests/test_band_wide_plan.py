"""Band plan of the wide cyclic reduction (CPU only): bandwidths of the multi-state OCP and grid
generators after RCM, the banded path's limit and the block-size rule."""

import pytest

from pygradflow_amd import problems
from pygradflow_amd.sparse import MAX_BANDWIDTH, BandPlan, block_size_for


def _plan(prob, block=None):
    return BandPlan(prob.hess_sparse(), prob.jac_sparse(), prob.num_vars, prob.num_cons, block=block)


@pytest.mark.parametrize("args,bw", [((400, 8, 4), 22), ((400, 16, 8), 46), ((400, 20, 10), 58),
                                     ((400, 24, 8), 70)])
def test_multistate_ocp_bandwidth(args, bw):
    prob = problems.multistate_ocp(*args)
    T, nx, nu = args
    assert (prob.num_vars, prob.num_cons) == (T * (nx + nu), T * nx)
    plan = _plan(prob)
    assert plan.bw == bw
    assert plan.supported == (bw <= 64)


@pytest.mark.parametrize("W,L,bw", [(30, 500, 30), (40, 2000, 41)])
def test_grid_box_qp_bandwidth(W, L, bw):
    prob = problems.grid_box_qp(W, L)
    assert (prob.num_vars, prob.num_cons) == (W * L, 0)
    assert _plan(prob).bw == bw


def test_supported_up_to_64():
    assert MAX_BANDWIDTH == 64
    plan = _plan(problems.grid_box_qp(40, 60))
    assert plan.bw <= 64 and plan.supported
    assert not _plan(problems.multistate_ocp(50, 24, 8)).supported


@pytest.mark.parametrize("bw,B", [(0, 8), (8, 8), (9, 16), (10, 16), (11, 16), (16, 16), (17, 32),
                                  (32, 32), (33, 64), (64, 64), (65, None)])
def test_block_size_rule(bw, B):
    assert block_size_for(bw) == B


def test_every_supported_bandwidth_gets_a_cyclic_reduction():
    """No bandwidth of the banded path is left without a block size (there is no other route)."""
    for bw in range(MAX_BANDWIDTH + 1):
        assert block_size_for(bw) in (8, 16, 32, 64), bw


def test_block_size_of_plans():
    assert _plan(problems.multistate_ocp(100, 8, 4)).block_size == 32
    assert _plan(problems.multistate_ocp(100, 16, 8)).block_size == 64
    assert _plan(problems.sparse_ocp(300)).block_size == 8
    assert _plan(problems.multistate_ocp(100, 8, 4), block=64).block_size == 64
    with pytest.raises(ValueError):
        _plan(problems.multistate_ocp(10, 2, 1), block=24)
