#!/usr/bin/env python3
"""Banded path under the schedule switches (GPU), against the CPU oracle.  Run in a child process
by tests/test_gpu_schedules.py (the switches are read once per process).

Default: a sparse optimal-control problem (bw 6, N = 9000), a tridiagonal box QP with a churning
mask (bw 1, N = 4099), both on the 8 x 8 cyclic reduction, and three problems from the bw 9 .. 10
range on B = 16 (grid_box_qp(9, 320), N = 2880, and multistate_ocp(400, 4, 2), N = 4000: both bw 10
after RCM; grid_box_qp(9, 500), N = 4500, bw 9).

--sweep: the block-count sweep of tests/test_band_narrow_gpu.py (band_util.SWEEP_BOX, SWEEP_OCP)
through the 8 x 8 reduction, Full x 2 + Simplified x 1 (PGF_BCR_PAIRS, PGF_BCR_FUSED,
PGF_BCR_PAIR_MAX), with a line "plan <name> nb <nb>: <levels> tail <blocks>" per problem: the launch
plan the switches in the environment give that block count (band_util.bcr_launch_plan, the
arithmetic of sp_launch_bcr_solve restated on the host), which the parent test checks, so that a
variant cannot quietly run the same plan as another.

Prints "route <name> bw <bw>: <route>" per problem, the route read from the plan's block size,
and (default mode) checked against the library: the guarded cyclic reductions leave a residual in
pgf_refinement_stats."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pygradflow_amd as pgf  # noqa: E402
from pygradflow_amd import problems  # noqa: E402
from oracle import newton_oracle as O  # noqa: E402  (test infrastructure: the checker)
from tests.band_util import SWEEP_BOX, SWEEP_OCP, bcr_launch_plan_from_env, plan_of  # noqa: E402


def rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1.0, np.max(np.abs(b)))) if a.size else 0.0


def route_of(prob):
    """Which solve the library runs for the problem: the cyclic reduction of the plan's block size."""
    plan = plan_of(prob)
    return plan.bw, f"bcr{plan.block_size}"


def check(name, prob, policies, want_bw=None, residual_tells=False):
    prob.pgf_force_band = True
    n, m = prob.num_vars, prob.num_cons
    bw, route = route_of(prob)
    assert want_bw is None or bw in want_bw, (name, bw)
    x0, y0 = np.zeros(n), np.zeros(m)
    worst = 0.0
    for pol, steps in policies:
        recs = O.NewtonOracle(prob, pol, x0, y0, 1.0, 1.0).run(x0, y0, steps)
        dn = pgf.DeviceNewton(prob, pol, x0, y0, 1.0, 1.0)
        assert dn.sparse
        for k, rec in enumerate(recs):
            diff, n_neg = dn.step()
            x, y = dn.point()
            assert np.array_equal(dn.mask(), rec["mask"]), (name, pol, k)
            e = max(rel(x, rec["xn"]), rel(y, rec["yn"]))
            worst = max(worst, e)
            assert e <= 1e-10, (name, pol, k, e)
            assert n_neg == m, (name, pol, k, n_neg)
        if residual_tells:
            # what the library itself says about the route: every cyclic reduction records a
            # residual per step (never exactly 0 at these sizes; the handle's initial value is 0)
            last_rel = dn.refinement_stats()[2]
            assert last_rel != 0.0, (name, route, last_rel)
        dn.close()
    print(f"route {name} bw {bw}: {route}", flush=True)
    print(f"{name}: ok", flush=True)
    return worst


worst = 0.0
if "--sweep" in sys.argv[1:]:
    cases = [(f"box{n}", problems.box_qp(n, seed=n)) for n in SWEEP_BOX]
    cases += [(f"ocp{m}", problems.sparse_ocp(m, seed=m)) for m in SWEEP_OCP]
    for name, prob in cases:
        worst = max(worst, check(name, prob, (("Full", 2), ("Simplified", 1)), want_bw=range(0, 9)))
        nb = (prob.num_vars + prob.num_cons + 7) // 8
        levels, tail = bcr_launch_plan_from_env(nb, os.environ)
        print(f"plan {name} nb {nb}:", " ".join(f"{k}@{st}" for k, st in levels) or "--", "tail", tail, flush=True)
    print("band sweep ok, worst", worst, flush=True)
else:
    long = (("Full", 4), ("Simplified", 3))
    worst = max(worst, check("ocp", problems.sparse_ocp(3000, seed=1), long, want_bw=(6,), residual_tells=True))
    worst = max(worst, check("box", problems.box_qp(4099, seed=2), long, want_bw=(1,), residual_tells=True))
    worst = max(worst, check("grid320", problems.grid_box_qp(9, 320), long, want_bw=(9, 10), residual_tells=True))
    worst = max(worst, check("mocp10", problems.multistate_ocp(400, 4, 2), long, want_bw=(9, 10), residual_tells=True))
    worst = max(worst, check("grid9x500", problems.grid_box_qp(9, 500, seed=3), long, want_bw=(9,), residual_tells=True))
    print("band ok, worst", worst, flush=True)
