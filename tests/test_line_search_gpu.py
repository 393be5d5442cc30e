"""The Globalized policy on the device (GPU): ``DeviceNewton(problem, "Globalized", ...)`` against
the reference's own steps (tests/golden/globalized/glob_*.npz, tools/gen_golden_globalized.py) on every route
-- dense, narrow band, wide band, bordered band --, the failure path, ``tau``, the refusals and
the host synchronisations of a step, which must not grow with its trial count."""

import math

import numpy as np
import pytest

from tests import line_search_ref as R
from tests.golden_util import rel_err

pytestmark = pytest.mark.gpu

TOL = R.TOL


def _routes(name):
    if name.startswith("box_qp"):
        return ["dense", "band"]
    if name.startswith("dense_qp"):
        return ["dense"]
    if name.startswith("budget_box_qp"):
        return ["border"]
    return ["band"]  # multistate_ocp: wide blocks; sparse_ocp: narrow, m > 0


CASES = [(name, route) for name in R.case_names() for route in _routes(name)]
_runs = {}


def _problem(case, route):
    attrs = {}
    if route == "band":
        attrs["pgf_force_band"] = True
    if route == "border":
        attrs["pgf_border"] = "auto"
    return R.build_problem(case, **attrs)


def _run(name, route):
    """Every step of the fixture on the device, once per (case, route): per step the point before,
    the mask, the direction, the line search's stats, the point after and the counters; after a
    failed step also a Full step on the same handle."""
    if (name, route) in _runs:
        return _runs[(name, route)]
    import pygradflow_amd as pgf
    from pygradflow_amd.errors import LineSearchError, StepSolverError

    case = R.load_case(name)
    prob = _problem(case, route)
    dn = pgf.DeviceNewton(prob, "Globalized", case["x0"], case["y0"], float(case["dt"]), float(case["rho"]),
                          tau=R.case_tau(case), newton_tol=float(case["newton_tol"]))
    rec = dict(sparse=dn.sparse, steps=[])
    if dn.sparse:
        rec["block"] = int(dn._hd.plan.block_size)
    try:
        for k in range(int(case["steps"])):
            before = dn.point()
            s0 = dn.step_stats()
            failed, diff = False, math.nan
            try:
                diff, _ = dn.step()
            except LineSearchError as e:
                assert not isinstance(e, StepSolverError)
                assert str(e) == "Line search failed to converge"
                failed = True
            s1 = dn.step_stats()
            rec["steps"].append(dict(before=before, after=dn.point(), mask=dn.mask(), failed=failed, diff=diff,
                                     direction=dn.direction(), ls=dn.line_search(),
                                     syncs=s1[0] - s0[0], redone=s1[1] - s0[1]))
        if rec["steps"][-1]["failed"]:
            dn.kind = "Full"  # the same handle, the same outer step
            dn.step()
            rec["full"] = dict(point=dn.point(), mask=dn.mask())
        rec["border"] = dn.border_stats()[0] if dn.sparse else 0
    finally:
        dn.close()
    _runs[(name, route)] = rec
    return rec


def test_routes_are_the_ones_named():
    assert not _run("box_qp_n64_dt1", "dense")["sparse"]
    band = _run("box_qp_n64_dt1", "band")
    assert band["sparse"] and band["block"] == 8 and band["border"] == 0
    wide = _run("multistate_ocp_fail", "band")
    assert wide["sparse"] and wide["block"] >= 16
    assert _run("budget_box_qp_n300", "border")["border"] >= 1


@pytest.mark.parametrize("name,route", CASES)
def test_steps_match_reference(name, route):
    case = R.load_case(name)
    rec = _run(name, route)
    assert len(rec["steps"]) == int(case["steps"])
    xhat, yhat = case["x0"], case["y0"]
    for k, st in enumerate(rec["steps"]):
        pre = f"{k}/"
        merit0 = float(case[pre + "merit0"])
        scale = 1e-10 * max(1.0, merit0)
        failed, trials = bool(case[pre + "failed"]), int(case[pre + "trials"])
        ls = st["ls"]
        ref_merits = case[pre + "merits"]
        err_m = float(np.max(np.abs(ls["trial_merits"][:trials] - ref_merits))) if trials else 0.0
        print(name, route, k, "trials", ls["trials"], "alpha", ls["alpha"], "merit0 err", abs(ls["merit0"] - merit0),
              "merit err", err_m, "dx err", rel_err(st["direction"][0], case[pre + "dx"]))
        assert rel_err(st["before"][0], case[pre + "x"]) <= TOL
        assert rel_err(st["before"][1], case[pre + "y"]) <= TOL
        assert np.array_equal(st["mask"], case[pre + "mask"])
        assert rel_err(st["direction"][0], case[pre + "dx"]) <= TOL
        assert rel_err(st["direction"][1], case[pre + "dy"]) <= TOL
        assert st["failed"] == failed
        assert ls["trials"] == trials
        assert abs(ls["merit0"] - merit0) <= scale
        if trials:
            assert abs(ls["slope"] - float(case[pre + "slope"])) <= scale
            assert err_m <= scale
        if failed:
            assert trials == 30
            # the point has not moved: bit for bit
            assert st["after"][0].tobytes() == st["before"][0].tobytes()
            assert st["after"][1].tobytes() == st["before"][1].tobytes()
            continue
        assert ls["alpha"] == float(case[pre + "alpha"])
        assert rel_err(st["after"][0], case[pre + "xn"]) <= TOL
        assert rel_err(st["after"][1], case[pre + "yn"]) <= TOL
        # the reported length: of (dx rewritten where clipped, alpha dy), measured from the outer point
        want = float(np.sqrt(np.sum((xhat - case[pre + "xn"]) ** 2) + np.sum((yhat - case[pre + "yn"]) ** 2)))
        assert abs(st["diff"] - want) <= TOL * max(1.0, want)
    if rec["steps"][-1]["failed"]:
        # the handle after a failed line search: a Full step from the same point matches its golden
        assert rel_err(rec["full"]["point"][0], case["full/xn"]) <= TOL
        assert rel_err(rec["full"]["point"][1], case["full/yn"]) <= TOL


@pytest.mark.parametrize("name", [n for n in R.case_names() if n.startswith("box_qp")])
def test_dense_and_band_agree(name):
    dense, band = _run(name, "dense"), _run(name, "band")
    for a, b in zip(dense["steps"], band["steps"]):
        assert a["failed"] == b["failed"] and a["ls"]["trials"] == b["ls"]["trials"]
        assert a["ls"]["alpha"] == b["ls"]["alpha"]
        assert np.array_equal(a["mask"], b["mask"])
        assert rel_err(a["after"][0], b["after"][0]) <= TOL
        assert rel_err(a["ls"]["trial_merits"], b["ls"]["trial_merits"]) <= TOL


def test_tau_case_uses_tau_less_masks_for_the_merit():
    """box_qp(64), dt = 10, tau = 0.05: one accepted step, then a failure.  The step's mask is the
    tau one; the recorded merits are the reference's value_at(iterate, rho), which takes no tau."""
    case = R.load_case("box_qp_n64_dt10_tau")
    assert R.case_tau(case) == 0.05
    rec = _run("box_qp_n64_dt10_tau", "dense")
    assert [s["failed"] for s in rec["steps"]] == [False, True]
    st = rec["steps"][1]
    assert np.max(np.abs(st["ls"]["trial_merits"] - case["1/merits"])) <= 1e-10 * max(1.0, float(case["1/merit0"]))


def test_host_syncs_do_not_grow_with_the_trial_count():
    """dense_qp(24, 6): trials 1, 10, 1, 10, 1.  The line search is one launch and one wait whatever
    k is accepted: a 10-trial step costs no more host synchronisations than the 1-trial steps of
    the same run (a redone speculative step's extra wait counted apart)."""
    rec = _run("dense_qp_n24_m6", "dense")
    trials = [s["ls"]["trials"] for s in rec["steps"]]
    assert trials == [1, 10, 1, 10, 1]
    cost = [s["syncs"] - s["redone"] for s in rec["steps"]]
    print("host syncs", [s["syncs"] for s in rec["steps"]], "redone", [s["redone"] for s in rec["steps"]])
    ones = [c for c, t in zip(cost, trials) if t == 1]
    for c, t in zip(cost, trials):
        if t == 10:
            assert c <= min(ones)
    assert min(cost) >= 2  # the step's status block, then the line search's block


def test_refusals():
    import pygradflow_amd as pgf
    from pygradflow_amd import _lib, problems

    prob = problems.dense_qp(24, 6, seed=1, boxed_frac=1.0, box=0.05)
    x0, y0 = np.zeros(24), np.zeros(6)
    # an unsymmetric formulation
    dn = pgf.DeviceNewton(prob, "Globalized", x0, y0, 1.0, 1.0, step_solver_type="Standard")
    try:
        with pytest.raises(ValueError, match="Symmetric"):
            dn.step()
    finally:
        dn.close()
    # the bit without its two companions
    dn = pgf.DeviceNewton(prob, "Globalized", x0, y0, 1.0, 1.0)
    try:
        h, lib = dn._hd.h, dn._lib
        for bits in (_lib.STEP_LINE_SEARCH, _lib.STEP_LINE_SEARCH | _lib.STEP_RECOMPUTE_MASK,
                     _lib.STEP_LINE_SEARCH | _lib.STEP_RECOMPUTE_MASK | _lib.STEP_REFACTOR_ON_CHANGE):
            assert lib.pgf_qp_step(h, bits, math.nan, 0, None, None) == _lib.PGF_INVALID
            assert lib.pgf_qp_step_async(h, bits, math.nan) == _lib.PGF_INVALID
        diff, _ = dn.step()  # and the handle serves the policy afterwards
        assert diff > 0.0 and dn.line_search()["trials"] == 1
    finally:
        dn.close()
    # a device batch
    from pygradflow_amd.batched import BatchedDeviceNewton

    with pytest.raises(NotImplementedError, match="Globalized"):
        BatchedDeviceNewton(lambda i: prob, 2, "Globalized", 1.0, 1.0)
    seq = BatchedDeviceNewton(lambda i: prob, 2, "Globalized", 1.0, 1.0, sequential=True)
    assert [s.kind for s in seq.solvers] == ["Globalized", "Globalized"]
    for s in seq.solvers:
        s.close()
