"""The one-launch formulation of the Globalized line search against the reference (CPU).

``line_search_ref.line_search`` computes every trial merit from ONE evaluation of the direction's
images (g - a v, c - a u) instead of evaluating g and c afresh at each trial point.  Replayed over
every fixture from the recorded x, y, dx, dy: the accepted k and the failures must be EQUAL to the
reference's, merit0, slope and every trial merit within 1e-10 max(1, merit0)."""

import numpy as np
import pytest

from tests import line_search_ref as R
from tests.golden_util import rel_err


def test_fixtures_cover_the_listed_cases():
    names = R.case_names()
    assert len(names) == 14
    counts = {}
    for name in names:
        case = R.load_case(name)
        counts[name] = [-1 if bool(case[f"{k}/failed"]) else int(case[f"{k}/trials"])
                        for k in range(int(case["steps"]))]
    assert counts["box_qp_n64_dt100"] == [3, 7, 3, 7, 3]
    assert counts["dense_qp_n24_m6"] == [1, 10, 1, 10, 1]
    assert counts["dense_qp_n40_m10_fail"] == [1, 6, 1, -1]
    assert counts["sparse_ocp_m20"] == [1, 0, 0]
    assert counts["budget_box_qp_n300"] == [5, 6, 2]


@pytest.mark.parametrize("name", R.case_names())
def test_linearised_ladder_matches_reference(name):
    case = R.load_case(name)
    prob = R.build_problem(case)
    dt, rho, tol = float(case["dt"]), float(case["rho"]), float(case["newton_tol"])
    xhat, yhat = case["x0"], case["y0"]
    for k in range(int(case["steps"])):
        pre = f"{k}/"
        got = R.line_search(prob, dt, rho, tol, xhat, yhat, case[pre + "x"], case[pre + "y"],
                            case[pre + "dx"], case[pre + "dy"])
        merit0 = float(case[pre + "merit0"])
        scale = 1e-10 * max(1.0, merit0)
        failed, trials = bool(case[pre + "failed"]), int(case[pre + "trials"])
        print(name, k, "trials", got["trials"], "merit0 diff", abs(got["merit0"] - merit0))
        assert got["failed"] == failed
        assert got["trials"] == trials
        assert abs(got["merit0"] - merit0) <= scale
        if trials:
            assert abs(got["slope"] - float(case[pre + "slope"])) <= scale
            assert np.max(np.abs(got["merits"][:trials] - case[pre + "merits"])) <= scale
        if not failed:
            assert got["alpha"] == float(case[pre + "alpha"])
            assert rel_err(got["xn"], case[pre + "xn"]) <= R.TOL
            assert rel_err(got["yn"], case[pre + "yn"]) <= R.TOL
