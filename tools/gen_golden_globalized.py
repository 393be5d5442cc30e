#!/usr/bin/env python3
"""Generate the golden vectors of the Globalized policy FROM THE REFERENCE.

In the pattern of ``tools/gen_golden.py``: runs only where the reference is importable
(``PGF_REFERENCE``; nothing from it is copied), drives ``GlobalizedNewtonMethod.step``
(reference ``pygradflow/newton.py:218-304``) from x0 = 0, y0 = 0 with rho = 1 on the problems of
``pygradflow_amd.problems`` and stores, per Newton step, what the line search saw and decided.
``tests/golden/globalized/glob_*.npz`` hold arrays and one JSON string (the problem's constructor call); the
tests build the problem again from it.

Per step ``k``: ``k/x, k/y`` the point; ``k/dx, k/dy`` the full direction (the step solver's, at
the OUTER point); ``k/mask`` the mask ``_set_iterate`` set; ``k/merit0``; ``k/slope`` (absent when
merit0 <= newton_tol: the reference does not form it); ``k/merits`` every trial merit in order;
``k/trials``; ``k/alpha``; ``k/xn, k/yn``; ``k/failed``.  After a failed step: ``full/xn, full/yn``,
the reference's Full step from the same point (the handle must still serve it).

The script ASSERTS that no recorded decision is within rounding of flipping: every trial merit of
an accepted step is at least 1e-6 merit0 away from the Armijo bound and 1e-3 (relative) away from
newton_tol, and so is merit0 from newton_tol.  In a FAILED step trial merit and bound both tend to
merit0 as alpha = 2^-k shrinks, so their gap shrinks with alpha and no fixed fraction of merit0 can
hold for k near 29 (the cases' own gaps reach 1e-10 merit0 there).  What can differ between two
correct evaluations of a merit is the rounding of a sum of n + m squares whose terms carry a few
roundings each, below 8 (n + m) 2^-53 merit0 < 1e-13 merit0 for the failing cases (n + m <= 120):
a failed step's gap must be at least 1e-11 merit0, a hundred times that.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_globalized.py
"""

import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("PGF_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
sys.path.insert(0, REPO)
sys.path.append(os.path.join(REPO, "tools", "_stubs"))  # cosmetic termcolor stand-in

from pygradflow.iterate import Iterate  # noqa: E402  (reference)
from pygradflow.newton import newton_method  # noqa: E402
from pygradflow.params import NewtonType, Params  # noqa: E402

from pygradflow_amd import problems as P  # noqa: E402  (ours; duck-typed)

# (a directory of their own: tests/golden_util.case_names takes every tests/golden/*.npz without a
# known prefix for a case of tools/gen_golden.py)
OUT = os.path.join(REPO, "tests", "golden", "globalized")
MAX_IT = 30

# name -> (constructor, args, kwargs, dt, steps, tau, the trials per step the reference is known to
# take: -1 a failed search, None not pinned); asserted, so a changed reference or problem shows
CASES = {
    "box_qp_n64_dt1": ("box_qp", [64], {}, 1.0, 5, None, [2, 3, 2, 3, 2]),
    "box_qp_n64_dt100": ("box_qp", [64], {}, 100.0, 5, None, [3, 7, 3, 7, 3]),
    "box_qp_n300_dt10": ("box_qp", [300], {}, 10.0, 4, None, [3, 6, 3, 5]),
    "box_qp_n513_dt1": ("box_qp", [513], {}, 1.0, 4, None, [2, 4, 2, 4]),
    "dense_qp_n24_m6": ("dense_qp", [24, 6], dict(seed=1, boxed_frac=1.0, box=0.05), 1.0, 5, None,
                        [1, 10, 1, 10, 1]),
    "dense_qp_n250_m9_s2": ("dense_qp", [250, 9], dict(seed=2, boxed_frac=1.0, box=0.2), 10.0, 4, None,
                            [1, 4, 1, 5]),
    "dense_qp_n250_m9_s3": ("dense_qp", [250, 9], dict(seed=3, boxed_frac=1.0, box=0.05), 10.0, 4, None,
                            [1, 10, 1, 10]),
    "dense_qp_n40_m10_fail": ("dense_qp", [40, 10], dict(seed=2, boxed_frac=1.0, box=0.1), 1.0, 4, None,
                              [1, 6, 1, -1]),
    "dense_qp_n96_m24_fail": ("dense_qp", [96, 24], dict(seed=1, boxed_frac=0.25), 1.0, 2, None, [1, -1]),
    "budget_box_qp_n300": ("budget_box_qp", [300], {}, 10.0, 3, None, [5, 6, 2]),
    "budget_box_qp_n64_fail": ("budget_box_qp", [64], {}, 10.0, 2, None, [2, -1]),
    "multistate_ocp_fail": ("multistate_ocp", [6, 8, 4], dict(ubound=0.05), 1.0, 2, None, [1, -1]),
    "sparse_ocp_m20": ("sparse_ocp", [20], {}, 1.0, 3, None, [1, 0, 0]),
    "box_qp_n64_dt10_tau": ("box_qp", [64], {}, 10.0, 2, 0.05, [None, -1]),
}


def _check_margins(name, k, merit0, slope, merits, tol, failed):
    """No decision may hinge on the last digits: returns the smallest relative Armijo margin."""
    assert abs(merit0 / tol - 1.0) >= 1e-3, (name, k, "merit0 at newton_tol", merit0)
    worst = np.inf
    for j, tm in enumerate(merits):
        alpha = 0.5 ** j
        assert abs(tm / tol - 1.0) >= 1e-3, (name, k, j, "trial merit at newton_tol", tm)
        gap = abs(tm - (merit0 + 1e-4 * alpha * slope))
        if failed:
            assert gap >= 1e-11 * merit0, (name, k, j, "failed step's trial at the Armijo bound", gap / merit0)
            continue
        assert gap >= 1e-6 * merit0, (name, k, j, "trial merit at the Armijo bound", gap / merit0)
        worst = min(worst, gap / merit0)
    return worst


def run_case(name, ctor, args, kwargs, dt, steps, tau, expect):
    problem = getattr(P, ctor)(*args, **kwargs)
    n, m = problem.num_vars, problem.num_cons
    rho = 1.0
    kw = dict(active_set_type="Explicit", active_set_tau=tau) if tau is not None else {}
    params = Params(newton_type=NewtonType.Globalized, **kw)
    tol = params.newton_tol
    x0, y0 = np.zeros(n), np.zeros(m)
    orig = Iterate(problem, params, x0, y0)
    method = newton_method(problem, params, orig, dt, rho, tau)
    func, solver = method.func, method.step_solver

    rec = {}
    value_at, solve, update_active_set = func.value_at, solver.solve, solver.update_active_set

    def value_at_rec(iterate, rho_, active_set=None):
        val = value_at(iterate, rho_, active_set)
        if active_set is None:  # (the line search's calls: its merits)
            rec["values"].append(val)
        return val

    def solve_rec(iterate):
        res = solve(iterate)
        rec["full"] = res
        return res

    def update_rec(mask):
        rec["mask"] = np.array(mask, dtype=bool)
        return update_active_set(mask)

    func.value_at, solver.solve, solver.update_active_set = value_at_rec, solve_rec, update_rec

    out = dict(
        problem=json.dumps(dict(ctor=ctor, args=args, kwargs=kwargs)),
        n=n, m=m, dt=dt, rho=rho, tau=np.nan if tau is None else tau, newton_tol=tol, x0=x0, y0=y0,
    )
    it = orig
    counts, worst = [], np.inf
    for k in range(steps):
        rec.clear()
        rec["values"] = []
        failed = False
        try:
            step = method.step(it)
        except Exception as e:  # the reference raises a bare Exception
            assert str(e) == "Line search failed to converge", e
            failed = True
        full = rec["full"]
        merits = np.array([0.5 * np.dot(v, v) for v in rec["values"]])
        merit0, trial_merits = merits[0], merits[1:]
        pre = f"{k}/"
        out[pre + "x"], out[pre + "y"] = it.x, it.y
        out[pre + "dx"], out[pre + "dy"] = full.dx, full.dy
        out[pre + "mask"] = rec["mask"]
        out[pre + "merit0"] = merit0
        out[pre + "merits"] = trial_merits
        out[pre + "trials"] = len(trial_merits)
        out[pre + "failed"] = failed
        if merit0 <= tol:
            assert len(trial_merits) == 0 and not failed
            assert abs(merit0 / tol - 1.0) >= 1e-3
            alpha = 1.0
        else:
            # the slope as the reference forms it (newton.py:260-268), from deriv_at
            func.value_at = value_at
            grad = func.deriv_at(it, rho).T @ rec["values"][0]
            func.value_at = value_at_rec
            slope = float(np.dot(grad[:n], full.dx) + np.dot(grad[n:], full.dy))
            out[pre + "slope"] = slope
            worst = min(worst, _check_margins(name, k, merit0, slope, trial_merits, tol, failed))
            alpha = 0.5 ** (len(trial_merits) - 1)
            if failed:
                assert len(trial_merits) == MAX_IT
        counts.append(-1 if failed else len(trial_merits))
        if failed:
            # the reference's Full step from the same point, same outer step
            fparams = Params(newton_type=NewtonType.Full, **kw)
            forig = Iterate(problem, fparams, x0, y0)
            fit = Iterate(problem, fparams, it.x, it.y)
            fstep = newton_method(problem, fparams, forig, dt, rho, tau).step(fit)
            out["full/xn"], out["full/yn"] = fstep.iterate.x, fstep.iterate.y
            out["full/mask"] = np.asarray(fstep.active_set, dtype=bool)
            out["steps"] = k + 1
            break
        out[pre + "alpha"] = alpha
        out[pre + "xn"], out[pre + "yn"] = step.iterate.x, step.iterate.y
        it = step.iterate
    else:
        out["steps"] = steps
    want = [c for c in expect]
    if None not in want:
        assert counts == want, (name, counts, want)
    else:
        assert counts[-1] == -1 and len(counts) == len(want), (name, counts)
    path = os.path.join(OUT, f"glob_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{name}: trials {counts}, smallest relative Armijo margin {worst:.2e}, "
          f"{os.path.getsize(path)} bytes")


def main():
    os.makedirs(OUT, exist_ok=True)
    for name, (ctor, args, kwargs, dt, steps, tau, expect) in CASES.items():
        run_case(name, ctor, args, kwargs, dt, steps, tau, expect)


if __name__ == "__main__":
    main()
