"""The Globalized policy's line search restated in numpy, in the form the device computes it.

For a linear-quadratic problem the trial point (x - a dx, y - a dy) has c - a u and g - a v with
u = A dx and v = Q dx + A'(rho u + dy): one evaluation of (u, v) serves all 30 trials of the ladder
a = 2^-k, and the slope is F . [lamb dx + keep v ; lamb dy - u].  ``line_search`` is steps 3 to 6
of the reference's ``GlobalizedNewtonMethod.step`` (pygradflow/newton.py:250-299) written that
way; the fixtures ``tests/golden/globalized/glob_*.npz`` (tools/gen_golden_globalized.py) hold what the
reference itself computed, trial by trial, from fresh evaluations.  Also the fixtures' loader.
"""

import glob
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "globalized")
ACTIVE_EPS = 1e-8  # reference implicit_func.py:44
MAX_IT = 30
TOL = 1e-10  # the project's parity scale (golden_util.rel_err)


def case_names():
    return sorted(os.path.basename(p)[5:-4] for p in glob.glob(os.path.join(GOLDEN, "glob_*.npz")))


def load_case(name):
    return np.load(os.path.join(GOLDEN, f"glob_{name}.npz"), allow_pickle=False)


def build_problem(case, **attrs):
    from pygradflow_amd import problems as P

    spec = json.loads(str(case["problem"]))
    prob = getattr(P, spec["ctor"])(*spec["args"], **spec["kwargs"])
    for k, v in attrs.items():
        setattr(prob, k, v)
    return prob


def case_tau(case):
    tau = float(case["tau"])
    return None if np.isnan(tau) else tau


def scaled_residual(lamb, xhat, yhat, x, y, g, c, slb, sub):
    """ScaledImplicitFunc.value_at with the tau-less mask of its own point
    (implicit_func.py:219-231, 246); also that mask."""
    p = lamb * xhat - g
    act = (p < slb - ACTIVE_EPS) | (p > sub + ACTIVE_EPS)
    proj = np.where(act, np.minimum(np.maximum(p, slb), sub), p)
    fx = lamb * x - proj
    fy = -(lamb * y - (lamb * yhat + c))
    return np.concatenate([fx, fy]), act


def direction_images(problem, rho, dx, dy):
    A, Q = problem.jac_sparse(), problem.hess_sparse()
    u = A @ dx
    v = Q @ dx + A.T @ (rho * u + dy)
    return np.asarray(u).ravel(), np.asarray(v).ravel()


def line_search(problem, dt, rho, newton_tol, xhat, yhat, x, y, dx, dy):
    """dict(merit0, slope, merits (all 30), trials, alpha, failed, xn, yn, diff); ``trials`` 0 and
    no slope when merit0 <= newton_tol."""
    lamb = 1.0 / dt
    lb, ub = np.asarray(problem.var_lb, float), np.asarray(problem.var_ub, float)
    slb, sub = lamb * lb, lamb * ub
    A, Q = problem.jac_sparse(), problem.hess_sparse()
    c = np.asarray(A @ x - problem.b).ravel()
    g = np.asarray(Q @ x + problem.q + A.T @ (rho * c + y)).ravel()
    u, v = direction_images(problem, rho, dx, dy)
    F0, act = scaled_residual(lamb, xhat, yhat, x, y, g, c, slb, sub)
    merit0 = 0.5 * np.dot(F0, F0)
    slope = float(np.dot(F0, np.concatenate([lamb * dx + np.where(act, 0.0, v), lamb * dy - u])))
    merits = np.empty(MAX_IT)
    for k in range(MAX_IT):
        a = 0.5 ** k
        Fk, _ = scaled_residual(lamb, xhat, yhat, x - a * dx, y - a * dy, g - a * v, c - a * u, slb, sub)
        merits[k] = 0.5 * np.dot(Fk, Fk)
    out = dict(merit0=merit0, slope=slope, merits=merits, failed=False, alpha=1.0, trials=0)
    if not merit0 <= newton_tol:
        out["failed"], out["trials"] = True, MAX_IT
        for k in range(MAX_IT):
            a = 0.5 ** k
            if merits[k] <= newton_tol or merits[k] <= merit0 + 1e-4 * a * slope:
                out.update(failed=False, trials=k + 1, alpha=a)
                break
    if not out["failed"]:
        # StepResult(orig_iterate, alpha dx, alpha dy) (newton.py:296, step_solver.py:25-48)
        d = out["alpha"] * dx
        xn = xhat - d
        low, up = xn < lb, xn > ub
        xn[low], d[low] = lb[low], xhat[low] - lb[low]
        xn[up], d[up] = ub[up], xhat[up] - ub[up]
        ddy = out["alpha"] * dy
        out.update(xn=xn, yn=yhat - ddy, diff=float(np.sqrt(np.dot(d, d) + np.dot(ddy, ddy))))
    return out
