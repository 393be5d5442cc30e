"""CPU side of the device-assembled Standard / Extended / Asymmetric formulations: the numpy
yardstick (tests/unsym_ref.py) against the matrices recorded from the reference, and the
reference's ``linear_solver(mat)`` override point, which must keep receiving the host-assembled
matrix."""

import numpy as np
import pytest
import scipy.sparse as sps

from tests import golden_util as G
from tests import unsym_ref as R
from tests.test_formulations import KINDS, _OracleScaledFunc, _ScipyLU

from pygradflow_amd import unsym_step_solvers as U
from pygradflow_amd.iterate import Iterate
from pygradflow_amd.params import Params


def _first_step_derivs(case, kind):
    """(H, J) the reference linearised with at the first Full step."""
    problem = G.rebuild_problem(case)
    orig = Iterate(problem, Params(newton_type="Full"), case["x0"], case["y0"])
    rho = float(case["rho"])
    H = orig.aug_lag_deriv_xx(rho if kind == "Standard" else 0.0)
    J = orig.aug_lag_deriv_xy()
    dense = lambda a: a.toarray() if sps.issparse(a) else np.asarray(a)  # noqa: E731
    return dense(H), dense(J).reshape(int(case["m"]), int(case["n"]))


@pytest.mark.parametrize("name", G.formulation_case_names())
def test_numpy_helper_reproduces_recorded_matrices(name):
    case = G.load_case(name)
    dt, rho = float(case["dt"]), float(case["rho"])
    n, m = int(case["n"]), int(case["m"])
    assert n + m in (16, 64, 120)
    for kind in KINDS:
        pre = f"{kind}/Full/0/"
        mask = case[pre + "mask"]
        ref = case[pre + "deriv"]
        assert 5 <= int(mask.sum()) <= 29
        cond = np.linalg.cond(ref)
        assert 6 <= cond <= 13, (kind, cond)
        H, J = _first_step_derivs(case, kind)
        M = R.newton_matrix(kind, H, J, mask, dt, rho)
        assert G.rel_err(M, ref) <= 1e-14, kind


@pytest.mark.parametrize("kind,own_func", [(k, True) for k in KINDS] + [("Standard", False)])
def test_linear_solver_override_receives_host_matrix(kind, own_func):
    """A subclass that overrides ``linear_solver`` takes the host assembly and is handed the
    matrix.  (Extended / Asymmetric with the default ``_make_func`` own a device handle for the
    scaled residual: that combination is in the GPU tests.)"""
    case = G.load_case("formul_quartic_n12_m4")
    problem = G.rebuild_problem(case)
    dt, rho = float(case["dt"]), float(case["rho"])
    base = {"Standard": U.StandardStepSolver, "Extended": U.ExtendedStepSolver,
            "Asymmetric": U.AsymmetricStepSolver}[kind]
    seen = []

    class Sub(base):
        def linear_solver(self, mat):
            seen.append(mat)
            return _ScipyLU(mat)

        if own_func:
            def _make_func(self):
                return _OracleScaledFunc(self)

    params = Params(newton_type="Full")
    orig = Iterate(problem, params, case["x0"], case["y0"])
    sv = Sub(problem, params, orig, dt, rho)
    assert not sv._on_device
    mask = case[f"{kind}/Full/0/mask"]
    sv.update_active_set(mask)
    sv.update_derivs(orig)
    step = sv.solve(orig)
    assert len(seen) == 1 and sps.issparse(seen[0])
    assert G.rel_err(seen[0].toarray(), case[f"{kind}/Full/0/deriv"]) <= 1e-14
    assert G.rel_err(step.dx, case[f"{kind}/Full/0/dx"]) <= 1e-10


@pytest.mark.parametrize("kind,form", [("Standard", 1), ("Extended", 2), ("Asymmetric", 3)])
def test_default_classes_choose_the_device_path(monkeypatch, kind, form):
    """Without an override a class asks for a handle set to ITS formulation and forwards the
    stashed mask / derivatives to it; PGF_UNSYM_HOST=1 asks for a plain handle and stays on the
    host.  (The handle is a recording stand-in: no GPU here.)"""
    made = []

    class FakeDev:
        def __init__(self, problem, params, orig, dt, rho, device=0, formulation=0):
            self.problem, self.orig_iterate, self.dt = problem, orig, dt
            self.formulation, self.func, self.masks, self.resets = formulation, object(), [], 0
            made.append(self)

        def update_active_set(self, mask):
            self.masks.append(mask)

        def reset_deriv(self):
            self.resets += 1

        def close(self):
            pass

    monkeypatch.setattr(U, "HipStepSolver", FakeDev)
    case = G.load_case("formul_quartic_n12_m4")
    problem = G.rebuild_problem(case)
    params = Params(newton_type="Full")
    orig = Iterate(problem, params, case["x0"], case["y0"])
    cls = getattr(U, kind + "StepSolver")
    monkeypatch.delenv("PGF_UNSYM_HOST", raising=False)
    sv = cls(problem, params, orig, float(case["dt"]), float(case["rho"]))
    assert sv._on_device and made[-1].formulation == form
    mask = case[f"{kind}/Full/0/mask"]
    sv.update_active_set(mask)
    sv.update_derivs(orig)
    assert np.array_equal(made[-1].masks[-1], mask) and made[-1].resets == 1
    assert made[-1]._hess is sv.hess and made[-1]._jac is sv.jac
    monkeypatch.setenv("PGF_UNSYM_HOST", "1")
    sv = cls(problem, params, orig, float(case["dt"]), float(case["rho"]))
    assert not sv._on_device and made[-1].formulation == 0
    sv.update_active_set(mask)
    assert made[-1].masks == []
