"""The Standard / Extended / Asymmetric formulations assembled, factorised and solved on the
device (``pgf_set_formulation``, csrc/pgf_unsym.hip): matrices against the reference's recorded
ones and the numpy yardstick (tests/unsym_ref.py), the plugin classes and ``DeviceNewton`` against
recorded trajectories and the oracle, and the proof that no (n + m)^2 matrix crosses PCIe
(``pgf_debug_unsym_stats``).  Tolerances are those of tests/test_formulations.py."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sps

from oracle import newton_oracle as O
from tests import golden_util as G
from tests import unsym_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-10
KINDS = ("Standard", "Extended", "Asymmetric")
FORM = {"Standard": 1, "Extended": 2, "Asymmetric": 3}
POLICIES = ("Simplified", "Full", "ActiveSet")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dense(a):
    return np.ascontiguousarray(a.toarray() if sps.issparse(a) else a, dtype=np.float64)


class _Raw:
    """A bare C-ABI handle set up for one formulation."""

    def __init__(self, n, m, lb, ub, xhat, yhat, dt, rho, form, sparse=False):
        from pygradflow_amd import _lib

        self.L, self.lib = _lib, _lib.load()
        _lib.require_gpu()
        self.n, self.m = n, m
        self.h = C.c_void_p()
        _lib.check(self.lib.pgf_create(n, m, 0, 1 if sparse else 0, C.byref(self.h)), None, "create")
        self.ck(self.lib.pgf_set_bounds(self.h, _lib.dptr(_lib.as_f64(lb)), _lib.dptr(_lib.as_f64(ub))))
        self.ck(self.lib.pgf_set_outer(self.h, _lib.dptr(_lib.as_f64(xhat)), _lib.dptr(_lib.as_f64(yhat)),
                                       float(dt), float(rho)))
        if form is not None:
            self.ck(self.lib.pgf_set_formulation(self.h, form))

    def ck(self, rc):
        self.L.check(rc, self.h)

    def derivs(self, H, J):
        H = _dense(H).reshape(self.n, self.n)
        J = _dense(J).reshape(self.m, self.n)
        self.ck(self.lib.pgf_set_derivs_dense(
            self.h, H.ctypes.data_as(C.c_void_p) if self.n else None, max(self.n, 1),
            J.ctypes.data_as(C.c_void_p) if self.m and self.n else None, max(self.n, 1), 0))

    def mask(self, mask):
        mk = np.ascontiguousarray(mask, dtype=np.bool_)
        self.ck(self.lib.pgf_set_active_set(self.h, self.L.u8ptr(mk)))

    def matrix(self):
        N = self.n + self.m
        M = np.full((N, N), np.nan)
        self.ck(self.lib.pgf_get_newton_matrix(self.h, self.L.dptr(M), N))
        return M

    def residual(self, x, y, g, c, mask):
        L = self.L
        out = np.empty(self.n + self.m)
        mk = np.ascontiguousarray(mask, dtype=np.bool_)
        self.ck(self.lib.pgf_residual(self.h, L.dptr(L.as_f64(x)), L.dptr(L.as_f64(y)), L.dptr(L.as_f64(g)),
                                      L.dptr(L.as_f64(c)), L.u8ptr(mk), L.dptr(out)))
        return out

    def close(self):
        self.lib.pgf_destroy(self.h)


# ---- 1. matrix and residual parity with the reference's recorded first step -----------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", G.formulation_case_names())
def test_device_matrix_and_residual_equal_reference(pgf, name, kind):
    case = G.load_case(name)
    problem = G.rebuild_problem(case)
    dt, rho = float(case["dt"]), float(case["rho"])
    n, m = int(case["n"]), int(case["m"])
    orig = pgf.Iterate(problem, pgf.Params(newton_type="Full"), case["x0"], case["y0"])
    pre = f"{kind}/Full/0/"
    mask = case[pre + "mask"]
    raw = _Raw(n, m, problem.var_lb, problem.var_ub, case["x0"], case["y0"], dt, rho, FORM[kind])
    try:
        raw.derivs(orig.aug_lag_deriv_xx(rho if kind == "Standard" else 0.0), orig.aug_lag_deriv_xy())
        raw.mask(mask)
        M = raw.matrix()
        err = G.rel_err(M, case[pre + "deriv"])
        print(f"{name} {kind}: matrix rel err {err:.3e}")
        assert err <= 1e-14
        F = raw.residual(orig.x, orig.y, orig.aug_lag_deriv_x(rho), orig.aug_lag_deriv_y(), mask)
        ferr = G.rel_err(F, case[pre + "F"])
        print(f"{name} {kind}: residual rel err {ferr:.3e}")
        assert ferr <= 1e-13
    finally:
        raw.close()


# ---- 2. shapes: tile edges, m = 0, |A| = 0, |A| = n -----------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,m", [(1, 0), (31, 2), (33, 31), (65, 0), (100, 57), (257, 129)])
def test_device_matrix_shapes_against_numpy(pgf, n, m, kind):
    rng = np.random.default_rng(1000 * n + m)
    S = rng.standard_normal((n, n))
    H = S + S.T
    # only the lower triangle of the uploaded H is valid: NaN above the diagonal must never be read
    H_up = np.where(np.triu(np.ones((n, n), dtype=bool), 1), np.nan, H)
    J = rng.standard_normal((m, n))
    dt, rho = 0.7, 1.3
    inf = np.full(n, np.inf)
    raw = _Raw(n, m, -inf, inf, np.zeros(n), np.zeros(m), dt, rho, FORM[kind])
    try:
        raw.derivs(H_up, J)
        half = np.zeros(n, dtype=bool)
        half[rng.permutation(n)[: n // 2]] = True
        for label, mask in (("none", np.zeros(n, dtype=bool)), ("all", np.ones(n, dtype=bool)),
                            ("half", half)):
            raw.mask(mask)
            M = raw.matrix()
            ref = R.newton_matrix(kind, H, J, mask, dt, rho)
            assert np.isfinite(M).all(), (label, "entries left unwritten")
            err = G.rel_err(M, ref)
            nbits = int(np.count_nonzero(M != ref))
            print(f"n={n} m={m} {kind} {label}: rel err {err:.3e}, entries not bit-equal: {nbits}")
            assert err <= 1e-14, label
    finally:
        raw.close()


# ---- 3. plugin path ---------------------------------------------------------------------------
def replay_plugin(pgf, name):
    """Every kind x policy of a recorded case through the product classes; returns the
    ``unsym_stats`` of every solver used."""
    from pygradflow_amd.newton import newton_method

    case = G.load_case(name)
    problem = G.rebuild_problem(case)
    dt, rho, tau = float(case["dt"]), float(case["rho"]), G.case_tau(case)
    stats = []
    for kind in KINDS:
        for pol in case["policies"]:
            params = pgf.Params(newton_type=str(pol), step_solver_type=kind)
            orig = pgf.Iterate(problem, params, case["x0"], case["y0"])
            method = newton_method(problem, params, orig, dt, rho, tau)
            curr = orig
            for k in range(int(case["steps"])):
                step = method.step(curr)
                curr = step.iterate
                pre = f"{kind}/{pol}/{k}/"
                assert np.array_equal(step.active_set, case[pre + "mask"]), (kind, pol, k)
                assert G.rel_err(step.dx, case[pre + "dx"]) <= TOL, (kind, pol, k)
                assert G.rel_err(step.dy, case[pre + "dy"]) <= TOL, (kind, pol, k)
                assert G.rel_err(step.iterate.x, case[pre + "xn"]) <= TOL, (kind, pol, k)
                assert G.rel_err(step.iterate.y, case[pre + "yn"]) <= TOL, (kind, pol, k)
                assert abs(step.diff - float(case[pre + "diff"])) <= TOL * max(1.0, step.diff)
            stats.append((kind, str(pol), method.step_solver.unsym_stats()))
            method.step_solver.close()
    return stats


@pytest.mark.parametrize("name", G.formulation_case_names())
def test_plugin_classes_run_on_the_device(pgf, name, monkeypatch):
    monkeypatch.delenv("PGF_UNSYM_HOST", raising=False)
    for kind, pol, (asm, lu, nbytes) in replay_plugin(pgf, name):
        assert asm >= 1 and lu >= 1, (kind, pol, asm, lu)
        assert nbytes == 0, (kind, pol, nbytes)


_CHILD = """
import sys
sys.path.insert(0, {repo!r})
import pygradflow_amd as pgf
from tests.test_unsym_device_gpu import replay_plugin
for kind, pol, (asm, lu, nbytes) in replay_plugin(pgf, {name!r}):
    assert nbytes > 0, (kind, pol, nbytes)
print("host path ok")
"""


@pytest.mark.parametrize("name", G.formulation_case_names())
def test_plugin_classes_host_path_when_forced(name):
    """PGF_UNSYM_HOST=1 (a child process: the switch is read per solver, the pooled handles'
    counters are per process): the same replay passes and the matrices are counted."""
    env = dict(os.environ, PGF_UNSYM_HOST="1")
    res = subprocess.run([sys.executable, "-c", _CHILD.format(repo=REPO, name=name)], env=env,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "host path ok" in res.stdout


# ---- 4. DeviceNewton on the recorded LQ trajectories -----------------------------------------
@pytest.mark.parametrize("pol", POLICIES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ["formul_box_qp_n64", "formul_dense_qp_boxed_n96_m24"])
def test_device_newton_formulations_replay_reference(pgf, name, kind, pol):
    case = G.load_case(name)
    problem = G.rebuild_problem(case)  # (a new problem object: its derivatives are uploaded anew)
    dt, rho, tau = float(case["dt"]), float(case["rho"]), G.case_tau(case)
    m = int(case["m"])
    dn = pgf.DeviceNewton(problem, pol, case["x0"], case["y0"], dt, rho, tau, step_solver_type=kind)
    try:
        asm0, lu0, bytes0 = dn.unsym_stats()
        builds0, _ = dn.gram_stats()
        for k in range(int(case["steps"])):
            diff, n_neg = dn.step()
            assert n_neg == -1
            pre = f"{kind}/{pol}/{k}/"
            x, y = dn.point()
            assert np.array_equal(dn.mask(), case[pre + "mask"]), (k,)
            assert G.rel_err(x, case[pre + "xn"]) <= TOL, (k,)
            assert G.rel_err(y, case[pre + "yn"]) <= TOL, (k,)
            assert abs(diff - float(case[pre + "diff"])) <= TOL * max(1.0, diff)
        asm1, lu1, bytes1 = dn.unsym_stats()
        assert bytes1 == bytes0 == 0
        assert asm1 - asm0 >= 1
        if pol == "Simplified":
            assert lu1 - lu0 == 1
        if kind == "Standard":
            # rho J'J from the resident Gram matrix, built once per upload (none without constraints)
            assert dn.gram_stats()[0] - builds0 == (1 if m else 0)
    finally:
        dn.close()


# ---- 5. BASELINE config 4's instance against the oracle's Symmetric step ---------------------
@pytest.mark.parametrize("kind", KINDS)
def test_device_newton_formulations_config4_against_oracle(pgf, kind):
    from pygradflow_amd import problems

    n, m = 1024, 256
    prob = problems.dense_qp(n, m, seed=0, boxed_frac=0.25)
    x0, y0 = np.zeros(n), np.zeros(m)
    recs = O.NewtonOracle(prob, "Full", x0, y0, 1.0, 1.0).run(x0, y0, 3)
    dn = pgf.DeviceNewton(prob, "Full", x0, y0, 1.0, 1.0, step_solver_type=kind)
    try:
        for k, rec in enumerate(recs):
            dn.step()
            x, y = dn.point()
            assert np.array_equal(dn.mask(), rec["mask"]), k
            ex, ey = G.rel_err(x, rec["xn"]), G.rel_err(y, rec["yn"])
            print(f"{kind} step {k}: x {ex:.3e} y {ey:.3e}")
            assert ex <= TOL and ey <= TOL, (k, ex, ey)
            if k == 0:
                Q, A = prob.hess_dense(), prob.jac_dense().reshape(m, n)
                H = Q + 1.0 * (A.T @ A) if kind == "Standard" else Q
                err = G.rel_err(dn.newton_matrix(), R.newton_matrix(kind, H, A, rec["mask"], 1.0, 1.0))
                print(f"{kind}: matrix rel err {err:.3e}")
                assert err <= 1e-14
        assert dn.unsym_stats()[2] == 0
    finally:
        dn.close()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n,m,boxed", [(33, 31, 0.5), (65, 0, 0.5), (40, 7, 0.0)])
def test_device_newton_formulations_odd_sizes(pgf, kind, n, m, boxed):
    """Sizes off the tile edge, no constraints, nothing active: every policy against the oracle."""
    from pygradflow_amd import problems

    prob = problems.dense_qp(n, m, seed=3, boxed_frac=boxed)
    x0, y0 = np.zeros(n), np.zeros(m)
    for pol in POLICIES:
        recs = O.NewtonOracle(prob, pol, x0, y0, 1.0, 1.0).run(x0, y0, 3)
        dn = pgf.DeviceNewton(prob, pol, x0, y0, 1.0, 1.0, step_solver_type=kind)
        try:
            for k, rec in enumerate(recs):
                dn.step()
                x, y = dn.point()
                assert np.array_equal(dn.mask(), rec["mask"]), (pol, k)
                assert G.rel_err(x, rec["xn"]) <= TOL and G.rel_err(y, rec["yn"]) <= TOL, (pol, k)
        finally:
            dn.close()


# ---- 6. refusals ---------------------------------------------------------------------------
def test_formulation_refusals(pgf):
    from pygradflow_amd import _lib, problems

    lib = _lib.load()
    n, m = 8, 2
    inf = np.full(n, np.inf)
    sp = _Raw(n, m, -inf, inf, np.zeros(n), np.zeros(m), 1.0, 1.0, None, sparse=True)
    try:
        with pytest.raises(ValueError):
            sp.ck(lib.pgf_set_formulation(sp.h, 1))
    finally:
        sp.close()
    raw = _Raw(n, m, -inf, inf, np.zeros(n), np.zeros(m), 1.0, 1.0, None)
    try:
        with pytest.raises(ValueError):
            raw.ck(lib.pgf_set_formulation(raw.h, 7))
        with pytest.raises(ValueError):  # Symmetric handle: there is no Newton matrix
            raw.matrix()
    finally:
        raw.close()
    prob = problems.dense_qp(n, m, seed=0, boxed_frac=0.25)
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(n), np.zeros(m), 1.0, 1.0, step_solver_type="Standard")
    try:
        with pytest.raises(ValueError):
            dn.step(inertia_check=True)
        arr = (C.c_void_p * 1)(dn._hd.h)
        b = C.c_void_p()
        with pytest.raises(ValueError):
            _lib.check(lib.pgf_batch_create(arr, 1, C.byref(b)), dn._hd.h, "pgf_batch_create")
        dn.step()  # the handle is still good
    finally:
        dn.close()
    # back in the pool as a Symmetric handle
    dn = pgf.DeviceNewton(prob, "Full", np.zeros(n), np.zeros(m), 1.0, 1.0)
    try:
        _, n_neg = dn.step()
        assert n_neg == m
    finally:
        dn.close()
    # a problem that takes the banded path has no unsymmetric formulations
    band = problems.LinearQuadraticProblem(sps.identity(n, format="csr") * 2.0, np.ones(n),
                                           sps.csr_matrix(np.eye(m, n)), np.zeros(m), -inf, inf)
    band.pgf_force_band = True
    with pytest.raises(NotImplementedError):
        pgf.DeviceNewton(band, "Full", np.zeros(n), np.zeros(m), 1.0, 1.0, step_solver_type="Extended")


def test_report_rcond_and_transposed_solve_on_device(pgf):
    """``.deriv`` is downloaded on demand and the handle solves with the transpose too."""
    case = G.load_case("formul_dense_qp_boxed_n96_m24")
    problem = G.rebuild_problem(case)
    dt, rho = float(case["dt"]), float(case["rho"])
    for kind in KINDS:
        params = pgf.Params(newton_type="Full", step_solver_type=kind)
        orig = pgf.Iterate(problem, params, case["x0"], case["y0"])
        from pygradflow_amd.unsym_step_solvers import step_solver

        sv = step_solver(problem, params, orig, dt, rho)
        try:
            mask = case[f"{kind}/Full/0/mask"]
            sv.update_active_set(mask)
            sv.update_derivs(orig)
            sv.solve(orig)
            M = sv.deriv.toarray()
            assert G.rel_err(M, case[f"{kind}/Full/0/deriv"]) <= 1e-14
            assert sv.solver.num_neg_eigvals() is None
            rhs = np.random.default_rng(5).standard_normal(M.shape[0])
            assert G.rel_err(sv.solver.solve(rhs), np.linalg.solve(M, rhs)) <= TOL
            assert G.rel_err(sv.solver.solve(rhs, trans=True), np.linalg.solve(M.T, rhs)) <= TOL
            assert sv.unsym_stats()[2] == 0
        finally:
            sv.close()
