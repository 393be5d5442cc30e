#!/usr/bin/env python3
"""The resident Gram matrix of the condensed factorisation (G = J^T J, csrc/pgf_api_factor.hip
``gram_prepare``) against the CPU oracle (GPU).  Run under PGF_CONDENSED=2 with
PGF_CONDENSED_GRAM = 0 (never: the virtual column blocks), 1 (default: G is built at the second
condensed factorisation since the last derivative upload) and 2 (at the first); the switches are
read once per process.  Used by tests/test_gram_condensed_gpu.py.

  * boxed dense QPs with ragged m, Full / Simplified / ActiveSet, six steps with an outer advance
    (new dt, rho: new lambda, delta, same G) every second step: masks bit for bit, iterates to
    1e-10, inertia m, and which factorisations used G (``pgf_debug_gram_stats``);
  * the linear-solver view (``pgf_factor``, ``pgf_linear_solve``) after such a factorisation
    against numpy.linalg.solve;
  * a new J through ``pgf_set_derivs_dense``: G is rebuilt, the steps match the new problem's
    oracle; derivatives uploaded before every step: G is never built under the default rule;
  * the 4 x 4 matrix whose condensed order meets an exact zero pivot: natural order inside the call.
"""
import ctypes as C
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from oracle import newton_oracle as O  # noqa: E402  (checker)
from pygradflow_amd import _lib, problems  # noqa: E402
from pygradflow_amd.newton import DeviceNewton  # noqa: E402

GRAM = int(os.environ.get("PGF_CONDENSED_GRAM", "1"))
assert os.environ.get("PGF_CONDENSED") == "2", "run with PGF_CONDENSED=2"
TOL = 1e-10
# (dt, rho) of the outer steps: two Newton steps each
OUTER = [(1.0, 1.0), (2.0, 1.0), (0.5, 2.0)]
CASES = [
    # n, m, policy
    (600, 200, "Full"),
    (900, 256, "Simplified"),
    (1100, 520, "ActiveSet"),
    (700, 300, "Full"),
]


def gram_stats(dn):
    a, b = C.c_int(0), C.c_int(0)
    assert dn._lib.pgf_debug_gram_stats(dn._hd.h, C.byref(a), C.byref(b)) == 0
    return a.value, b.value


def rel(a, ref):
    return float(np.max(np.abs(a - ref)) / max(1.0, np.max(np.abs(ref)))) if ref.size else 0.0


def oracle_run(prob, kind, x, y, outer, per=2):
    """per steps at each (dt, rho) of outer, every outer step starting at the point reached."""
    recs = []
    for dt, rho in outer:
        part = O.NewtonOracle(prob, kind, x, y, dt, rho).run(x, y, per)
        recs.extend(part)
        x, y = part[-1]["xn"], part[-1]["yn"]
    return recs


def check_step(dn, rec, what):
    x, y = dn.point()
    assert np.array_equal(dn.mask(), rec["mask"]), (what, "mask")
    ex, ey = rel(x, rec["xn"]), rel(y, rec["yn"])
    print(f"   {what}: err x {ex:.2e} y {ey:.2e} kind {dn.factor_kind()} gram {gram_stats(dn)}", flush=True)
    assert ex <= TOL and ey <= TOL, (what, ex, ey)
    return max(ex, ey)


worst = 0.0
mask_changed = False
for n, m, kind in CASES:
    prob = problems.dense_qp(n, m, seed=11 + n, boxed_frac=0.3)
    x0, y0 = np.zeros(n), np.zeros(m)
    recs = oracle_run(prob, kind, x0, y0, OUTER)
    dn = DeviceNewton(prob, kind, x0, y0, *OUTER[0])
    b0, f0 = gram_stats(dn)
    kinds, used = [], []
    for k, rec in enumerate(recs):
        if k and k % 2 == 0:
            dn.advance_outer(*OUTER[k // 2])
        diff, n_neg = dn.step()
        worst = max(worst, check_step(dn, rec, f"n={n} m={m} {kind} step {k}"))
        assert n_neg == m, (n, m, kind, k, n_neg)  # m + the inertia of S (positive definite here)
        kinds.append(dn.factor_kind())
        used.append(gram_stats(dn)[1] - f0)
        if k and not np.array_equal(rec["mask"], recs[k - 1]["mask"]):
            mask_changed = True
    builds = gram_stats(dn)[0] - b0
    refined, lu, _ = dn.refinement_stats()
    assert lu == 0, (n, m, kind, lu)
    assert kinds[0] == 2 and kinds[1] == 2, (n, m, kind, kinds)  # (dt = 1: as tools/check_condensed.py)
    if GRAM == 0:
        assert builds == 0 and used[-1] == 0, (builds, used)
    else:
        assert builds == 1, (n, m, kind, builds)
        if kind == "Full":  # every step factorises
            ncond = np.cumsum([kd == 2 for kd in kinds])
            want = ncond if GRAM == 2 else np.maximum(ncond - 1, 0)
            # the default rule mixes the paths: no Gram use at the first condensed factorisation
            # after the upload, Gram use from the second one on
            assert list(used) == list(want), (n, m, kind, kinds, used)
        else:
            assert used[-1] >= 1, (n, m, kind, used)
    if kind == "Full":
        # the linear-solver view: factorise without a right-hand side row, solve with any vector
        h, lib = dn._hd.h, dn._lib
        nI, N = C.c_int(0), C.c_int(0)
        assert lib.pgf_reduced_dims(h, C.byref(nI), C.byref(N)) == 0
        N = N.value
        K = np.zeros((N, N))
        _lib.check(lib.pgf_get_kkt(h, _lib.dptr(K), N), h, "pgf_get_kkt")
        K = np.tril(K) + np.tril(K, -1).T
        nn = C.c_int(-1)
        _lib.check(lib.pgf_factor(h, C.byref(nn)), h, "pgf_factor")
        assert nn.value == m, (nn.value, m)
        assert dn.factor_kind() == kinds[-1]
        g1 = gram_stats(dn)[1]
        assert (g1 - f0 == used[-1] + 1) if (GRAM and kinds[-1] == 2) else (g1 - f0 == used[-1])
        rhs = np.random.default_rng(n).standard_normal(N)
        sol = np.empty(N)
        _lib.check(lib.pgf_linear_solve(h, _lib.dptr(rhs), 0, _lib.dptr(sol)), h, "pgf_linear_solve")
        ref = np.linalg.solve(K, rhs)
        err = float(np.max(np.abs(sol - ref)) / np.max(np.abs(ref)))
        print(f"   linear solve after the factorisation: rel err {err:.2e}", flush=True)
        assert err <= TOL, err
    dn.close()
    print(f"n={n} m={m} {kind}: kinds {kinds}, gram use {used}, builds {builds}", flush=True)
assert mask_changed, "no case changed its mask between steps: G[I,I] was gathered with one I only"

# ---- a new J (same H): G goes with the upload
n, m = 640, 200
prob = problems.dense_qp(n, m, seed=3, boxed_frac=0.3)
Q = np.ascontiguousarray(prob.hess_dense(), dtype=np.float64)
A1 = np.ascontiguousarray(prob.jac_dense(), dtype=np.float64).reshape(m, n)
A2 = np.ascontiguousarray(A1[::-1] * 1.25 + np.roll(A1, 7, axis=1) * 0.5)
prob2 = problems.LinearQuadraticProblem(Q, np.array(prob.q), A2, np.array(prob.b), np.array(prob.var_lb),
                                        np.array(prob.var_ub))
x0, y0 = np.zeros(n), np.zeros(m)
recs = O.NewtonOracle(prob, "Full", x0, y0, 1.0, 1.0).run(x0, y0, 3)
dn = DeviceNewton(prob, "Full", x0, y0, 1.0, 1.0)
h, lib = dn._hd.h, dn._lib
b0, f0 = gram_stats(dn)
for k, rec in enumerate(recs):
    dn.step()
    worst = max(worst, check_step(dn, rec, f"first J, step {k}"))
assert gram_stats(dn)[0] - b0 == (1 if GRAM else 0)
_lib.check(lib.pgf_set_derivs_dense(h, Q.ctypes.data_as(C.c_void_p), n, A2.ctypes.data_as(C.c_void_p), n,
                                    _lib.PGF_HOST), h, "pgf_set_derivs_dense")
dn._hd.derivs_key = None  # (the pooled handle no longer holds `prob')
x, y = recs[-1]["xn"], recs[-1]["yn"]
dn.set_outer(x, y, 1.0, 1.0)
recs2 = O.NewtonOracle(prob2, "Full", x, y, 1.0, 1.0).run(x, y, 3)
for k, rec in enumerate(recs2):
    diff, n_neg = dn.step()
    worst = max(worst, check_step(dn, rec, f"second J, step {k}"))
    assert n_neg == m
b1, f1 = gram_stats(dn)
assert b1 - b0 == (2 if GRAM else 0), (b0, b1)
assert f1 - f0 == {0: 0, 1: 4, 2: 6}[GRAM], (f0, f1)
# derivatives uploaded before every step: the default rule never builds G
x, y = recs2[-1]["xn"], recs2[-1]["yn"]
recs3 = O.NewtonOracle(prob2, "Full", x, y, 1.0, 1.0).run(x, y, 3)
for k, rec in enumerate(recs3):
    _lib.check(lib.pgf_set_derivs_dense(h, Q.ctypes.data_as(C.c_void_p), n, A2.ctypes.data_as(C.c_void_p), n,
                                        _lib.PGF_HOST), h, "pgf_set_derivs_dense")
    if k == 0:
        dn.set_outer(x, y, 1.0, 1.0)
    dn.step()
    worst = max(worst, check_step(dn, rec, f"upload before step {k}"))
b2, f2 = gram_stats(dn)
assert b2 - b1 == {0: 0, 1: 0, 2: 3}[GRAM], (b1, b2)
assert f2 - f1 == {0: 0, 1: 0, 2: 3}[GRAM], (f1, f2)
dn.close()
print("invalidation ok", flush=True)

# ---- S[0][0] = -2 + 1 / delta = 0 exactly (tools/check_condensed.py): with G as with the virtual
# blocks the factorisation is repeated in the natural order inside the call
Q = np.diag([-3.0, 2.0, 1.0, 4.0])
A = np.array([[1.0, 1.0, 0.0, 0.0]])
prob = problems.LinearQuadraticProblem(Q, np.ones(4), A, np.zeros(1), np.full(4, -np.inf), np.full(4, np.inf))
rec = O.NewtonOracle(prob, "Full", np.zeros(4), np.zeros(1), 1.0, 1.0).run(np.zeros(4), np.zeros(1), 1)[0]
dn = DeviceNewton(prob, "Full", np.zeros(4), np.zeros(1), 1.0, 1.0)
b0, f0 = gram_stats(dn)
diff, n_neg = dn.step()
x, y = dn.point()
assert n_neg == 2, n_neg
assert dn.factor_kind() == 1, dn.factor_kind()
assert np.max(np.abs(x - rec["xn"])) <= 1e-12 and np.max(np.abs(y - rec["yn"])) <= 1e-12
b1, f1 = gram_stats(dn)
assert b1 - b0 == (1 if GRAM == 2 else 0) and f1 == f0, (b0, b1, f0, f1)  # (the discarded one is not counted)
dn.close()
print("zero pivot with G: repeated in the natural order, inertia", n_neg, flush=True)
print("gram ok, worst", worst, flush=True)
