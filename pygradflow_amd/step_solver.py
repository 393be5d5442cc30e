"""``StepSolver``-shaped front end of the HIP Newton/KKT step.

Drop-in for the reference's plugin hook ``Params(step_solver=HipStepSolver)``
(``pygradflow/params.py:234``; called as ``step_solver(problem, params, iterate,
dt, rho)`` at ``pygradflow/step/solver/__init__.py:18-19``).  Surface mirrored from
``StepSolver`` / ``ScaledStepSolver`` / ``SymmetricStepSolver``
(``step/solver/step_solver.py:66-130``, ``scaled_step_solver.py:15-107``,
``symmetric_step_solver.py:13-164``) and ``StepResult`` (``step_solver.py:16-63``).

All arithmetic of the path runs in libpgf_hip.so; this module only moves numpy
arrays across the C ABI and keeps the reference's call protocol:
``update_active_set`` / ``update_derivs`` only stash and invalidate, ``solve`` does
the work, failures surface as ``StepSolverError``.
"""

from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
import scipy.sparse as sps

from . import _lib
from .errors import LinearSolverError, StepSolverError
from .linear_solver import HipLinearSolver
from .sparse import BandPlan, MAX_BANDWIDTH, apply_band_split, border_key, effective_band_split

DENSE_LIMIT = 20000  # n + m above which sparse derivatives take the banded path
DENSE_MAX = 60000    # largest n + m the dense path accepts (pgf_create; 28.8 GB of KKT matrix)


# --------------------------------------------------------------------------- handles
class _HandlePool:
    """Device workspaces keyed by (n, m, device): a solver object lives for one outer
    step (reference ``newton.py:313``), its 200+ MB of HBM should not."""

    def __init__(self):
        self._free = {}

    def acquire(self, n, m, device, sparse=False):
        key = (n, m, device, bool(sparse))
        lst = self._free.get(key)
        if lst:
            return lst.pop()
        lib = _lib.load()
        h = C.c_void_p()
        flags = _lib.CREATE_SPARSE if sparse else 0
        _lib.check(lib.pgf_create(n, m, device, flags, C.byref(h)), None, "pgf_create")
        return _Handle(h, n, m, device, bool(sparse))

    def release(self, handle):
        self._free.setdefault((handle.n, handle.m, handle.device, handle.sparse), []).append(handle)

    def clear(self):
        lib = _lib.load()
        for lst in self._free.values():
            for hd in lst:
                lib.pgf_destroy(hd.h)
        self._free.clear()


class _Handle:
    def __init__(self, h, n, m, device, sparse=False):
        self.h, self.n, self.m, self.device, self.sparse = h, n, m, device, sparse
        self.derivs_key = None  # identity of the matrices currently resident in HBM
        self.plan = None        # BandPlan of a sparse handle
        self.keepalive = None


POOL = _HandlePool()


def _content_hash(arr):
    """Hash of an array's FULL content (xxh3 where available: ~10 GB/s; else blake2b)."""
    if arr is None:
        return 0
    parts = [arr.data, arr.indices, arr.indptr] if sps.issparse(arr) else [arr]
    try:
        import xxhash

        hs = xxhash.xxh3_64()
    except Exception:  # pragma: no cover
        import hashlib

        hs = hashlib.blake2b(digest_size=8)
    for part in parts:
        a = np.ascontiguousarray(part)
        hs.update(str(a.shape).encode())
        hs.update(memoryview(a).cast("B"))
    return hs.intdigest() if hasattr(hs, "intdigest") else int.from_bytes(hs.digest(), "little")


def residency_key(problem):
    """Identity under which a constant-derivative problem's H, J (and q, b) stay resident in
    HBM: a token pinned to the problem object (so that an id cannot be recycled) PLUS the
    state of its data --
      * ``LinearQuadraticProblem``: a version counter that every assignment to Q / A / q / b
        bumps; the arrays themselves are frozen, an in-place edit raises (problems.py), so the
        counter cannot miss a change;
      * any other problem that declares ``pgf_constant_derivs``: a hash of the FULL content of
        its Q / A / q / b (a strided sample, as in round 2, misses edits between the samples:
        ADVICE r2).
    A stale key means: upload again."""
    token = getattr(problem, "_pgf_token", None)
    if token is None:
        token = object()
        try:
            problem._pgf_token = token
        except Exception:
            return None
    version = getattr(problem, "_pgf_version", None)
    if version is not None:
        return (token, ("v", int(version)))
    fp = tuple(_content_hash(getattr(problem, nm, None)) for nm in ("Q", "A", "q", "b"))
    return (token, fp)


def same_key(a, b):
    return a is not None and b is not None and a[0] is b[0] and a[1] == b[1]


def _dense_f64(mat, shape):
    if mat is None:
        return np.zeros(shape, dtype=np.float64)
    if sps.issparse(mat):
        mat = mat.toarray()
    mat = np.ascontiguousarray(mat, dtype=np.float64)
    if mat.shape != shape:
        raise ValueError(f"matrix shape {mat.shape}, expected {shape}")
    return mat


# --------------------------------------------------------------------------- step result
class StepResult:
    """Reference ``StepResult`` (``step_solver.py:16-63``); ``xn``, the rewritten
    ``dx`` and ``diff`` come from the device (same formulas)."""

    def __init__(self, orig_iterate, dx, dy, active_set, rcond=None, xn=None, yn=None, diff=None):
        self.orig_iterate = orig_iterate
        self.dx = dx
        self.dy = dy
        self.active_set = active_set
        self.rcond = rcond
        self.xn = xn
        self._yn = yn
        self._diff = diff
        if xn is None:
            # host construction (line search of the Globalized policy): clip like the
            # reference does (step_solver.py:25-48)
            lb, ub = orig_iterate.problem.var_lb, orig_iterate.problem.var_ub
            x = orig_iterate.x
            xn = x - dx
            dx = np.copy(dx)
            low = xn < lb
            xn[low] = lb[low]
            dx[low] = x[low] - lb[low]
            up = xn > ub
            xn[up] = ub[up]
            dx[up] = x[up] - ub[up]
            self.dx, self.xn = dx, xn

    @functools.cached_property
    def iterate(self):
        it = self.orig_iterate
        xn = self.xn.astype(it.x.dtype, copy=False)
        yn = self._yn if self._yn is not None else it.y - self.dy
        return type(it)(it.problem, it.params, xn, yn, it.eval)

    @functools.cached_property
    def diff(self):
        if self._diff is not None:
            return self._diff
        return float(np.sqrt(np.dot(self.dx, self.dx) + np.dot(self.dy, self.dy)))


# --------------------------------------------------------------------------- step function
class HipStepFunc:
    """Scaled residual function ``lambda * F`` of one implicit Euler step
    (reference ``ScaledImplicitFunc``, ``implicit_func.py:202-294``)."""

    def __init__(self, owner: "HipStepSolver"):
        self._o = owner
        self.problem = owner.problem
        self.orig_iterate = owner.orig_iterate
        self.dt = owner.dt
        self.lamb = 1.0 / owner.dt
        self.n, self.m = owner.n, owner.m

    # a3 + a4 on the device -------------------------------------------------
    def compute_active_set(self, iterate, rho, tau=None):
        o = self._o
        o._ensure_outer()
        x = _lib.as_f64(iterate.x)
        g = o._aug_lag_deriv_x(iterate, rho)
        mask = np.empty((self.n,), dtype=np.bool_)
        rc = o._lib.pgf_active_set(o._hd.h, _lib.dptr(x), _lib.dptr(g),
                                   math.nan if tau is None else float(tau), _lib.u8ptr(mask))
        _lib.check(rc, o._hd.h, "pgf_active_set")
        return mask

    # a5 + a6 on the device -------------------------------------------------
    def value_at(self, iterate, rho, active_set=None):
        o = self._o
        o._ensure_outer()
        x, y = _lib.as_f64(iterate.x), _lib.as_f64(iterate.y)
        g = o._aug_lag_deriv_x(iterate, rho)
        c = _lib.as_f64(iterate.aug_lag_deriv_y())
        mask = None if active_set is None else np.ascontiguousarray(active_set, dtype=np.bool_)
        out = np.empty((self.n + self.m,), dtype=np.float64)
        rc = o._lib.pgf_residual(o._hd.h, _lib.dptr(x), _lib.dptr(y), _lib.dptr(g), _lib.dptr(c),
                                 _lib.u8ptr(mask), _lib.dptr(out))
        _lib.check(rc, o._hd.h, "pgf_residual")
        return out

    # generalized Jacobian of the scaled residual: host-side, off the hot path (only the
    # Globalized policy and tests ask for it; reference implicit_func.py:254-294)
    def deriv(self, jac, hess, active_set):
        n, m, lamb = self.n, self.m, self.lamb
        keep = sps.diags(np.logical_not(active_set).astype(np.float64))
        F11 = lamb * sps.eye(n) + keep @ sps.csr_matrix(hess)
        F12 = keep @ sps.csr_matrix(jac).T
        F21 = -sps.csr_matrix(jac)
        F22 = sps.diags([lamb], shape=(m, m))
        return sps.bmat([[F11, F12], [F21, F22]], format="csc")

    def deriv_at(self, iterate, rho, active_set=None):
        if active_set is None:
            active_set = self.compute_active_set(iterate, rho)
        return self.deriv(iterate.aug_lag_deriv_xy(), iterate.aug_lag_deriv_xx(rho), active_set)


# --------------------------------------------------------------------------- step solver
class HipStepSolver:
    """``formulation``: 0 (default) the Symmetric reduced system; ``_lib.FORM_STANDARD`` /
    ``_EXTENDED`` / ``_ASYMMETRIC`` make the handle assemble and factor the reference's
    unsymmetric ``(n + m)`` system on the device instead (``pgf_set_formulation``; the product
    classes of ``unsym_step_solvers.py`` drive it, dense handles only)."""

    def __init__(self, problem, params, orig_iterate, dt, rho, device: int = 0, formulation: int = 0):
        if not (dt > 0.0 and rho > 0.0):
            raise ValueError("dt and rho must be positive")
        if np.dtype(params.dtype) != np.float64:
            raise ValueError(
                "HipStepSolver computes in float64 only (Precision.Single is outside the "
                "1e-10 parity contract); use the reference step solver for float32"
            )
        _lib.require_gpu()
        self._lib = _lib.load()
        self.problem = problem
        self.params = params
        self.n = problem.num_vars
        self.m = problem.num_cons
        self.orig_iterate = orig_iterate
        self.dt = dt
        self.rho = rho
        self.solver = None  # LinearSolver-shaped view of the device factor, set by solve()
        self._active_set = None
        self._jac = None
        self._hess = None
        self._derivs_dirty = True
        self._mask_dirty = True
        self._outer_sent = False
        # sparse (banded) mode: problems too large for a dense KKT matrix, or on request
        self.formulation = int(formulation)
        # ``problem.pgf_border`` ("auto" or KKT node indices): a bordered band (sparse.BandPlan)
        self._border = getattr(problem, "pgf_border", None)
        # ``problem.pgf_border_limit``: up to 1024 border nodes (None: 64)
        self._border_limit = getattr(problem, "pgf_border_limit", None)
        self._border_tried = None  # size of an automatic border that did not fit
        self.sparse = not self.formulation and (
            bool(getattr(problem, "pgf_force_band", False)) or self._border is not None
            or (self.n + self.m > DENSE_LIMIT))
        self._hd = POOL.acquire(self.n, self.m, device, sparse=self.sparse)
        self._set_formulation()
        self._func = HipStepFunc(self)
        self.last_n_neg = None

    # -- lifetime ----------------------------------------------------------
    def close(self):
        if getattr(self, "_hd", None) is not None:
            if self.formulation:
                # handles go back to the pool as Symmetric ones
                _lib.check(self._lib.pgf_set_formulation(self._hd.h, _lib.FORM_SYMMETRIC), self._hd.h,
                           "pgf_set_formulation")
                if self.formulation == _lib.FORM_STANDARD:
                    self._hd.derivs_key = None  # H in HBM carries the rho J'J term
            POOL.release(self._hd)
            self._hd = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _set_formulation(self):
        """On every dense handle taken from the pool, also to Symmetric: whatever the handle's
        last user left does not matter (banded handles have no formulations)."""
        if not self.sparse:
            _lib.check(self._lib.pgf_set_formulation(self._hd.h, self.formulation), self._hd.h,
                       "pgf_set_formulation")

    # -- StepSolver surface ------------------------------------------------
    @property
    def func(self):
        return self._func

    @property
    def active_set(self):
        assert self._active_set is not None
        return self._active_set

    @property
    def jac(self):
        assert self._jac is not None
        return self._jac

    @property
    def hess(self):
        assert self._hess is not None
        return self._hess

    def linear_solver(self, mat):
        return HipLinearSolver(mat, symmetric=True, device=self._hd.device)

    def update_active_set(self, active_set):
        self._active_set = np.array(active_set, dtype=np.bool_, copy=True)
        self._mask_dirty = True
        self.solver = None

    def update_derivs(self, iterate):
        # stash only (scaled_step_solver.py:76-79); H = lag_hess(x, y), no rho J'J term
        self._jac = iterate.aug_lag_deriv_xy()
        self._hess = iterate.aug_lag_deriv_xx(rho=0.0)
        self._derivs_dirty = True
        self.solver = None

    def reset_deriv(self):
        self._derivs_dirty = True
        self.solver = None

    # -- device state ------------------------------------------------------
    def _ensure_outer(self):
        if self._outer_sent:
            return
        hd, p, it = self._hd, self.problem, self.orig_iterate
        lb, ub = _lib.as_f64(p.var_lb), _lib.as_f64(p.var_ub)
        _lib.check(self._lib.pgf_set_bounds(hd.h, _lib.dptr(lb), _lib.dptr(ub)), hd.h, "pgf_set_bounds")
        xh, yh = _lib.as_f64(it.x), _lib.as_f64(it.y)
        _lib.check(self._lib.pgf_set_outer(hd.h, _lib.dptr(xh), _lib.dptr(yh), float(self.dt),
                                           float(self.rho)), hd.h, "pgf_set_outer")
        self._outer_sent = True
        self._mask_dirty = True

    def _push_state(self):
        self._ensure_outer()
        hd = self._hd
        if self._derivs_dirty:
            # constant H, J (linear-quadratic problems) stay resident in HBM across
            # Newton steps and outer steps; the token pins the problem object so the
            # identity cannot be recycled
            key = None
            # (Standard uploads aug_lag_deriv_xx(rho), which changes with rho: never resident)
            if (getattr(self.problem, "pgf_constant_derivs", False)
                    and self.formulation != _lib.FORM_STANDARD):
                key = residency_key(self.problem)
            if self.sparse and not same_key(key, hd.derivs_key):
                if self._push_sparse_derivs():
                    hd.derivs_key = key
                else:
                    # the pattern is not banded enough for the banded kernels: take the dense
                    # path (CSR upload, densified on the device) -- the reference's SuperLU takes
                    # any pattern (lu_solver.py:14), so must this solver, as long as the dense
                    # KKT matrix fits
                    self._switch_to_dense()
                    return self._push_state()
            elif not same_key(key, hd.derivs_key):
                if self._csr_upload_pays():
                    self._push_csr_derivs()
                else:
                    H = _dense_f64(self._hess, (self.n, self.n))
                    J = _dense_f64(self._jac, (self.m, self.n))
                    rc = self._lib.pgf_set_derivs_dense(
                        hd.h, H.ctypes.data_as(C.c_void_p), max(self.n, 1),
                        J.ctypes.data_as(C.c_void_p), max(self.n, 1), _lib.PGF_HOST)
                    _lib.check(rc, hd.h, "pgf_set_derivs_dense")
                hd.derivs_key = key
            self._derivs_dirty = False
        if self._mask_dirty:
            mask = np.ascontiguousarray(self.active_set)
            _lib.check(self._lib.pgf_set_active_set(hd.h, _lib.u8ptr(mask)), hd.h, "pgf_set_active_set")
            self._mask_dirty = False

    def _csr_upload_pays(self):
        """scipy-sparse derivatives with under a quarter of the entries stored: send the
        non-zeros (12 bytes each) and densify on the device instead of sending n*n doubles."""
        if not (sps.issparse(self._hess) and (self.m == 0 or sps.issparse(self._jac))):
            return False
        nnz = self._hess.nnz + (self._jac.nnz if self.m else 0)
        return 4 * nnz < self.n * (self.n + self.m)

    def _push_csr_derivs(self):
        hd = self._hd
        hess = sps.csr_matrix(self._hess, dtype=np.float64)
        jac = sps.csr_matrix(self._jac, dtype=np.float64) if self.m else sps.csr_matrix((0, self.n))
        if hess.shape != (self.n, self.n) or jac.shape != (self.m, self.n):
            raise ValueError("derivative shapes do not match the problem")
        ip = C.POINTER(C.c_int)

        def arrs(mat):
            ptr = np.ascontiguousarray(mat.indptr, dtype=np.int32)
            idx = np.ascontiguousarray(mat.indices, dtype=np.int32)
            val = np.ascontiguousarray(mat.data, dtype=np.float64)
            return ptr, idx, val

        hp, hi, hv = arrs(hess)
        jp, ji, jv = arrs(jac)
        rc = self._lib.pgf_set_derivs_csr(
            hd.h, hp.ctypes.data_as(ip), hi.ctypes.data_as(ip), _lib.dptr(hv),
            jp.ctypes.data_as(ip), ji.ctypes.data_as(ip), _lib.dptr(jv))
        _lib.check(rc, hd.h, "pgf_set_derivs_csr")

    def _switch_to_dense(self):
        if self.n + self.m > DENSE_MAX:
            if self._border is None:
                # too large for a dense KKT matrix: a few dense rows / columns may be all that
                # keeps the pattern from a band -- try a bordered band before giving up
                self._border = "auto"
                return
            tried = "" if self._border_tried is None else (
                f" (a border of {self._border_tried} nodes does not bring the rest under it either)")
            raise NotImplementedError(
                f"sparse problem with half-bandwidth > {MAX_BANDWIDTH} after RCM{tried} and "
                f"n + m = {self.n + self.m} > {DENSE_MAX}: neither the banded nor the dense path "
                "can take it")
        device = self._hd.device
        POOL.release(self._hd)
        self.sparse = False
        self._hd = POOL.acquire(self.n, self.m, device, sparse=False)
        self._set_formulation()
        self._outer_sent = False
        self._mask_dirty = True
        self._derivs_dirty = True

    def _push_sparse_derivs(self):
        """Upload pattern (once) and values; False if the pattern is too wide for the banded
        kernels."""
        hd = self._hd
        hess = sps.csr_matrix(self._hess)
        jac = sps.csr_matrix(self._jac) if self.m else sps.csr_matrix((0, self.n))
        block = getattr(self.problem, "pgf_band_block", None)
        if apply_band_split(self._lib, hd.h, self.problem):
            hd.plan = None  # (a large border left the handle with the split: upload again)
        if hd.plan is not None and (hd.plan.block != (int(block) if block else None)
                                    or hd.plan.border_spec != border_key(self._border, self._border_limit)):
            hd.plan = None  # a different block size or border was asked for: upload again
        for attempt in (0, 1):
            if hd.plan is None:
                plan = BandPlan(hess, jac, self.n, self.m, block=block, border=self._border,
                                border_limit=self._border_limit, split=effective_band_split(self.problem))
                if not plan.supported:
                    self._border_tried = plan.k if self._border is not None else None
                    return False
                plan.upload(self._lib, hd.h)
                hd.plan = plan
            try:
                hv, jv = hd.plan.values(hess, jac)
                break
            except ValueError:
                if attempt:
                    raise
                hd.plan = None  # pattern changed: re-plan once
        _lib.check(self._lib.pgf_sparse_set_values(hd.h, _lib.dptr(hv), _lib.dptr(jv)), hd.h,
                   "pgf_sparse_set_values")
        return True

    def reduced_dims(self):
        if self.sparse:
            ni = int(self.n - np.count_nonzero(self.active_set))
            return ni, ni + self.m
        a, b = C.c_int(0), C.c_int(0)
        _lib.check(self._lib.pgf_reduced_dims(self._hd.h, C.byref(a), C.byref(b)), self._hd.h)
        return a.value, b.value

    def kkt_matrix(self):
        """Assembled reduced KKT matrix (lower triangle) -- debug / parity only."""
        if self.sparse:
            raise NotImplementedError("kkt_matrix: dense mode only")
        self._push_state()
        _, N = self.reduced_dims()
        K = np.zeros((N, N), dtype=np.float64)
        if N:
            _lib.check(self._lib.pgf_get_kkt(self._hd.h, _lib.dptr(K), N), self._hd.h, "pgf_get_kkt")
        return K

    def _host_reduced_kkt(self):
        """Reduced KKT matrix as scipy CSR (banded mode, diagnostics only: the products of the
        condition estimate; reference symmetric_step_solver.py:49-77)."""
        ina = np.where(np.logical_not(self.active_set))[0]
        lamb = 1.0 / self.dt
        H = sps.csr_matrix(self._hess) + sps.diags([lamb], shape=(self.n, self.n))
        Hii = sps.csr_matrix(H)[ina, :][:, ina]
        if self.m == 0:
            return sps.csr_matrix(Hii)
        Ji = sps.csc_matrix(self._jac)[:, ina]
        lower = sps.diags([-lamb / (1.0 + lamb * self.rho)], shape=(self.m, self.m))
        return sps.bmat([[Hii, Ji.T], [Ji, lower]], format="csr")

    def refinement_stats(self):
        """(refinement steps, LU fallbacks, relative residual of the last checked solve) of
        the device handle this solver uses (``pgf_refinement_stats``)."""
        a, b, r = C.c_int(0), C.c_int(0), C.c_double(0.0)
        _lib.check(self._lib.pgf_refinement_stats(self._hd.h, C.byref(a), C.byref(b), C.byref(r)),
                   self._hd.h)
        return a.value, b.value, r.value

    def band_stats(self):
        """(reductions, solve phases, panel solves) of the wide banded solve enqueued on this
        solver's handle since its creation (``pgf_debug_band_stats``)."""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        _lib.check(self._lib.pgf_debug_band_stats(self._hd.h, C.byref(a), C.byref(b), C.byref(c)),
                   self._hd.h)
        return a.value, b.value, c.value

    def border_stats(self):
        """(border size, factor phases, solve phases) of the bordered band on this solver's handle
        (``pgf_debug_border_stats``; zeros without a border)."""
        k, a, b = C.c_int(0), C.c_int(0), C.c_int(0)
        _lib.check(self._lib.pgf_debug_border_stats(self._hd.h, C.byref(k), C.byref(a), C.byref(b)),
                   self._hd.h)
        return k.value, a.value, b.value

    def solver_for_tests(self):
        """``LinearSolver`` view of the device factor without taking a step (parity tests:
        the factorisation is triggered by the first ``solve`` / ``num_neg_eigvals``)."""
        self._push_state()
        return _DeviceFactorView(self)

    def _aug_lag_deriv_x(self, iterate, rho):
        """``iterate.aug_lag_deriv_x(rho)`` (``obj_grad + J'(rho c + y)``, iterate.py:91-93), kept
        for the iterate it was last computed for: FullNewtonMethod.step asks the residual function
        for the active set and then the solver for the step at the SAME iterate (newton.py:83-89),
        and the reference's Iterate forms the product anew each time -- at config 2 a 4-million-entry
        sparse mat-vec on the host, 7.6 ms of a 10 ms plug-in step.  Iterates are immutable."""
        ck = getattr(self, "_g_cache", None)
        if ck is not None and ck[0] is iterate and ck[1] == rho:
            return ck[2]
        g = _lib.as_f64(iterate.aug_lag_deriv_x(rho))
        self._g_cache = (iterate, rho, g)
        return g

    # -- the step (scaled_step_solver.py:85-107) ---------------------------
    def solve(self, iterate):
        params = self.params
        try:
            self._push_state()
            hd = self._hd
            x, y = _lib.as_f64(iterate.x), _lib.as_f64(iterate.y)
            g = self._aug_lag_deriv_x(iterate, self.rho)
            c = _lib.as_f64(iterate.aug_lag_deriv_y())
            dx, xn = np.empty(self.n), np.empty(self.n)
            dy, yn = np.empty(self.m), np.empty(self.m)
            diff = C.c_double(0.0)
            rc = self._lib.pgf_newton_solve(
                hd.h, _lib.dptr(x), _lib.dptr(y), _lib.dptr(g), _lib.dptr(c),
                0 if self.formulation else int(bool(getattr(params, "inertia_correction", False))),
                _lib.dptr(dx), _lib.dptr(dy), _lib.dptr(xn), _lib.dptr(yn), C.byref(diff))
            _lib.check(rc, hd.h, "pgf_newton_solve")
        except LinearSolverError as e:
            raise StepSolverError(str(e)) from e
        self.solver = _DeviceFactorView(self)
        rcond = None
        if getattr(params, "report_rcond", False) and not self.formulation:
            from .cond_estimate import estimate_rcond

            # the estimator's products K x, K' x: on the device for the dense path (no N x N
            # copy over PCIe), with the host CSR matrix in banded mode
            Kop = self._host_reduced_kkt() if self.sparse else _DeviceKkt(self)
            rcond = estimate_rcond(Kop, self.solver, params)
        return StepResult(iterate, dx, dy, self.active_set, rcond, xn=xn, yn=yn, diff=diff.value)


class _DeviceKkt:
    """``mat`` of the condition estimate: ``mat @ x`` and ``mat.T @ x`` through
    ``pgf_kkt_apply`` (K is symmetric)."""

    def __init__(self, owner: HipStepSolver):
        self._o = owner
        n_red = owner.reduced_dims()[1]
        self.shape = (n_red, n_red)

    @property
    def T(self):
        return self

    def __matmul__(self, x):
        o = self._o
        x = _lib.as_f64(x)
        out = np.empty_like(x)
        _lib.check(o._lib.pgf_kkt_apply(o._hd.h, _lib.dptr(x), _lib.dptr(out)), o._hd.h, "pgf_kkt_apply")
        return out


class _DeviceFactorView:
    """``LinearSolver`` view of the factor the step solver holds on the device."""

    symmetric = True

    def __init__(self, owner: HipStepSolver):
        self._o = owner

    def solve(self, rhs, trans=False, initial_sol=None):
        """``rhs``: one right-hand side (rows,) or several (rows, nrhs), as ``LUSolver.solve``
        takes them; the result has the same shape."""
        o = self._o
        rhs = np.asarray(rhs, dtype=np.float64)
        if rhs.ndim == 2:
            return self._solve_multi(rhs, trans)
        if rhs.ndim != 1:
            raise ValueError("rhs must have one or two dimensions")
        rhs = _lib.as_f64(rhs)
        if o.sparse:
            # the banded system keeps its full size (active variables are identity rows):
            # expand the reduced right-hand side, solve, gather the reduced solution
            ina = np.logical_not(o.active_set)
            ni = int(np.count_nonzero(ina))
            if rhs.shape != (ni + o.m,):
                raise ValueError("rhs shape mismatch")
            full = np.zeros(o.n + o.m)
            full[: o.n][ina] = rhs[:ni]
            full[o.n:] = rhs[ni:]
            out = np.empty_like(full)
            rc = o._lib.pgf_linear_solve(o._hd.h, _lib.dptr(full), int(bool(trans)), _lib.dptr(out))
            _lib.check(rc, o._hd.h, "pgf_linear_solve")
            return np.concatenate([out[: o.n][ina], out[o.n:]])
        if o.formulation and rhs.shape != (o.n + o.m,):
            raise ValueError("rhs shape mismatch")
        sol = np.empty_like(rhs)
        rc = o._lib.pgf_linear_solve(o._hd.h, _lib.dptr(rhs), int(bool(trans)), _lib.dptr(sol))
        _lib.check(rc, o._hd.h, "pgf_linear_solve")
        return sol

    def _rows(self):
        """Length of a right-hand side of ``solve``."""
        o = self._o
        if o.sparse:
            return int(o.n - np.count_nonzero(o.active_set)) + o.m
        return o.n + o.m if o.formulation else o.reduced_dims()[1]

    def _solve_multi(self, rhs, trans):
        """(rows, nrhs) through ``pgf_linear_solve_multi``: the columns go to the library as
        contiguous vectors (column j at ``j * ld``)."""
        o = self._o
        rows, nrhs = rhs.shape
        if rows != self._rows():
            raise ValueError("rhs shape mismatch")
        if nrhs == 0:
            return np.empty((rows, 0))
        if o.sparse:
            ina = np.logical_not(o.active_set)
            ni = int(np.count_nonzero(ina))
            full = np.zeros((nrhs, o.n + o.m))
            full[:, : o.n][:, ina] = rhs[:ni].T
            full[:, o.n:] = rhs[ni:].T
        else:
            full = np.ascontiguousarray(rhs.T)
        out = np.empty_like(full)
        ld = max(full.shape[1], 1)
        rc = o._lib.pgf_linear_solve_multi(o._hd.h, _lib.dptr(full), nrhs, ld, int(bool(trans)),
                                           _lib.dptr(out))
        _lib.check(rc, o._hd.h, "pgf_linear_solve_multi")
        if o.sparse:
            return np.concatenate([out[:, : o.n][:, ina], out[:, o.n:]], axis=1).T.copy()
        return out.T.copy()

    def num_neg_eigvals(self):
        o = self._o
        if o.formulation:
            return None  # (an LU has no inertia: LUSolver.num_neg_eigvals())
        out = C.c_int(0)
        _lib.check(o._lib.pgf_factor(o._hd.h, C.byref(out)), o._hd.h, "pgf_factor")
        return out.value

    def rcond(self):
        return None
