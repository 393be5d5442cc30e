"""Batched mode: independent NLP instances sharded over the GPUs of one node.

The reference has no distributed code; its only parallelism is a process pool over
independent instances (``pygradflow/runners/runner.py:107-153``).  Here instance ``i`` of
``B`` lives on rank ``i // ceil(B / world)`` (contiguous blocks), every rank advances its
own instances with the device-resident Newton step, and per batched step there is exactly
ONE collective: an all-gather of the ranks' residual norms ``||F(z_i)||_2`` (fp64, 8 bytes
per instance) so that every rank sees all ``B`` norms for a global accept / stop decision
(SURVEY.md 8e).  RCCL over xGMI when the process group is ``nccl``; the same code runs on
``gloo`` for the CPU tests.
"""

from __future__ import annotations

import numpy as np


def shard_range(num_instances: int, world: int, rank: int):
    """Contiguous block of instance indices owned by ``rank`` (last ranks may own fewer)."""
    if world < 1 or not (0 <= rank < world) or num_instances < 0:
        raise ValueError("bad shard arguments")
    per = -(-num_instances // world) if num_instances else 0
    lo = min(rank * per, num_instances)
    hi = min(lo + per, num_instances)
    return lo, hi


def per_rank_capacity(num_instances: int, world: int) -> int:
    return -(-num_instances // world) if num_instances else 0


def gather_residual_norms(local_norms, num_instances: int, group=None):
    """All-gather the ranks' residual norms into one vector of length ``num_instances``.

    ``local_norms``: 1-d float64 torch tensor (device tensor for nccl, CPU tensor for gloo)
    holding this rank's norms in shard order.  Returns a tensor of all norms on every rank.
    Single process (no initialised group): returns ``local_norms`` unchanged.
    """
    import torch
    import torch.distributed as dist

    if not (dist.is_available() and dist.is_initialized()):
        return local_norms[:num_instances]
    world = dist.get_world_size(group)
    cap = per_rank_capacity(num_instances, world)
    send = torch.zeros(cap, dtype=torch.float64, device=local_norms.device)
    send[: local_norms.numel()] = local_norms
    out = torch.empty(cap * world, dtype=torch.float64, device=local_norms.device)
    dist.all_gather_into_tensor(out, send, group=group)
    if out.is_cuda:  # the solver's queue should not run beside the collective's
        torch.cuda.current_stream(out.device).synchronize()
    # drop the padding of short shards
    keep = []
    for r in range(world):
        lo, hi = shard_range(num_instances, world, r)
        keep.append(out[r * cap : r * cap + (hi - lo)])
    return torch.cat(keep) if keep else out[:0]


def batch_kind(shapes):
    """``"dense"`` or ``"band"`` for the ``(n, m, sparse)`` triples of a device batch's instances.
    One ``(n, m)`` is needed whatever the kind; whether banded instances fit together (pattern,
    bandwidth, border) and whether kinds are mixed is the library's to say, with its message."""
    shapes = list(shapes)
    if len({(n, m) for n, m, _ in shapes}) != 1:
        raise ValueError("a device batch needs instances of one (n, m)")
    return "band" if all(sp for _, _, sp in shapes) else "dense"


class BatchedDeviceNewton:
    """This rank's shard of a batch of linear-quadratic instances, all resident in HBM.

    ``make_problem(i)`` builds instance ``i`` (all of one shape).  The shard's instances are
    grouped into ONE device batch (``pgf_batch_*``): every kernel of the Newton step runs
    over all local instances at once, with no host round trip inside a step.  ``step()``
    advances every local instance by one Newton step and returns the gathered residual
    norms of the whole batch (one all-gather, nothing else crosses ranks).
    ``sequential=True`` drives the instances one after another through their own handles
    instead (the same kernels without the batch dimension; kept as the cross-check).

    Banded instances (``pgf_force_band``, or ``n + m`` above the dense limit: ``DeviceNewton``
    decides) form a BAND batch when all of them are banded on the narrow route (half-bandwidth
    <= 8, no border unless ``border=True``) with one sparsity pattern; values, vectors, bounds, ``dt`` and ``rho`` are
    each instance's own.  ``wide_band=True`` creates the batch through ``pgf_batch_create_ex`` with
    ``PGF_BATCH_WIDE_BAND``: instances on the wide route (block size 16, 32 or 64) are admitted
    too, when they share the block size and the setting of the factor / solve split.  What the
    library refuses (dense and banded mixed, different patterns, a wide band or a border without
    its flag) is raised as ``ValueError`` with its message.  ``self.band`` tells which kind the
    device batch is, ``self.band_block`` the block size of a band batch (``None`` otherwise).

    ``border=True`` (``PGF_BATCH_BORDER``) admits bordered instances on the narrow route: block size
    8 and one border size k (1..64) for all of them.  Each instance runs the factor phase of the
    bordered solve only where its matrix changed, the solve phase every step; the results are those
    of the single handles bit for bit.  ``self.band_border`` is k for a band batch (0 without a
    border, ``None`` on a dense batch), ``border_stats()`` counts the phases per instance.  A border
    on a wide remainder (without ``wide_border``) and a border under ``band_ctl`` (without
    ``border_ctl``) are refused.

    ``wide_border=True`` (``PGF_BATCH_WIDE_BORDER``; it sets ``wide_band`` and ``border`` too, the
    three bits go together) admits bordered instances whose remainder is on the wide route: one
    block size (16, 32 or 64), one border size k, the factor / solve split on for every handle.  An
    instance whose matrix changed factorises its band once and forms Y by one panel solve against
    the kept factors; every step solves against them.  ``band_block`` is 16, 32 or 64 and
    ``band_border`` is k; ``border_stats()`` counts the phases and ``band_wide_stats()`` the
    factor-only reductions and kept-factor solves of the band, which equal them.  Host-driven steps
    unless ``border_ctl`` is given (``band_ctl`` without it refuses a border); no effect with
    ``sequential=True``.

    ``band_ctl=True`` (``PGF_BATCH_BAND_CTL``, alone or with ``wide_band``) opens the device-resident
    step controller (``ctl_init / ctl_iterate / ctl_read``) to a band batch; without it a band batch
    refuses ``ctl_init`` as before, and a dense batch takes no notice of it.  Inside ``ctl_iterate``
    an instance whose solve misses its handle's ``refine_tol`` is not repaired on its handle (that
    needs the host): its step is rejected with 2 lambda, like a failed factorisation.
    ``ctl_stats()`` counts such steps.

    ``border_ctl=True`` (``PGF_BATCH_BORDER_CTL``; the library takes it only with ``border`` and
    ``band_ctl``, which are the caller's to give) lets the device-resident controller drive a bordered
    band batch, on the narrow route and, with ``wide_border``, on the wide one.  Without it the
    refusal stays; instances without a border take no notice of it.

    ``ctl_refine=True`` (``PGF_BATCH_CTL_REFINE``, only with ``band_ctl``) refines such an instance
    inside ``ctl_iterate`` on the device, as the host-driven batch repairs it on its handle: at most
    two rounds by the handle's rule, the same device functions in the same order.  The step is
    rejected only when the measure stays above the handle's ``refine_fail``.  Every banded step of
    the loop then carries the launches of two rounds, whose workgroups return at once for instances
    that do not refine.  ``ctl_refine_stats()`` counts refined steps and rounds.

    ``"Globalized", line_search=True`` (``PGF_BATCH_LINE_SEARCH``, alone or with ``wide_band``) runs
    the reference's ``GlobalizedNewtonMethod.step`` for every instance of a dense or band batch, each
    instance's Armijo line search in the same launches behind the step update: one host wait per
    step.  ``newton_tol`` is ``Params.newton_tol`` for the handles and the batch.  ``step_local()``
    reports an instance whose search accepted no trial as ``PGF_LINE_SEARCH`` in ``status`` -- its
    point has not moved and its ``diff`` is 0 -- and raises nothing; ``line_search()`` returns the
    last step's searches.  With another ``newton_type``, or with ``border`` / ``wide_border`` /
    ``band_ctl`` / ``border_ctl`` / ``ctl_refine``, ``line_search=True`` is a ``ValueError``, as is a
    negative ``newton_tol``, before any handle is built.  Without ``line_search`` a Globalized device
    batch is refused as before; ``sequential=True, line_search=True`` is the loop of single handles
    with the same surface (a handle's ``LineSearchError`` becomes the status).
    """

    def __init__(self, make_problem, num_instances, newton_type, dt, rho, device=0, rank=0,
                 world=1, group=None, tau=None, sequential=False, wide_band=False, band_ctl=False,
                 border=False, wide_border=False, border_ctl=False, ctl_refine=False,
                 line_search=False, newton_tol=1e-8):
        import ctypes as C
        import math

        import torch

        from . import _lib
        from .newton import _POLICY_BITS, DeviceNewton
        from .params import enum_name

        self.num_instances = num_instances
        self.rank, self.world, self.group = rank, world, group
        self.lo, self.hi = shard_range(num_instances, world, rank)
        self.count = self.hi - self.lo
        self.kind = enum_name(newton_type) if not isinstance(newton_type, str) else newton_type
        self.line_search_on = bool(line_search)
        self.newton_tol = float(newton_tol)
        if self.line_search_on:
            if self.kind != "Globalized":
                raise ValueError(f"line_search=True is the Globalized policy's, not {self.kind}'s")
            given = [name for name, on in (("border", border), ("wide_border", wide_border),
                                           ("band_ctl", band_ctl), ("border_ctl", border_ctl),
                                           ("ctl_refine", ctl_refine)) if on]
            if given:
                raise ValueError("line_search=True goes alone or with wide_band, not with " + ", ".join(given))
        if not self.newton_tol >= 0.0:
            raise ValueError("newton_tol must not be negative")
        if self.kind == "Globalized" and not sequential and not self.line_search_on:
            raise NotImplementedError(
                "Globalized: not in the device batch (its line search is per handle); "
                "sequential=True runs the instances through their own handles")
        self.policy = _POLICY_BITS[self.kind]
        self.tau = math.nan if tau is None else float(tau)
        self.dt, self.rho = float(dt), float(rho)
        self.sequential = bool(sequential)
        self.solvers = []
        for i in range(self.lo, self.hi):
            prob = make_problem(i)
            x0, y0 = np.zeros(prob.num_vars), np.zeros(prob.num_cons)
            self.solvers.append(DeviceNewton(prob, newton_type, x0, y0, dt, rho, tau=tau,
                                             device=device, newton_tol=self.newton_tol))
        self._torch = torch
        self._lib, self._C = _lib, C
        self.device = torch.device("cuda", device)
        self.norms = torch.zeros(max(1, self.count), dtype=torch.float64, device=self.device)
        self._b = None
        self.band = False
        self.band_block = None
        self.wide_border = bool(wide_border)
        self.wide_band = bool(wide_band) or self.wide_border
        self.band_ctl = bool(band_ctl)
        self.border = bool(border) or self.wide_border
        self.border_ctl = bool(border_ctl)
        self.ctl_refine = bool(ctl_refine)
        self.band_border = None
        self._frozen = None
        self._outer_points = [s.point() for s in self.solvers] if self.sequential else []
        if self.count and not self.sequential:
            self.band = batch_kind([(s.n, s.m, s.sparse) for s in self.solvers]) == "band"
            self.n, self.m = self.solvers[0].n, self.solvers[0].m
            lib = _lib.load()
            arr = (C.c_void_p * self.count)(*[s._hd.h for s in self.solvers])
            b = C.c_void_p()
            rc = self._create(lib, arr, C.byref(b))
            _lib.check(rc, self.solvers[0]._hd.h, "pgf_batch_create")
            self._b = b
            if self.line_search_on:
                _lib.check(lib.pgf_batch_set_line_search(b, self.newton_tol), batch=b,
                           what="pgf_batch_set_line_search")
            if self.band:
                self.band_block = int(self.solvers[0]._hd.plan.block_size)
                self.band_border = int(self.solvers[0]._hd.plan.k)
            self._begin_outer()

    def _create(self, lib, handles, out):
        """The device batch over ``handles``: through ``pgf_batch_create_ex`` with
        ``PGF_BATCH_WIDE_BAND``, ``PGF_BATCH_BAND_CTL``, ``PGF_BATCH_BORDER``,
        ``PGF_BATCH_WIDE_BORDER``, ``PGF_BATCH_BORDER_CTL`` and / or ``PGF_BATCH_CTL_REFINE`` when
        ``wide_band`` / ``band_ctl`` / ``border`` / ``wide_border`` / ``border_ctl`` / ``ctl_refine``
        was asked for (``wide_border`` has set the first and the third as well: the library takes its
        bit only with both; the last two are passed as given, and the library refuses them without
        their companions), ``pgf_batch_create`` otherwise."""
        flags = (self._lib.BATCH_WIDE_BAND if self.wide_band else 0) | \
            (self._lib.BATCH_BAND_CTL if getattr(self, "band_ctl", False) else 0) | \
            (self._lib.BATCH_BORDER if getattr(self, "border", False) else 0) | \
            (self._lib.BATCH_WIDE_BORDER if getattr(self, "wide_border", False) else 0) | \
            (self._lib.BATCH_BORDER_CTL if getattr(self, "border_ctl", False) else 0) | \
            (self._lib.BATCH_CTL_REFINE if getattr(self, "ctl_refine", False) else 0) | \
            (self._lib.BATCH_LINE_SEARCH if getattr(self, "line_search_on", False) else 0)
        if flags:
            return lib.pgf_batch_create_ex(handles, self.count, flags, out)
        return lib.pgf_batch_create(handles, self.count, out)

    def _begin_outer(self):
        lib, b = self._lib.load(), self._b
        self._lib.check(lib.pgf_batch_advance_outer(b, self.dt, self.rho), batch=b,
                        what="pgf_batch_advance_outer")
        if self.kind == "Simplified":
            self._lib.check(lib.pgf_batch_update_active_set(b, self.tau), batch=b,
                            what="pgf_batch_update_active_set")

    def advance_outer(self, dt=None, rho=None):
        self.dt = self.dt if dt is None else float(dt)
        self.rho = self.rho if rho is None else float(rho)
        if self._b is None:
            self._frozen = None
            for k, s in enumerate(self.solvers):
                self._outer_points[k] = s.point()
                s.advance_outer(self.dt, self.rho)
        else:
            self._begin_outer()

    def advance_outer_each(self, dt, rho, accepted=None):
        """New outer step with per-instance ``dt[i]``, ``rho[i]``; ``accepted[i]`` False sends
        instance i back to its outer point (a rejected step) before it retries."""
        dt = np.ascontiguousarray(dt, dtype=np.float64)
        rho = np.ascontiguousarray(np.broadcast_to(rho, dt.shape), dtype=np.float64)
        if dt.shape != (self.count,):
            raise ValueError("one dt per local instance")
        if self._b is None:
            for k, s in enumerate(self.solvers):
                if accepted is not None and not accepted[k]:
                    s.set_point(*self._outer_points[k])
                self._outer_points[k] = s.point()
                s.advance_outer(float(dt[k]), float(rho[k]))
            return
        acc = None
        if accepted is not None:
            acc = np.ascontiguousarray(accepted, dtype=np.bool_)
        lib, b = self._lib.load(), self._b
        self._lib.check(lib.pgf_batch_advance_outer_each(
            b, self._lib.dptr(dt), self._lib.dptr(rho), self._lib.u8ptr(acc)), batch=b,
            what="pgf_batch_advance_outer_each")
        if self.kind == "Simplified":
            self._lib.check(lib.pgf_batch_update_active_set(b, self.tau), batch=b,
                            what="pgf_batch_update_active_set")

    def set_frozen(self, frozen=None):
        """Instances with ``frozen[i]`` True sit out the following Newton steps (until the next
        ``advance_outer*``).  Device batch only."""
        if self._b is None:
            self._frozen = None if frozen is None else np.array(frozen, dtype=bool)
            return
        fz = None if frozen is None else np.ascontiguousarray(frozen, dtype=np.bool_)
        self._lib.check(self._lib.load().pgf_batch_set_frozen(self._b, self._lib.u8ptr(fz)),
                        batch=self._b, what="pgf_batch_set_frozen")

    def residual_norms_local(self):
        """Unscaled residual norms of the local instances at their current points (host)."""
        if self._b is None:
            return np.array([s.residual_norm() for s in self.solvers])
        out = np.empty(self.count)
        self._lib.check(self._lib.load().pgf_batch_residual_norms(self._b, self._lib.dptr(out),
                                                                   None), batch=self._b,
                        what="pgf_batch_residual_norms")
        return out

    def step_local(self):
        """One Newton step of every local instance; returns (status, n_neg, diff) arrays.
        The norms of the new points are left in ``self.norms`` (device)."""
        C = self._C
        cnt = self.count
        status = np.zeros(cnt, dtype=np.int32)
        n_neg = np.zeros(cnt, dtype=np.int32)
        diff = np.zeros(cnt)
        if cnt == 0:
            return status, n_neg, diff
        if self._b is None:
            from .errors import LineSearchError, StepSolverError

            base = self.norms.data_ptr()
            frozen = getattr(self, "_frozen", None)
            for k, s in enumerate(self.solvers):
                if frozen is not None and frozen[k]:
                    continue
                try:
                    diff[k], n_neg[k] = s.step()
                except StepSolverError:
                    status[k] = self._lib.PGF_SINGULAR
                    continue
                except LineSearchError:
                    if not self.line_search_on:
                        raise
                    status[k] = self._lib.PGF_LINE_SEARCH  # (the point has not moved)
                s.residual_norm(base + 8 * k)
            return status, n_neg, diff
        lib, b = self._lib.load(), self._b
        self._lib.check(lib.pgf_batch_step_async(b, self.policy, self.tau), batch=b,
                        what="pgf_batch_step_async")
        ip = C.POINTER(C.c_int)
        self._lib.check(lib.pgf_batch_sync(b, status.ctypes.data_as(ip), n_neg.ctypes.data_as(ip),
                                           self._lib.dptr(diff)), batch=b, what="pgf_batch_sync")
        self._lib.check(lib.pgf_batch_residual_norms(b, None, self.norms.data_ptr()), batch=b,
                        what="pgf_batch_residual_norms")
        return status, n_neg, diff

    def step(self):
        self.step_local()
        return gather_residual_norms(self.norms[: self.count], self.num_instances, self.group)

    def line_search(self):
        """The last Globalized step's line searches: dict(alpha[count], trials[count],
        merit0[count], slope[count], trial_merits[count, 30]) (``pgf_batch_line_search_stats``; with
        ``sequential=True`` the handles' own).  A frozen instance keeps what its last search left."""
        cnt = self.count
        out = dict(alpha=np.zeros(cnt), trials=np.zeros(cnt, dtype=np.int32), merit0=np.zeros(cnt),
                   slope=np.zeros(cnt), trial_merits=np.zeros((cnt, self._lib.LS_TRIALS)))
        if self._b is None:
            for k, s in enumerate(self.solvers):
                one = s.line_search()
                for key in out:
                    out[key][k] = one[key]
            return out
        self._lib.check(self._lib.load().pgf_batch_line_search_stats(
            self._b, self._lib.dptr(out["alpha"]), out["trials"].ctypes.data_as(self._C.POINTER(self._C.c_int)),
            self._lib.dptr(out["merit0"]), self._lib.dptr(out["slope"]), self._lib.dptr(out["trial_merits"])),
            batch=self._b, what="pgf_batch_line_search_stats")
        return out

    def line_search_stats(self):
        """(stage_launches, host_waits) of the last Globalized step of a device batch
        (``pgf_batch_debug_line_search_stats``): the launches its line-search stage enqueued for the
        whole batch and the stream waits the step took."""
        if self._b is None:
            raise NotImplementedError("device batch only")
        a, w = self._C.c_int(0), self._C.c_int(0)
        self._lib.check(self._lib.load().pgf_batch_debug_line_search_stats(
            self._b, self._C.byref(a), self._C.byref(w)), batch=self._b)
        return a.value, w.value

    def points(self):
        """(x[count][n], y[count][m]) of the local instances (host copies)."""
        if self._b is None:
            pts = [s.point() for s in self.solvers]
            return np.array([p[0] for p in pts]), np.array([p[1] for p in pts])
        x = np.empty((self.count, self.n))
        y = np.empty((self.count, self.m))
        self._lib.check(self._lib.load().pgf_batch_get_points(self._b, self._lib.dptr(x),
                                                               self._lib.dptr(y)), batch=self._b)
        return x, y

    def masks(self):
        if self._b is None:
            return np.array([s.mask() for s in self.solvers])
        mk = np.empty((self.count, self.n), dtype=np.bool_)
        self._lib.check(self._lib.load().pgf_batch_get_masks(self._b, self._lib.u8ptr(mk)),
                        batch=self._b)
        return mk

    def measures(self, active_tol=1e-8):
        """[count][4] array: stat_res, cons_violation, bound_violation, ||y||_inf per local
        instance (``Iterate.stat_res`` etc., evaluated on device)."""
        if self._b is None:
            rows = [s.measures(active_tol) for s in self.solvers]
            return np.array([[r["stat_res"], r["cons_violation"], r["bound_violation"], r["y_inf"]]
                             for r in rows]).reshape(self.count, 4)
        out = np.empty((self.count, 4))
        self._lib.check(self._lib.load().pgf_batch_measures(self._b, float(active_tol),
                                                            self._lib.dptr(out)), batch=self._b)
        return out

    # -- device-resident step controller (pgf_batch_ctl_*) ------------------------------
    def ctl_init(self, params, rho=None, max_iterations=64, lamb_init=None):
        """Arm the device-resident ``DistanceRatioController`` of every local instance."""
        if self._b is None:
            raise NotImplementedError("device batch only")
        if self.band and not self.band_ctl:
            raise NotImplementedError("dense batch only")
        vals = np.array([params.newton_tol, params.lamb_red, params.lamb_min, params.lamb_inc,
                         params.theta_max, params.K_P, params.K_I, params.theta_ref], dtype=np.float64)
        rho = self.rho if rho is None else float(rho)
        lamb = float(params.lamb_init if lamb_init is None else lamb_init)
        self._ctl_cap = int(max_iterations)
        self._lib.check(self._lib.load().pgf_batch_ctl_init(self._b, lamb, rho, self._lib.dptr(vals),
                                                            self._ctl_cap), batch=self._b,
                        what="pgf_batch_ctl_init")

    def ctl_iterate(self, iterations):
        """Enqueue ``iterations`` outer iterations (two batched Newton steps + the controller's
        decisions each) without a host synchronisation in between."""
        self._lib.check(self._lib.load().pgf_batch_ctl_iterate(self._b, self.policy, self.tau,
                                                               int(iterations)), batch=self._b,
                        what="pgf_batch_ctl_iterate")

    def ctl_read(self):
        """Wait; returns (lamb_next[count], accepted[count], log[iterations][count][3]) with
        log rows (lambda used, lambda next, accepted) per outer iteration so far."""
        lamb = np.empty(self.count)
        acc = np.empty(self.count, dtype=np.bool_)
        log = np.zeros((self._ctl_cap, self.count, 3))
        self._lib.check(self._lib.load().pgf_batch_ctl_read(
            self._b, self._lib.dptr(lamb), self._lib.u8ptr(acc), self._lib.dptr(log), self._ctl_cap),
            batch=self._b, what="pgf_batch_ctl_read")
        return lamb, acc, log

    def repaired(self):
        """Instances whose step the accuracy guard repaired inside a batched step so far
        (``pgf_batch_refinement_stats``): sampled residual failed, the instance's handle refined
        or fell back to the pivoted LU."""
        C = self._C
        k = C.c_int(0)
        if self._b is not None:
            self._lib.check(self._lib.load().pgf_batch_refinement_stats(self._b, C.byref(k)), batch=self._b)
        return k.value

    def band_stats(self):
        """(reductions, assemblies): batched launch sequences of a band batch enqueued so far
        (``pgf_batch_debug_band_stats``; zeros on a dense batch).  Device batch only."""
        if self._b is None:
            raise NotImplementedError("device batch only")
        C = self._C
        a, b = C.c_int(0), C.c_int(0)
        self._lib.check(self._lib.load().pgf_batch_debug_band_stats(self._b, C.byref(a), C.byref(b)),
                        batch=self._b)
        return a.value, b.value

    def band_wide_stats(self):
        """(reductions[count], solve_phases[count], lean_steps) of a wide band batch
        (``pgf_batch_debug_band_wide_stats``): per instance the wide reductions and the solve
        phases against kept factors its workgroups ran since the batch was created, and the steps
        enqueued without inversion launches.  Zeros on a dense or narrow batch.  On a bordered wide
        batch (``wide_border``): the factor-only reductions of the band and the solve phases against
        its kept factors, equal to the columns of ``border_stats()``, and the steps enqueued without
        any factor-phase launch.  Device batch only."""
        if self._b is None:
            raise NotImplementedError("device batch only")
        C = self._C
        red = np.zeros(self.count, dtype=np.int32)
        sol = np.zeros(self.count, dtype=np.int32)
        lean = C.c_int(0)
        ip = C.POINTER(C.c_int)
        self._lib.check(self._lib.load().pgf_batch_debug_band_wide_stats(
            self._b, red.ctypes.data_as(ip), sol.ctypes.data_as(ip), C.byref(lean)), batch=self._b)
        return red, sol, lean.value

    def border_stats(self):
        """(factor_phases[count], solve_phases[count]) of a bordered band batch
        (``pgf_batch_debug_border_stats``): per instance the factor phases (assembly, Y, S and its
        factor) and the solve phases it ran since the batch was created, counted on the device.
        Zeros on any other batch.  Device batch only."""
        if self._b is None:
            raise NotImplementedError("device batch only")
        fac = np.zeros(self.count, dtype=np.int32)
        sol = np.zeros(self.count, dtype=np.int32)
        ip = self._C.POINTER(self._C.c_int)
        self._lib.check(self._lib.load().pgf_batch_debug_border_stats(
            self._b, fac.ctypes.data_as(ip), sol.ctypes.data_as(ip)), batch=self._b)
        return fac, sol

    def ctl_stats(self):
        """(pivot_rejects[count], guard_rejects[count]) of a ``band_ctl`` batch
        (``pgf_batch_debug_ctl_stats``): per instance the Newton steps ``ctl_iterate`` rejected for
        a zero or non-finite pivot and those it rejected because the solve missed ``refine_tol``.
        Zeros on any other batch.  Device batch only."""
        if self._b is None:
            raise NotImplementedError("device batch only")
        piv = np.zeros(self.count, dtype=np.int32)
        grd = np.zeros(self.count, dtype=np.int32)
        ip = self._C.POINTER(self._C.c_int)
        self._lib.check(self._lib.load().pgf_batch_debug_ctl_stats(
            self._b, piv.ctypes.data_as(ip), grd.ctypes.data_as(ip)), batch=self._b)
        return piv, grd

    def ctl_refine_stats(self):
        """(refined_steps[count], rounds[count]) of a ``ctl_refine`` batch
        (``pgf_batch_debug_ctl_refine_stats``): per instance the Newton steps ``ctl_iterate`` refined
        on the device and the refinement rounds they ran.  Zeros on any other batch.  Device batch
        only."""
        if self._b is None:
            raise NotImplementedError("device batch only")
        ref = np.zeros(self.count, dtype=np.int32)
        rnd = np.zeros(self.count, dtype=np.int32)
        ip = self._C.POINTER(self._C.c_int)
        self._lib.check(self._lib.load().pgf_batch_debug_ctl_refine_stats(
            self._b, ref.ctypes.data_as(ip), rnd.ctypes.data_as(ip)), batch=self._b)
        return ref, rnd

    def factor_kind(self):
        """Pivot order of the factors the batch's instances hold: 0 none yet, 1 the natural
        order, 2 the condensed system (``pgf_batch_debug_factor_kind``).  Device batch only."""
        if self._b is None:
            raise NotImplementedError("device batch only")
        return int(self._lib.load().pgf_batch_debug_factor_kind(self._b))

    def profile(self, on=True):
        if self._b is not None:
            self._lib.check(self._lib.load().pgf_batch_profile_enable(self._b, int(on)),
                            batch=self._b)

    def profile_read(self):
        """Device time / launches / algorithmic flops of the trailing-update launches."""
        C = self._C
        ms, cnt, fl = C.c_double(0), C.c_int64(0), C.c_double(0)
        if self._b is not None:
            self._lib.check(self._lib.load().pgf_batch_profile_read(
                self._b, C.byref(ms), C.byref(cnt), C.byref(fl)), batch=self._b)
        return dict(update_ms=ms.value, update_launches=cnt.value, update_flops=fl.value)

    def close(self):
        if self._b is not None:
            self._lib.load().pgf_batch_destroy(self._b)
            self._b = None
        for s in self.solvers:
            s.close()
        self.solvers = []
