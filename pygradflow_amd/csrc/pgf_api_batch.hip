// The batch driver behind the C ABI: pgf_batch_* (one launch sequence for many dense handles), the
// device-resident step controller pgf_batch_ctl_* and the RCCL communicator pgf_comm_*.  What it
// needs of the dense step is listed in pgf_api_internal.h.  A batch of banded handles (b->band)
// shares the entry points and the vector kernels; its own half is pgf_api_band_batch.hip, and each
// entry point that differs hands over in one line.
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "pgf_api_internal.h"
#include "pgf_kernels.h"

// ---------------------------------------------------------------- batched mode
// (pgf_batch_s, bfail, BHIPCHK: pgf_api_internal.h -- shared with the banded half, pgf_api_band_batch.hip)
const char *pgf_batch_last_error(pgf_batch b) { return b ? b->err.c_str() : k_no_handle; }

// ||H||_inf, ||J||_1, ||J||_inf of every instance into the host copy of ps (residual_norms: one
// pass over H and J per handle, cached until its derivatives change)
static int batch_store_norms(pgf_batch b) {
  for (int i = 0; i < b->B; ++i) {
    pgf_handle h = b->hs[i];
    int rc = residual_norms(h);
    if (rc) return rc;
    double *p = b->h_ps + (size_t)BPS_STRIDE * i;
    p[BPS_NORM_H] = h->guard.h_rs[4];
    p[BPS_NORM_J1] = h->guard.h_rs[6];
    p[BPS_NORM_JINF] = h->guard.h_rs[5];
  }
  return PGF_OK;
}

int pgf_batch_create(const pgf_handle *handles, int count, pgf_batch *out) {
  return pgf_batch_create_ex(handles, count, 0u, out);
}

int pgf_batch_create_ex(const pgf_handle *handles, int count, unsigned flags, pgf_batch *out) {
  if (!out || !handles || count <= 0 || count > 65535) return PGF_INVALID;
  if (flags & ~(PGF_BATCH_WIDE_BAND | PGF_BATCH_BAND_CTL | PGF_BATCH_BORDER | PGF_BATCH_WIDE_BORDER |
                PGF_BATCH_BORDER_CTL | PGF_BATCH_CTL_REFINE | PGF_BATCH_LINE_SEARCH))
    return PGF_INVALID;
  // The Globalized policy: dense, narrow and wide band batches, host-driven steps.  The flag is
  // taken off before the batch is built and the line search attached behind it.
  if (flags & PGF_BATCH_LINE_SEARCH) {
    if (flags & (PGF_BATCH_BORDER | PGF_BATCH_WIDE_BORDER | PGF_BATCH_BAND_CTL | PGF_BATCH_BORDER_CTL |
                 PGF_BATCH_CTL_REFINE))
      return fail(handles[0], PGF_INVALID,
                  "batch: PGF_BATCH_LINE_SEARCH goes alone or with PGF_BATCH_WIDE_BAND (no border, no "
                  "device-resident controller)");
    int rc = pgf_batch_create_ex(handles, count, flags & ~PGF_BATCH_LINE_SEARCH, out);
    if (rc) return rc;
    if ((rc = batch_ls_attach(*out))) {
      if (handles[0]) handles[0]->err = (*out)->err;
      pgf_batch_destroy(*out);
      *out = nullptr;
    }
    return rc;
  }
  // (a border on a wide remainder: only together with the two flags it combines)
  if ((flags & PGF_BATCH_WIDE_BORDER) &&
      (flags & (PGF_BATCH_BORDER | PGF_BATCH_WIDE_BAND)) != (PGF_BATCH_BORDER | PGF_BATCH_WIDE_BAND))
    return PGF_INVALID;
  // (a border under the device-resident controller, refinement inside its loop: likewise)
  if ((flags & PGF_BATCH_BORDER_CTL) &&
      (flags & (PGF_BATCH_BORDER | PGF_BATCH_BAND_CTL)) != (PGF_BATCH_BORDER | PGF_BATCH_BAND_CTL))
    return PGF_INVALID;
  if ((flags & PGF_BATCH_CTL_REFINE) && !(flags & PGF_BATCH_BAND_CTL)) return PGF_INVALID;
  const pgf_handle h0 = handles[0];
  if (!h0) return PGF_INVALID;
  for (int i = 0; i < count; ++i)  // any banded handle: a band batch, or its refusal
    if (handles[i] && handles[i]->sparse) return band_batch_create(handles, count, flags, out);
  for (int i = 0; i < count; ++i) {
    const pgf_handle h = handles[i];
    if (!h) return PGF_INVALID;
    if (h->n != h0->n || h->m != h0->m || h->device != h0->device)
      return fail(h, PGF_INVALID, "batch: instances must share n, m and the device");
    if (h->sparse) return fail(h, PGF_INVALID, "batch: dense handles only");
    if (h->unsym.form) return fail(h, PGF_INVALID, "batch: the Symmetric formulation only");
    if (!h->qp_mode || !h->bounds_set || !h->point_set)
      return fail(h, PGF_NOT_READY, "batch: pgf_set_bounds, pgf_qp_set_problem, pgf_qp_set_point first");
    if (h->step_pending) return fail(h, PGF_NOT_READY, "batch: a step is pending");
  }
  pgf_batch b = new (std::nothrow) pgf_batch_s();
  if (!b) return PGF_INVALID;
  b->hs.assign(handles, handles + count);
  b->B = count;
  b->n = h0->n;
  b->m = h0->m;
  b->device = h0->device;
  b->sc.n = b->n;
  b->sc.m = b->m;
  (void)hipSetDevice(b->device);
  hipError_t e;
  std::vector<BInst> tab(count);
  if ((e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipMalloc((void **)&b->tab, count * sizeof(BInst))) != hipSuccess ||
      (e = hipMalloc((void **)&b->ctl, (size_t)count * 4 * sizeof(int))) != hipSuccess ||
      (e = hipMalloc((void **)&b->flags_out, ((size_t)count * 3 + 1) * sizeof(int))) != hipSuccess ||
      (e = hipMalloc((void **)&b->diff_out, count * sizeof(double))) != hipSuccess ||
      (e = hipMalloc((void **)&b->norm_out, count * sizeof(double))) != hipSuccess ||
      (e = hipMalloc((void **)&b->red4,
                     (size_t)count * 4 * ((h0->n + h0->m + 255) / 256 + 1) * sizeof(double))) !=
          hipSuccess ||
      (e = hipMalloc((void **)&b->meas_out, (size_t)count * 4 * sizeof(double))) != hipSuccess ||
      (e = hipMalloc((void **)&b->ps, (size_t)count * BPS_STRIDE * sizeof(double))) != hipSuccess ||
      (e = hipHostMalloc((void **)&b->h_ps, (size_t)count * BPS_STRIDE * sizeof(double))) !=
          hipSuccess ||
      (e = hipMalloc((void **)&b->bytes, (size_t)count)) != hipSuccess ||
      (e = hipHostMalloc((void **)&b->h_bytes, (size_t)count)) != hipSuccess ||
      (e = hipHostMalloc((void **)&b->h_meas, (size_t)count * 4 * sizeof(double))) != hipSuccess ||
      (e = hipHostMalloc((void **)&b->h_flags, (size_t)count * 3 * sizeof(int))) != hipSuccess ||
      (e = hipHostMalloc((void **)&b->h_diff, count * sizeof(double))) != hipSuccess ||
      (e = hipHostMalloc((void **)&b->h_norm, count * sizeof(double))) != hipSuccess) {
    pgf_batch_destroy(b);
    return PGF_HIP_ERROR + (int)e;
  }
  // the condensed order: dense handles, a constraint block worth a column block
  const bool cond_possible = condensed_mode() != 0 && !h0->sparse && h0->m > 0 && h0->m <= h0->n &&
                             (condensed_mode() == 2 ||
                              (h0->m >= 64 && (h0->n + h0->m + 255) / 256 > (h0->n + 255) / 256));
  b->cond_ok = cond_possible;
  b->cond_mp = round_up32(h0->m);
  for (int i = 0; i < count; ++i) {
    const pgf_handle h = handles[i];
    (void)hipStreamSynchronize(h->stream);
    BInst &t = tab[i];
    t.H = h->H;
    t.J = h->J;
    t.ldh = h->ldh;
    t.ldj = h->ldj;
    t.lb = h->lb;
    t.ub = h->ub;
    t.q = h->q;
    t.b = h->b;
    t.slb = h->slb;
    t.sub = h->sub;
    t.xhat = h->xhat;
    t.yhat = h->yhat;
    t.x = h->x;
    t.y = h->y;
    t.xn = h->xn;
    t.yn = h->yn;
    t.g = h->g;
    t.c = h->c;
    t.F = h->F;
    t.b0full = h->b0full;
    t.rhs = h->rhs;
    t.sol = h->sol;
    t.dx = h->dx;
    t.dy = h->dy;
    t.w = h->w;
    t.tmpn = h->tmpn;
    t.partial = h->partial;
    t.red = h->red;
    t.mask = h->mask;
    t.mask_new = h->mask_new;
    t.idxI = h->idxI;
    t.idxA = h->idxA;
    t.pos = h->pos;
    t.counts = h->counts;
    t.ctl = b->ctl + 4 * i;
    t.ps = b->ps + (size_t)BPS_STRIDE * i;
    t.K = h->fac.K;
    t.ldk = h->fac.ldk;
    t.W = h->fac.W;
    t.wstride = (int64_t)h->fac.wstride;
    t.dvec = h->fac.dvec;
    t.dinv = h->fac.dinv;
    t.zwork = h->fac.zwork;
    t.Linv = h->fac.Linv;
    t.LinvT = h->fac.LinvT;
    t.flags = h->fac.flags;
    t.hctl = h->fac.hctl;
    t.xpub = h->fac.xpub;
    t.cctl = h->fac.chain + 2 * h->fac.chain_stride;
    t.capblk = h->fac.chain_stride;
    t.V = nullptr;
    t.vd = nullptr;
    t.ldv = 0;
    if (cond_possible) {
      if ((e = condensed_reserve(h)) != hipSuccess) {
        pgf_batch_destroy(b);
        return PGF_HIP_ERROR + (int)e;
      }
      t.V = h->fac.V;
      t.vd = h->fac.vd;
      t.ldv = condensed_ldv(h->m);
    }
    // the batch owns the device-side state of the handle from here on
    h->mask_set = false;
    h->eval_fresh = false;
    h->unb.lists_ready = false;
    drop_norm(h);
    invalidate_factor(h);
  }
  if ((e = hipMemcpy(b->tab, tab.data(), count * sizeof(BInst), hipMemcpyHostToDevice)) !=
          hipSuccess ||
      (e = hipMemset(b->ctl, 0, (size_t)count * 4 * sizeof(int))) != hipSuccess ||
      (e = hipMemset(b->flags_out, 0, ((size_t)count * 3 + 1) * sizeof(int))) != hipSuccess) {
    pgf_batch_destroy(b);
    return PGF_HIP_ERROR + (int)e;
  }
  // the matrix norms of every instance are on the device before any step (the device-resident
  // controller writes only lambda and its kin into ps)
  std::memset(b->h_ps, 0, (size_t)count * BPS_STRIDE * sizeof(double));
  int rc = batch_store_norms(b);
  if (rc == PGF_OK &&
      (e = hipMemcpy(b->ps, b->h_ps, (size_t)count * BPS_STRIDE * sizeof(double), hipMemcpyHostToDevice)) !=
          hipSuccess)
    rc = PGF_HIP_ERROR + (int)e;
  if (rc) {
    pgf_batch_destroy(b);
    return rc;
  }
  *out = b;
  return PGF_OK;
}

int pgf_batch_destroy(pgf_batch b) {
  if (!b) return PGF_OK;
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  band_batch_free(b);
  batch_ls_free(b);
  for (void *p : {(void *)b->tab, (void *)b->ctl, (void *)b->flags_out, (void *)b->diff_out,
                  (void *)b->norm_out, (void *)b->red4, (void *)b->meas_out, (void *)b->ps,
                  (void *)b->bytes, (void *)b->dctl_cs, (void *)b->dctl_cp, (void *)b->dctl_log})
    if (p) (void)hipFree(p);
  for (void *p : {(void *)b->h_flags, (void *)b->h_diff, (void *)b->h_norm, (void *)b->h_meas,
                  (void *)b->h_ps, (void *)b->h_bytes})
    if (p) (void)hipHostFree(p);
  for (hipEvent_t e : b->prof.pool) (void)hipEventDestroy(e);
  for (auto &sp : b->prof.update_spans) {
    (void)hipEventDestroy(sp.first);
    (void)hipEventDestroy(sp.second);
  }
  if (b->stream) (void)hipStreamDestroy(b->stream);
  delete b;
  return PGF_OK;
}

int pgf_batch_stream(pgf_batch b, void **stream_out) {
  if (!b || !stream_out) return PGF_INVALID;
  *stream_out = (void *)b->stream;
  return PGF_OK;
}

// Start a new outer step for every instance with ITS OWN dt_i, rho_i (every instance has its
// own step-size controller).  accept[i] != 0 (or accept == NULL): (x^, y^) <- (x, y), the
// last steps were accepted; accept[i] == 0: (x, y) <- (x^, y^), the instance goes back to its
// outer point and retries with the new dt_i (StepController.compute_step: rejected steps keep
// the iterate, step_control.py:80-107).
int pgf_batch_advance_outer_each(pgf_batch b, const double *dt, const double *rho,
                                 const uint8_t *accept) {
  if (!b || !dt || !rho) return PGF_INVALID;
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  for (int i = 0; i < b->B; ++i)
    if (!(dt[i] > 0.0) || !(rho[i] > 0.0))
      return bfail(b, PGF_INVALID, "dt and rho must be positive");
  if (accept && !b->outer_set)
    for (int i = 0; i < b->B; ++i)
      if (!accept[i]) return bfail(b, PGF_NOT_READY, "nothing to go back to before the first outer step");
  (void)hipSetDevice(b->device);
  // the pinned staging buffers may still be in flight from the previous call
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  // g = Qx + q + A'(rho c + y) and c only change when a point moves (a rejected instance goes
  // back to its outer point) or its rho does: otherwise what the last step evaluated ahead stays
  bool eval_stays = b->eval_fresh;
  for (int i = 0; i < b->B; ++i) {
    if ((accept && !accept[i]) || rho[i] != b->hs[i]->rho) eval_stays = false;
    double *p = b->h_ps + (size_t)BPS_STRIDE * i;
    const double lamb = 1.0 / dt[i];
    p[BPS_DT] = dt[i];
    p[BPS_LAMB] = lamb;
    p[BPS_RHO] = rho[i];
    p[BPS_FACT] = 1.0 / (1.0 + lamb * rho[i]);
    p[BPS_DELTA] = lamb / (1.0 + lamb * rho[i]);
    b->h_bytes[i] = accept ? (accept[i] ? 1 : 0) : 1;
    pgf_handle h = b->hs[i];  // keep the handles' host-side view consistent
    h->dt = dt[i];
    h->lamb = lamb;
    h->rho = rho[i];
    h->fact = p[BPS_FACT];
    h->delta = p[BPS_DELTA];
    h->outer_set = true;
  }
  // condensed order for this outer step: the growth bound of condensed_wanted, for EVERY instance
  // (one launch sequence serves them all)
  b->cond_wanted = false;
  if (b->cond_ok) {
    bool all = true;
    for (int i = 0; i < b->B && all; ++i) {
      pgf_handle h = b->hs[i];
      if (residual_norms(h)) {
        all = false;
        break;
      }
      all = condensed_growth_ok(h);
    }
    b->cond_wanted = all;
  }
  b->cond_free = true;  // every instance refactorises in the next step (new lambda)
  // (a band batch guards with the full residual of every instance: no norm bound needed)
  if (!b->band)
    if (int rc = batch_store_norms(b)) return bfail(b, rc, "matrix norms of an instance");
  b->frozen.assign(b->B, 0);  // kb_advance clears ctl[3]
  BHIPCHK(b, hipMemcpyAsync(b->ps, b->h_ps, (size_t)b->B * BPS_STRIDE * sizeof(double),
                            hipMemcpyHostToDevice, b->stream));
  BHIPCHK(b, hipMemcpyAsync(b->bytes, b->h_bytes, (size_t)b->B, hipMemcpyHostToDevice, b->stream));
  batch_launch_advance(b->stream, b->tab, b->B, b->sc, b->bytes);
  b->eval_fresh = eval_stays;  // g depends on rho, and rejected instances moved
  b->ls.hat_fresh = false;     // (g, c at the outer points: evaluated by the next Globalized step)
  b->outer_set = true;
  b->have_mask = false;
  b->all_factored = false;
  BHIPCHK(b, hipGetLastError());
  return PGF_OK;
}

int pgf_batch_advance_outer(pgf_batch b, double dt, double rho) {
  if (!b) return PGF_INVALID;
  std::vector<double> dts(b->B, dt), rhos(b->B, rho);
  return pgf_batch_advance_outer_each(b, dts.data(), rhos.data(), nullptr);
}

// frozen[i] != 0: instance i sits out the following Newton steps (until the next
// pgf_batch_advance_outer*): the controller's early exits (converged after the first step,
// failed factorisation) must not move the instance any further.  NULL clears all.
int pgf_batch_set_frozen(pgf_batch b, const uint8_t *frozen) {
  if (!b) return PGF_INVALID;
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  (void)hipSetDevice(b->device);
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  for (int i = 0; i < b->B; ++i) b->h_bytes[i] = (frozen && frozen[i]) ? 1 : 0;
  b->frozen.assign(b->h_bytes, b->h_bytes + b->B);
  BHIPCHK(b, hipMemcpyAsync(b->bytes, b->h_bytes, (size_t)b->B, hipMemcpyHostToDevice, b->stream));
  batch_launch_set_frozen(b->stream, b->tab, b->B, b->bytes);
  BHIPCHK(b, hipGetLastError());
  return PGF_OK;
}

static void batch_eval(pgf_batch b) {
  if (b->eval_fresh) return;
  if (b->band)
    band_batch_eval(b);
  else
    batch_launch_eval(b->stream, b->tab, b->B, b->sc, PGF_GEMVT_PARTS);
  b->eval_fresh = true;
}

int pgf_batch_update_active_set(pgf_batch b, double tau) {
  if (!b) return PGF_INVALID;
  if (!b->outer_set) return bfail(b, PGF_NOT_READY, "pgf_batch_advance_outer first");
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  (void)hipSetDevice(b->device);
  batch_eval(b);
  batch_launch_mask(b->stream, b->tab, b->B, b->sc, 1, tau);
  b->have_mask = true;
  b->all_factored = false;
  BHIPCHK(b, hipGetLastError());
  return PGF_OK;
}

// everything of one batched Newton step, enqueued; host_knows_factored: the host's view that
// every instance holds a valid factor (lets a Simplified step skip the factor launches)
//
// PGF_STEP_LINE_SEARCH (a batch created with PGF_BATCH_LINE_SEARCH): the mask comes from the current
// points as always, but the residual, the right-hand side and the step update read the table that
// names the OUTER points (step_solver.solve(self.orig_iterate), newton.py:248), whose g, c are
// evaluated between the evaluation at the current points and the mask, as ls_enter orders them on
// the handle; the step update leaves the clipped direction and moves nothing.
static void batch_enqueue_step(pgf_batch b, unsigned policy, double tau, bool host_knows_factored) {
  const bool recompute = (policy & PGF_STEP_RECOMPUTE_MASK) != 0;
  const bool force = (policy & PGF_STEP_REFACTOR) != 0;
  const bool search = (policy & PGF_STEP_LINE_SEARCH) != 0;
  const BInst *st = search ? b->ls.otab : b->tab;
  batch_eval(b);
  if (search) batch_ls_eval_outer(b);
  batch_launch_mask(b->stream, b->tab, b->B, b->sc, recompute ? (force ? 2 : 1) : 0, tau);
  b->have_mask = true;
  // pivot order: free to choose when every instance refactorises (Full, or the first step of an
  // outer step); otherwise the one the factors in place were made with
  const bool cond = (force || b->cond_free) ? b->cond_wanted : b->cond_last;
  b->cond_last = cond;
  b->cond_free = false;
  b->stepped = true;
  batch_launch_rhs_assemble(b->stream, st, b->B, b->sc, cond ? b->cond_mp : 0);
  // (condensed: the factor and solve kernels see nI rows -- their `m' is 0)
  const int Nmax = cond ? b->n : b->n + b->m, mf = cond ? 0 : b->m;
  // kernels of instances whose factor is still valid return at once (ctl[0] == 0); when the
  // host knows that every instance refactorises (Full) or none does, skip the other half
  const bool none_factor = !recompute && host_knows_factored;
  if (!none_factor) {
    ldlt_batch_factor_async(b->stream, b->tab, b->B, Nmax, mf, b->prof.enabled ? &b->prof : nullptr,
                            cond ? b->cond_mp : 0);
    if (b->inject_helper_failure) {
      b->inject_helper_failure = 0;
      ldlt_inject_helper_failure(b->stream, b->hs[0]->fac.flags);
    }
  }
  if (cond && !force) batch_launch_cond_prep_fwd(b->stream, b->tab, b->B, b->sc);
  ldlt_batch_solve_async(b->stream, b->tab, b->B, Nmax, mf, !force, cond);
  if (cond) batch_launch_cond_y(b->stream, b->tab, b->B, b->sc);
  batch_launch_step_update(b->stream, st, b->B, b->sc, b->diff_out, b->flags_out, /*move=*/!search);
  b->eval_fresh = false;
}

int pgf_batch_debug_fail_next_helper(pgf_batch b) {
  if (!b) return PGF_INVALID;
  if (b->band) return bfail(b, PGF_INVALID, "band batch: no chain helpers");
  b->inject_helper_failure = 1;
  return PGF_OK;
}

int pgf_batch_step_async(pgf_batch b, unsigned policy, double tau) {
  if (!b) return PGF_INVALID;
  if (!b->outer_set) return bfail(b, PGF_NOT_READY, "pgf_batch_advance_outer first");
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  const bool search = (policy & PGF_STEP_LINE_SEARCH) != 0;
  if (search && !b->ls.on)
    return bfail(b, PGF_INVALID, "batch: PGF_STEP_LINE_SEARCH is served by single handles only");
  (void)hipSetDevice(b->device);
  const bool recompute = (policy & PGF_STEP_RECOMPUTE_MASK) != 0;
  const bool force = (policy & PGF_STEP_REFACTOR) != 0;
  if (search && !(recompute && force))
    return bfail(b, PGF_INVALID,
                 "PGF_STEP_LINE_SEARCH needs PGF_STEP_RECOMPUTE_MASK | PGF_STEP_REFACTOR (the Globalized policy)");
  if (!recompute && !b->have_mask)
    return bfail(b, PGF_NOT_READY, "no active set: pgf_batch_update_active_set first");
  if (!recompute && force)
    return bfail(b, PGF_INVALID, "batch: PGF_STEP_REFACTOR needs PGF_STEP_RECOMPUTE_MASK");
  if (b->band) return band_batch_step_async(b, policy, tau);
  batch_enqueue_step(b, policy, tau, b->all_factored);
  // (the Globalized policy: every instance's line search directly behind the step update)
  if (search)
    if (int rc = batch_ls_enqueue_stage(b)) return rc;
  // g and c at the new points, enqueued ahead of the host synchronisation (as pgf_qp_step_async):
  // behind it the five small launches would wait for the host one by one
  if (eval_ahead()) batch_eval(b);
  BHIPCHK(b, hipMemcpyAsync(b->h_diff, b->diff_out, b->B * sizeof(double), hipMemcpyDeviceToHost,
                            b->stream));
  BHIPCHK(b, hipMemcpyAsync(b->h_flags, b->flags_out, (size_t)b->B * 3 * sizeof(int),
                            hipMemcpyDeviceToHost, b->stream));
  b->step_pending = true;
  return PGF_OK;
}

// ---- device-resident DistanceRatioController ------------------------------
static const char *const k_band_ctl =
    "band batch: the device-resident controller is for dense batches (drive dt per instance with "
    "pgf_batch_advance_outer_each)";
int pgf_batch_ctl_init(pgf_batch b, double lamb_init, double rho, const double *params,
                       int max_iterations) {
  if (!b || !params || !(lamb_init > 0.0) || !(rho > 0.0) || max_iterations < 1) return PGF_INVALID;
  if (b->band && !b->band_ctl) return bfail(b, PGF_INVALID, k_band_ctl);
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  (void)hipSetDevice(b->device);
  const size_t ncs = (size_t)b->B * DCS_STRIDE;
  if (!b->dctl_cs) BHIPCHK(b, dalloc(&b->dctl_cs, ncs));
  if (!b->dctl_cp) BHIPCHK(b, dalloc(&b->dctl_cp, (size_t)DCP_COUNT));
  if (b->dctl_log_cap < max_iterations) {
    if (b->dctl_log) (void)hipFree(b->dctl_log);
    b->dctl_log = nullptr;
    BHIPCHK(b, dalloc(&b->dctl_log, (size_t)max_iterations * b->B * 3));
    b->dctl_log_cap = max_iterations;
  }
  std::vector<double> cs(ncs, 0.0), cp(DCP_COUNT, 0.0);
  for (int i = 0; i < b->B; ++i) {
    cs[(size_t)DCS_STRIDE * i + DCS_LAMB] = lamb_init;
    cs[(size_t)DCS_STRIDE * i + DCS_ACCEPTED] = 1.0;
  }
  cp[DCP_RHO] = rho;
  // params: newton_tol, lamb_red, lamb_min, lamb_inc, theta_max, K_P, K_I, theta_ref
  cp[DCP_NEWTON_TOL] = params[0];
  cp[DCP_LAMB_RED] = params[1];
  cp[DCP_LAMB_MIN] = params[2];
  cp[DCP_LAMB_INC] = params[3];
  cp[DCP_THETA_MAX] = params[4];
  cp[DCP_K_P] = params[5];
  cp[DCP_K_I] = params[6];
  if (!(params[7] > 0.0)) return bfail(b, PGF_INVALID, "theta_ref must be positive");
  cp[DCP_LOG_THETA_REF] = std::log(params[7]);
  BHIPCHK(b, hipMemcpyAsync(b->dctl_cs, cs.data(), ncs * sizeof(double), hipMemcpyHostToDevice, b->stream));
  BHIPCHK(b, hipMemcpyAsync(b->dctl_cp, cp.data(), DCP_COUNT * sizeof(double), hipMemcpyHostToDevice,
                            b->stream));
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  b->dctl_logged = 0;
  if (b->band) return band_batch_ctl_init(b);
  return PGF_OK;
}

// One Newton step of the loop below, finished on the device: diff_out and flags_out are what
// kb_dctl_mid / kb_dctl_end read.  The host cannot know all_factored inside the loop; lean (band
// batches): what it can still know, see there.
static void ctl_enqueue_step(pgf_batch b, unsigned policy, double tau, bool lean) {
  if (b->band) {
    band_batch_enqueue_step(b, policy, tau, lean);
    // (PGF_BATCH_CTL_REFINE: the host cannot know which instances refine, so both rounds go in)
    if (b->ctl_refine) band_batch_enqueue_refine(b);
    band_batch_enqueue_final(b);
  } else {
    batch_enqueue_step(b, policy, tau, false);
  }
}

int pgf_batch_ctl_iterate(pgf_batch b, unsigned policy, double tau, int iterations) {
  if (!b || iterations < 0) return PGF_INVALID;
  if (policy & PGF_STEP_LINE_SEARCH)
    return bfail(b, PGF_INVALID, "batch: PGF_STEP_LINE_SEARCH is for host-driven steps (pgf_batch_step_async)");
  if (b->band && !b->band_ctl) return bfail(b, PGF_INVALID, k_band_ctl);
  if (!b->dctl_cs) return bfail(b, PGF_NOT_READY, "pgf_batch_ctl_init first");
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  if (b->dctl_logged + iterations > b->dctl_log_cap)
    return bfail(b, PGF_INVALID, "more iterations than pgf_batch_ctl_init reserved a log for");
  const bool recompute = (policy & PGF_STEP_RECOMPUTE_MASK) != 0;
  if (!recompute && (policy & PGF_STEP_REFACTOR))
    return bfail(b, PGF_INVALID, "batch: PGF_STEP_REFACTOR needs PGF_STEP_RECOMPUTE_MASK");
  (void)hipSetDevice(b->device);
  hipStream_t s = b->stream;
  b->ls.hat_fresh = false;  // (the loop moves the outer points)
  for (int it = 0; it < iterations; ++it) {
    // outer step of every instance at its own lambda; rejected instances go back first
    batch_launch_dctl_begin(s, b->B, b->dctl_cs, b->dctl_cp, b->ps, b->bytes);
    batch_launch_advance(s, b->tab, b->B, b->sc, b->bytes);
    // (lambda lives on the device here: the host cannot bound the growth of the condensed order)
    b->cond_wanted = false;
    b->cond_free = true;
    b->eval_fresh = false;
    b->outer_set = true;
    if (!recompute) {  // Simplified: mask and derivatives frozen at the outer point
      batch_eval(b);
      batch_launch_mask(s, b->tab, b->B, b->sc, 2, tau);
    }
    // lambda has changed: every instance assembles and factorises (ctl[0], decided on the device)
    ctl_enqueue_step(b, policy, tau, false);
    batch_eval(b);
    batch_launch_res_norm(s, b->tab, b->B, b->sc, b->norm_out);
    batch_launch_dctl_mid(s, b->tab, b->B, b->dctl_cs, b->dctl_cp, b->diff_out, b->flags_out,
                          b->norm_out);
    // Band batches, a policy that keeps the mask: the second step is enqueued without the assembly
    // and, on the wide route with the split on, without the inversion launches.  Every instance
    // still live has a clean factor of the band step one assembled: a bad pivot or a miss of the
    // guard in step one set its flag word, and kb_dctl_mid has frozen it for this step; the mask
    // is kept, so the band stays valid (ctl[1] = 1 from step one's update, ctl[0] = 0 here), and
    // the workgroups of the launches left out would all return.
    ctl_enqueue_step(b, policy, tau, !recompute);
    batch_launch_dctl_end(s, b->B, b->dctl_cs, b->dctl_cp, b->diff_out, b->flags_out,
                          b->dctl_log + (size_t)b->dctl_logged * b->B * 3);
    ++b->dctl_logged;
  }
  b->all_factored = false;
  BHIPCHK(b, hipGetLastError());
  return PGF_OK;
}

int pgf_batch_ctl_read(pgf_batch b, double *lamb, uint8_t *accepted, double *log3, int log_rows) {
  if (!b) return PGF_INVALID;
  if (b->band && !b->band_ctl) return bfail(b, PGF_INVALID, k_band_ctl);
  if (!b->dctl_cs) return bfail(b, PGF_NOT_READY, "pgf_batch_ctl_init first");
  (void)hipSetDevice(b->device);
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  // A failed hand-over of a chain helper or of a chained solve looked like a singular matrix to
  // the device-resident controller (kb_dctl_mid / _end: reject, 2 lambda) -- correct for that
  // iteration, but with the helpers still on it could repeat every iteration and lambda would
  // grow without bound.  The sticky word behind the flag triples says whether any
  // step of the loop saw one: helpers and chained solves go off, as pgf_batch_sync does.
  if (b->band) {
    if (int rc = band_batch_ctl_read(b)) return rc;  // (no helpers: the frozen flags instead)
  } else {
    int sticky = 0;
    BHIPCHK(b, hipMemcpy(&sticky, b->flags_out + 3 * (size_t)b->B, sizeof(int), hipMemcpyDeviceToHost));
    if (sticky) {
      ldlt_chain_helpers_off();
      ldlt_chain_set_enabled(false);
      for (int i = 0; i < b->B; ++i) {
        DenseLdlt &f = b->hs[i]->fac;
        BHIPCHK(b, hipMemsetAsync(f.xpub, 0xff, 2 * (size_t)f.chain_stride * 64 * sizeof(double), b->stream));
      }
      BHIPCHK(b, hipMemsetAsync(b->flags_out + 3 * (size_t)b->B, 0, sizeof(int), b->stream));
      BHIPCHK(b, hipStreamSynchronize(b->stream));
    }
  }
  std::vector<double> cs((size_t)b->B * DCS_STRIDE);
  BHIPCHK(b, hipMemcpy(cs.data(), b->dctl_cs, cs.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int i = 0; i < b->B; ++i) {
    if (lamb) lamb[i] = cs[(size_t)DCS_STRIDE * i + DCS_LAMB];
    if (accepted) accepted[i] = cs[(size_t)DCS_STRIDE * i + DCS_ACCEPTED] != 0.0;
    // the handles' host-side scalars follow the device's (the next host-driven call may use them)
    pgf_handle h = b->hs[i];
    const double l = cs[(size_t)DCS_STRIDE * i + DCS_USED];
    if (l > 0.0) {
      h->dt = 1.0 / l;
      h->lamb = 1.0 / h->dt;
      h->fact = 1.0 / (1.0 + h->lamb * h->rho);
      h->delta = h->lamb / (1.0 + h->lamb * h->rho);
    }
  }
  if (log3 && log_rows > 0) {
    const int rows = std::min(log_rows, b->dctl_logged);
    BHIPCHK(b, hipMemcpy(log3, b->dctl_log, (size_t)rows * b->B * 3 * sizeof(double),
                         hipMemcpyDeviceToHost));
  }
  return PGF_OK;
}

// An instance whose sampled residual failed (kb_sample_residual; kb_step_update then left its point
// alone): the single-instance accuracy guard on its handle -- full residual with K applied from H,
// J and the mask, iterative refinement with the factor the batch made, the pivoted LU if that does
// not contract (refine_if_needed) -- then the step update from the repaired solution.  The batch's
// stream is idle (pgf_batch_sync); the handle's buffers ARE the instance's.  Returns 0 when the
// instance's step is good now (its point, step length and factor state are in place).
//
// search (the step carried PGF_STEP_LINE_SEARCH): the stage sat the instance out, so its point is
// where the step found it.  The right-hand side in h->rhs is the outer point's and the residual and
// the refinement read nothing of the point; the step update does, so the handle is in its entered
// state for it ((x, y) name the outer point's vectors, as while a single handle's Globalized step is
// in flight) and leaves the repaired clipped direction.  Then the handle's own ls_search, exactly
// what pgf_qp_sync runs behind a settled step.  Returns PGF_LINE_SEARCH when that finds no trial.
static int batch_repair_instance(pgf_batch b, int i, double *diff_out, bool search) {
  pgf_handle h = b->hs[i];
  if (h->sparse || !h->guard.refine_mode) return PGF_SINGULAR;
  adopt_batch_factor(h, b->h_flags[3 * i + 2], b->h_flags[3 * i + 1], b->cond_last, b->cond_mp);
  DenseLdlt &f = h->fac;
  enqueue_residual(h);
  hipError_t e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) return hip_fail(h, e, "batched repair");
  int rc = refine_if_needed(h, /*swapped=*/false, /*with_step=*/false);
  if (rc) return rc;
  if (search) batch_ls_handle_enter(b, i);
  enqueue_step_update(h);  // (x, y) -> (xn, yn), dx, dy, ||d||
  if (search) {
    ls_leave(h);
  } else {
    launch_copy(h->stream, h->x, h->xn, h->n);
    launch_copy(h->stream, h->y, h->yn, h->m);
  }
  if ((e = hipMemcpyAsync(h->h_scal, h->scal, sizeof(double), hipMemcpyDeviceToHost, h->stream)) != hipSuccess ||
      (e = hipStreamSynchronize(h->stream)) != hipSuccess)
    return hip_fail(h, e, "batched repair");
  if (ldlt_chain_check(f)) return fail(h, PGF_HIP_ERROR, k_chain_msg);
  *diff_out = h->h_scal[0];
  if (search) {
    b->ls.host_waits += 2;  // (the residual's and the step update's above)
    rc = batch_ls_handle_search(b, i, diff_out);
  }
  // (host-side view only.  In the batch, kb_step_final left ctl[1] = 0 and pgf_batch_sync keeps
  // all_factored false: the instance's next step assembles K again and launches the factorisation,
  // a Simplified step included)
  invalidate_factor(h);
  return search ? rc : PGF_OK;
}

int pgf_batch_sync(pgf_batch b, int *status, int *n_neg, double *diff) {
  if (!b) return PGF_INVALID;
  if (!b->step_pending) return bfail(b, PGF_NOT_READY, "no step pending");
  b->step_pending = false;
  (void)hipSetDevice(b->device);
  if (b->band) return band_batch_sync(b, status, n_neg, diff);
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  const bool search = b->ls.pending;
  b->ls.pending = false;
  if (search) {
    ++b->ls.host_waits;
    b->ls.have_stats = true;
  }
  bool all_ok = true, any_repaired = false;
  for (int i = 0; i < b->B; ++i) {
    // bit 2 alone: the factorisation went through but the sampled residual of the solve is too
    // large (element growth): repaired on the instance's handle where the reference's pivoted LU
    // would simply have solved -- only an instance that cannot be repaired
    // reports a failed step
    if (b->h_flags[3 * i] == 4) {
      double d = 0.0;
      const int rrc = batch_repair_instance(b, i, &d, search);
      if (rrc == PGF_OK || (search && rrc == PGF_LINE_SEARCH)) {
        b->h_flags[3 * i] = 0;
        b->h_diff[i] = d;
        b->eval_fresh = false;  // the instance moved after the evaluation made ahead
        ++b->repaired;
        any_repaired = true;
      }
    }
    const bool bad = b->h_flags[3 * i] != 0;
    // bit 1: the instance's chain helpers failed a hand-over check (kb_step_final): the step is
    // reported like a failed factorisation -- the controllers reject and repeat it -- and the
    // helpers are off from here on
    if (b->h_flags[3 * i] & 2) {
      // (or one of its chained solves: those go off too, and the publication halves of the
      // instance's handle get their sentinels back)
      (void)hipMemsetAsync(b->flags_out + 3 * (size_t)b->B, 0, sizeof(int), b->stream);
      ldlt_chain_helpers_off();
      ldlt_chain_set_enabled(false);
      DenseLdlt &f = b->hs[i]->fac;
      (void)hipMemsetAsync(f.xpub, 0xff, 2 * (size_t)f.chain_stride * 64 * sizeof(double), b->stream);
    }
    all_ok = all_ok && !bad;
    if (status) status[i] = bad ? PGF_SINGULAR : PGF_OK;
    if (n_neg) n_neg[i] = b->h_flags[3 * i + 1] + (b->cond_last ? b->m : 0);  // (+ the m pivots -delta)
    if (diff) diff[i] = b->h_diff[i];
    // (the Globalized policy: the instance's search decides its status and the length of its step)
    if (search && !bad) batch_ls_report(b, i, status, diff);
  }
  // a repaired instance holds no factor the batch can reuse (its ctl[1] is 0): a following
  // Simplified step must not skip the factor launch, or it would solve with the bare matrix
  b->all_factored = all_ok && !any_repaired;
  return PGF_OK;
}

// ---- RCCL without PyTorch: the all-gather of residual norms as a C entry point ---------------
// (librccl.so through dlopen: a process that already runs torch.distributed keeps ITS copy of the
// library, and a host that never gathers never loads one)
namespace {
struct RcclApi {
  void *lib = nullptr;
  int (*GetUniqueId)(void *) = nullptr;
  // ncclUniqueId is passed BY VALUE: a 128-byte struct
  struct Id {
    char b[PGF_COMM_ID_BYTES];
  };
  int (*CommInitRank)(void **, int, Id, int) = nullptr;
  int (*CommDestroy)(void *) = nullptr;
  int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
  bool ok = false;
};
RcclApi &rccl() {
  static RcclApi a = []() {
    RcclApi r;
    for (const char *name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
      r.lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
      if (r.lib) break;
    }
    if (!r.lib) return r;
    r.GetUniqueId = (int (*)(void *))dlsym(r.lib, "ncclGetUniqueId");
    r.CommInitRank = (int (*)(void **, int, RcclApi::Id, int))dlsym(r.lib, "ncclCommInitRank");
    r.CommDestroy = (int (*)(void *))dlsym(r.lib, "ncclCommDestroy");
    r.AllGather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))dlsym(r.lib, "ncclAllGather");
    r.ok = r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.AllGather;
    return r;
  }();
  return a;
}
}  // namespace
struct pgf_comm_s {
  void *comm = nullptr;
  int nranks = 0, rank = 0, device = 0;
};

int pgf_comm_unique_id(void *id_out) {
  if (!id_out) return PGF_INVALID;
  if (!rccl().ok) return PGF_NOT_READY;
  return rccl().GetUniqueId(id_out) == 0 ? PGF_OK : PGF_HIP_ERROR;
}

int pgf_comm_create(int nranks, int rank, const void *id, int device, pgf_comm *out) {
  if (!out || !id || nranks <= 0 || rank < 0 || rank >= nranks) return PGF_INVALID;
  if (!rccl().ok) return PGF_NOT_READY;
  if (hipSetDevice(device) != hipSuccess) return PGF_INVALID;
  pgf_comm c = new (std::nothrow) pgf_comm_s();
  if (!c) return PGF_HIP_ERROR;
  RcclApi::Id uid;
  std::memcpy(uid.b, id, PGF_COMM_ID_BYTES);
  if (rccl().CommInitRank(&c->comm, nranks, uid, rank) != 0) {
    delete c;
    return PGF_HIP_ERROR;
  }
  c->nranks = nranks;
  c->rank = rank;
  c->device = device;
  *out = c;
  return PGF_OK;
}

int pgf_comm_destroy(pgf_comm c) {
  if (!c) return PGF_OK;
  if (c->comm && rccl().ok) (void)rccl().CommDestroy(c->comm);
  delete c;
  return PGF_OK;
}

int pgf_batch_allgather_norms(pgf_batch b, pgf_comm c, double *all_dev) {
  if (!b || !c || !all_dev) return PGF_INVALID;
  if (!b->outer_set) return bfail(b, PGF_NOT_READY, "pgf_batch_advance_outer first");
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  if (c->device != b->device) return bfail(b, PGF_INVALID, "communicator and batch live on different devices");
  (void)hipSetDevice(b->device);
  batch_eval(b);
  batch_launch_res_norm(b->stream, b->tab, b->B, b->sc, b->norm_out);
  double *slot = all_dev + (size_t)c->rank * b->B;
  BHIPCHK(b, hipMemcpyAsync(slot, b->norm_out, b->B * sizeof(double), hipMemcpyDeviceToDevice, b->stream));
  // in place: every rank's send buffer is its own slot of the receive buffer (ncclFloat64 = 8)
  if (rccl().AllGather(slot, all_dev, (size_t)b->B, /*ncclFloat64*/ 8, c->comm, b->stream) != 0)
    return bfail(b, PGF_HIP_ERROR, "ncclAllGather failed");
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  return PGF_OK;
}

int pgf_batch_refinement_stats(pgf_batch b, int *repaired) {
  if (!b) return PGF_INVALID;
  if (repaired) *repaired = b->repaired;
  return PGF_OK;
}

int pgf_batch_debug_factor_kind(pgf_batch b) {
  if (!b || !b->stepped || b->band) return 0;
  return b->cond_last ? 2 : 1;
}

int pgf_batch_profile_enable(pgf_batch b, int on) {
  if (!b) return PGF_INVALID;
  b->prof.enabled = on != 0;
  return PGF_OK;
}

// Accumulated device time of the K = LDLT_OB trailing-update launches since the last call and
// their algorithmic flops, from the reduced sizes of the last synchronised step.
int pgf_batch_profile_read(pgf_batch b, double *update_ms, int64_t *update_launches,
                           double *update_flops) {
  if (!b) return PGF_INVALID;
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  (void)hipSetDevice(b->device);
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  PgfProfile &p = b->prof;
  double ms_sum = 0.0, fl_sum = 0.0;
  for (size_t i = 0; i < p.update_spans.size(); ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.update_spans[i].first, p.update_spans[i].second) == hipSuccess)
      ms_sum += ms;
    // update_flops[i] >= 0: first row of the launch's trailing region, K-depth LDLT_OB; < 0: the rank-m
    // launch of the condensed order over the whole lower triangle, K-depth = -value
    const double start = p.update_flops[i];
    for (int k = 0; k < b->B; ++k) {
      const double Nk = (double)(b->h_flags[3 * k + 2] + (b->cond_last ? 0 : b->m));
      const double T = start < 0 ? Nk : Nk - start;
      const double depth = start < 0 ? -start : (double)LDLT_OB;
      if (T > 0) fl_sum += 2.0 * depth * (0.5 * T * (T + 1.0) + T);
    }
    p.pool.push_back(p.update_spans[i].first);
    p.pool.push_back(p.update_spans[i].second);
  }
  if (update_ms) *update_ms = ms_sum;
  if (update_launches) *update_launches = (int64_t)p.update_spans.size();
  if (update_flops) *update_flops = fl_sum;
  p.update_spans.clear();
  p.update_flops.clear();
  return PGF_OK;
}

int pgf_batch_residual_norms(pgf_batch b, double *norms_out, double *norms_out_dev) {
  if (!b) return PGF_INVALID;
  if (!b->outer_set) return bfail(b, PGF_NOT_READY, "pgf_batch_advance_outer first");
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  (void)hipSetDevice(b->device);
  batch_eval(b);
  batch_launch_res_norm(b->stream, b->tab, b->B, b->sc, b->norm_out);
  if (norms_out_dev)
    BHIPCHK(b, hipMemcpyAsync(norms_out_dev, b->norm_out, b->B * sizeof(double),
                              hipMemcpyDeviceToDevice, b->stream));
  BHIPCHK(b, hipMemcpyAsync(b->h_norm, b->norm_out, b->B * sizeof(double), hipMemcpyDeviceToHost,
                            b->stream));
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  if (norms_out) std::memcpy(norms_out, b->h_norm, b->B * sizeof(double));
  return PGF_OK;
}

int pgf_batch_measures(pgf_batch b, double active_tol, double *out) {
  if (!b || !out) return PGF_INVALID;
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  (void)hipSetDevice(b->device);
  if (!b->outer_set) return bfail(b, PGF_NOT_READY, "pgf_batch_advance_outer first");
  batch_eval(b);
  if (b->band) {
    band_batch_measures_eval(b);
    batch_launch_measures_final(b->stream, b->tab, b->B, b->sc, active_tol, b->red4, b->meas_out);
  } else {
    batch_launch_measures(b->stream, b->tab, b->B, b->sc, PGF_GEMVT_PARTS, active_tol, b->red4,
                          b->meas_out);
  }
  b->eval_fresh = false;  // tmpn / w were reused
  BHIPCHK(b, hipMemcpyAsync(b->h_meas, b->meas_out, (size_t)b->B * 4 * sizeof(double),
                            hipMemcpyDeviceToHost, b->stream));
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  std::memcpy(out, b->h_meas, (size_t)b->B * 4 * sizeof(double));
  return PGF_OK;
}

int pgf_batch_get_points(pgf_batch b, double *x, double *y) {
  if (!b) return PGF_INVALID;
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  (void)hipSetDevice(b->device);
  for (int i = 0; i < b->B; ++i) {
    if (x && b->n)
      BHIPCHK(b, hipMemcpyAsync(x + (size_t)i * b->n, b->hs[i]->x, b->n * sizeof(double),
                                hipMemcpyDeviceToHost, b->stream));
    if (y && b->m)
      BHIPCHK(b, hipMemcpyAsync(y + (size_t)i * b->m, b->hs[i]->y, b->m * sizeof(double),
                                hipMemcpyDeviceToHost, b->stream));
  }
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  return PGF_OK;
}

int pgf_batch_get_masks(pgf_batch b, uint8_t *mask) {
  if (!b || !mask) return PGF_INVALID;
  if (!b->have_mask) return bfail(b, PGF_NOT_READY, "no active set");
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  (void)hipSetDevice(b->device);
  for (int i = 0; i < b->B; ++i)
    if (b->n)
      BHIPCHK(b, hipMemcpyAsync(mask + (size_t)i * b->n, b->hs[i]->mask, b->n,
                                hipMemcpyDeviceToHost, b->stream));
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  return PGF_OK;
}
