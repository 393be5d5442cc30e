// The batch driver behind the C ABI: pgf_batch_* (one launch sequence for many dense handles) --
// lifecycle, the outer step and the host-driven Newton step, with what both kinds of batch share at
// creation.  What it needs of the dense step is listed in pgf_api_internal.h.  A batch of banded
// handles (b->band.on) shares the entry points and the vector kernels; its own half is
// pgf_api_band_batch.hip, and each entry point that differs hands over in one line.  The
// device-resident controller: pgf_api_batch_ctl.hip; the read-outs: pgf_api_batch_read.hip.
#include <cstring>
#include <new>

#include "pgf_api_internal.h"
#include "pgf_kernels.h"

// ---------------------------------------------------------------- batched mode
// (pgf_batch_s, bfail, BHIPCHK: pgf_api_internal.h)
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

// ---- what both creates share ---------------------------------------------------------------------
void batch_alloc_bytes(pgf_batch b, hipError_t *e, void **p, size_t bytes, unsigned kind) {
  if (*e != hipSuccess) return;
  if (!bytes) bytes = 1;
  *e = (kind & BA_PINNED) ? hipHostMalloc(p, bytes) : hipMalloc(p, bytes);
  if (*e != hipSuccess) {
    *p = nullptr;
    return;
  }
  b->mem.emplace_back(*p, (kind & BA_PINNED) != 0);
  if (!(kind & BA_ZERO)) return;
  if (kind & BA_PINNED)
    std::memset(*p, 0, bytes);
  else
    *e = hipMemset(*p, 0, bytes);
}

int batch_check_shape(pgf_handle h, pgf_handle h0, const char **msg) {
  if (h->n != h0->n || h->m != h0->m || h->device != h0->device) {
    *msg = "batch: instances must share n, m and the device";
    return PGF_INVALID;
  }
  if (h->unsym.form) {
    *msg = "batch: the Symmetric formulation only";
    return PGF_INVALID;
  }
  return PGF_OK;
}

int batch_check_state(pgf_handle h, bool band, const char **msg) {
  if (!h->qp_mode || !h->bounds_set || !h->point_set) {
    *msg = band ? "batch: pgf_set_bounds, pgf_qp_set_vectors, pgf_qp_set_point first"
                : "batch: pgf_set_bounds, pgf_qp_set_problem, pgf_qp_set_point first";
    return PGF_NOT_READY;
  }
  if (h->step_pending) {
    *msg = "batch: a step is pending";
    return PGF_NOT_READY;
  }
  return PGF_OK;
}

hipError_t batch_begin(pgf_batch b, const pgf_handle *handles, int count) {
  const pgf_handle h0 = handles[0];
  b->hs.assign(handles, handles + count);
  b->B = count;
  b->n = h0->n;
  b->m = h0->m;
  b->device = h0->device;
  b->sc.n = b->n;
  b->sc.m = b->m;
  (void)hipSetDevice(b->device);
  return hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
}

// what both records name of an instance's handle and its batch slots
template <typename T>
static void fill_shared(pgf_batch b, int i, T &t) {
  const pgf_handle h = b->hs[i];
  t.lb = h->lb;
  t.ub = h->ub;
  t.q = h->q;
  t.b = h->b;
  t.x = h->x;
  t.y = h->y;
  t.xn = h->xn;
  t.yn = h->yn;
  t.g = h->g;
  t.c = h->c;
  t.F = h->F;
  t.b0full = h->b0full;
  t.dx = h->dx;
  t.dy = h->dy;
  t.w = h->w;
  t.tmpn = h->tmpn;
  t.mask = h->mask;
  t.counts = h->counts;
  t.ctl = b->ctl + BCTL_STRIDE * i;
  t.ps = b->ps + (size_t)BPS_STRIDE * i;
}

void batch_fill_vectors(pgf_batch b, int i, BandInst &u) { fill_shared(b, i, u); }

void batch_fill_vectors(pgf_batch b, int i, BInst &t) {
  const pgf_handle h = b->hs[i];
  fill_shared(b, i, t);
  t.slb = h->slb;
  t.sub = h->sub;
  t.xhat = h->xhat;
  t.yhat = h->yhat;
  t.rhs = h->rhs;
  t.sol = h->sol;
  t.partial = h->partial;
  t.red = h->red;
  t.mask_new = h->mask_new;
  t.idxI = h->idxI;
  t.idxA = h->idxA;
  t.pos = h->pos;
  t.flags = h->fac.flags;
}

// (sp.vec.stat_pending, sp.blk.kept: the banded handle's -- the batch's reductions write its block arrays;
// unb.lists_ready and the norm: the dense handle's.  Each is at rest on a handle of the other kind.)
void batch_own_handle(pgf_handle h) {
  h->mask_set = false;
  h->eval_fresh = false;
  h->sp.vec.stat_pending = false;
  h->sp.blk.kept = 0;
  h->unb.lists_ready = false;
  drop_norm(h);
  invalidate_factor(h);
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
  for (int i = 0; i < count; ++i) {  // (dense handles only from here on)
    const pgf_handle h = handles[i];
    if (!h) return PGF_INVALID;
    const char *msg = nullptr;
    int rc;
    if ((rc = batch_check_shape(h, h0, &msg)) || (rc = batch_check_state(h, /*band=*/false, &msg)))
      return fail(h, rc, msg);
  }
  pgf_batch b = new (std::nothrow) pgf_batch_s();
  if (!b) return PGF_INVALID;
  const size_t cnt = (size_t)count;
  hipError_t e = batch_begin(b, handles, count);
  batch_alloc(b, &e, &b->tab, cnt);
  batch_alloc(b, &e, &b->ctl, cnt * BCTL_STRIDE, BA_ZERO);
  batch_alloc(b, &e, &b->out.flags, cnt * BFL_STRIDE + 1, BA_ZERO);
  batch_alloc(b, &e, &b->out.diff, cnt);
  batch_alloc(b, &e, &b->out.norm, cnt);
  batch_alloc(b, &e, &b->out.red4, cnt * 4 * ((h0->n + h0->m + 255) / 256 + 1));
  batch_alloc(b, &e, &b->out.meas, cnt * 4);
  batch_alloc(b, &e, &b->ps, cnt * BPS_STRIDE);
  // (zeroed: the matrix norms of every instance are on the device before any step -- the
  // device-resident controller writes only lambda and its kin into ps)
  batch_alloc(b, &e, &b->h_ps, cnt * BPS_STRIDE, BA_PINNED | BA_ZERO);
  batch_alloc(b, &e, &b->bytes, cnt);
  batch_alloc(b, &e, &b->h_bytes, cnt, BA_PINNED);
  batch_alloc(b, &e, &b->out.h_meas, cnt * 4, BA_PINNED);
  batch_alloc(b, &e, &b->out.h_flags, cnt * BFL_STRIDE, BA_PINNED);
  batch_alloc(b, &e, &b->out.h_diff, cnt, BA_PINNED);
  batch_alloc(b, &e, &b->out.h_norm, cnt, BA_PINNED);
  // the condensed order: dense handles, a constraint block worth a column block
  const bool cond_possible = condensed_mode() != 0 && !h0->sparse && h0->m > 0 && h0->m <= h0->n &&
                             (condensed_mode() == 2 ||
                              (h0->m >= 64 && (h0->n + h0->m + 255) / 256 > (h0->n + 255) / 256));
  b->cond.ok = cond_possible;
  b->cond.mp = round_up32(h0->m);
  b->htab.resize(cnt);
  for (int i = 0; i < count && e == hipSuccess; ++i) {
    const pgf_handle h = handles[i];
    (void)hipStreamSynchronize(h->stream);
    BInst &t = b->htab[i];
    batch_fill_vectors(b, i, t);
    t.H = h->H;
    t.J = h->J;
    t.ldh = h->ldh;
    t.ldj = h->ldj;
    t.K = h->fac.K;
    t.ldk = h->fac.ldk;
    t.W = h->fac.W;
    t.wstride = (int64_t)h->fac.wstride;
    t.dvec = h->fac.dvec;
    t.dinv = h->fac.dinv;
    t.zwork = h->fac.zwork;
    t.Linv = h->fac.Linv;
    t.LinvT = h->fac.LinvT;
    t.hctl = h->fac.hctl;
    t.xpub = h->fac.xpub;
    t.cctl = h->fac.chain + 2 * h->fac.chain_stride;
    t.capblk = h->fac.chain_stride;
    t.V = nullptr;
    t.vd = nullptr;
    t.ldv = 0;
    if (cond_possible) {
      if ((e = condensed_reserve(h)) != hipSuccess) break;
      t.V = h->fac.V;
      t.vd = h->fac.vd;
      t.ldv = condensed_ldv(h->m);
    }
    batch_own_handle(h);
  }
  if (e == hipSuccess) e = hipMemcpy(b->tab, b->htab.data(), cnt * sizeof(BInst), hipMemcpyHostToDevice);
  int rc = e == hipSuccess ? batch_store_norms(b) : PGF_HIP_ERROR + (int)e;
  if (rc == PGF_OK &&
      (e = hipMemcpy(b->ps, b->h_ps, cnt * BPS_STRIDE * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess)
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
  for (const auto &a : b->mem) (void)(a.second ? hipHostFree(a.first) : hipFree(a.first));
  for (double *p : {b->dctl.cs, b->dctl.cp, b->dctl.log})
    if (p) (void)hipFree(p);
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
    pgf_handle h = b->hs[i];  // the handles' host-side view stays consistent, and is what goes to ps
    set_outer_scalars(h, dt[i], rho[i]);
    h->outer_set = true;
    double *p = b->h_ps + (size_t)BPS_STRIDE * i;
    p[BPS_DT] = dt[i];
    p[BPS_LAMB] = h->lamb;
    p[BPS_RHO] = rho[i];
    p[BPS_FACT] = h->fact;
    p[BPS_DELTA] = h->delta;
    b->h_bytes[i] = accept ? (accept[i] ? 1 : 0) : 1;
  }
  // condensed order for this outer step: the growth bound of condensed_wanted, for EVERY instance
  // (one launch sequence serves them all)
  b->cond.wanted = false;
  if (b->cond.ok) {
    bool all = true;
    for (int i = 0; i < b->B && all; ++i) {
      pgf_handle h = b->hs[i];
      if (residual_norms(h)) {
        all = false;
        break;
      }
      all = condensed_growth_ok(h);
    }
    b->cond.wanted = all;
  }
  b->cond.free = true;  // every instance refactorises in the next step (new lambda)
  // (a band batch guards with the full residual of every instance: no norm bound needed)
  if (!b->band.on)
    if (int rc = batch_store_norms(b)) return bfail(b, rc, "matrix norms of an instance");
  b->band.frozen.assign(b->B, 0);  // kb_advance clears ctl[3]
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
  b->band.frozen.assign(b->h_bytes, b->h_bytes + b->B);
  BHIPCHK(b, hipMemcpyAsync(b->bytes, b->h_bytes, (size_t)b->B, hipMemcpyHostToDevice, b->stream));
  batch_launch_set_frozen(b->stream, b->tab, b->B, b->bytes);
  BHIPCHK(b, hipGetLastError());
  return PGF_OK;
}

void batch_eval(pgf_batch b) {
  if (b->eval_fresh) return;
  if (b->band.on)
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
void batch_enqueue_step(pgf_batch b, unsigned policy, double tau, bool host_knows_factored) {
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
  const bool cond = (force || b->cond.free) ? b->cond.wanted : b->cond.last;
  b->cond.last = cond;
  b->cond.free = false;
  b->stepped = true;
  batch_launch_rhs_assemble(b->stream, st, b->B, b->sc, cond ? b->cond.mp : 0);
  // (condensed: the factor and solve kernels see nI rows -- their `m' is 0)
  const int Nmax = cond ? b->n : b->n + b->m, mf = cond ? 0 : b->m;
  // kernels of instances whose factor is still valid return at once (ctl[0] == 0); when the
  // host knows that every instance refactorises (Full) or none does, skip the other half
  const bool none_factor = !recompute && host_knows_factored;
  if (!none_factor) {
    ldlt_batch_factor_async(b->stream, b->tab, b->B, Nmax, mf, b->prof.enabled ? &b->prof : nullptr,
                            cond ? b->cond.mp : 0);
    if (b->dbg.inject_helper_failure) {
      b->dbg.inject_helper_failure = 0;
      ldlt_inject_helper_failure(b->stream, b->hs[0]->fac.flags);
    }
  }
  if (cond && !force) batch_launch_cond_prep_fwd(b->stream, b->tab, b->B, b->sc);
  ldlt_batch_solve_async(b->stream, b->tab, b->B, Nmax, mf, !force, cond);
  if (cond) batch_launch_cond_y(b->stream, b->tab, b->B, b->sc);
  batch_launch_step_update(b->stream, st, b->B, b->sc, b->out.diff, b->out.flags, /*move=*/!search);
  b->eval_fresh = false;
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
  if (b->band.on) return band_batch_step_async(b, policy, tau);
  batch_enqueue_step(b, policy, tau, b->all_factored);
  // (the Globalized policy: every instance's line search directly behind the step update)
  if (search)
    if (int rc = batch_ls_enqueue_stage(b)) return rc;
  // g and c at the new points, enqueued ahead of the host synchronisation (as pgf_qp_step_async):
  // behind it the five small launches would wait for the host one by one
  if (eval_ahead()) batch_eval(b);
  BHIPCHK(b, hipMemcpyAsync(b->out.h_diff, b->out.diff, b->B * sizeof(double), hipMemcpyDeviceToHost,
                            b->stream));
  BHIPCHK(b, hipMemcpyAsync(b->out.h_flags, b->out.flags, (size_t)b->B * BFL_STRIDE * sizeof(int),
                            hipMemcpyDeviceToHost, b->stream));
  b->step_pending = true;
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
  const int *fl = b->out.h_flags + BFL_STRIDE * i;
  adopt_batch_factor(h, fl[BFL_NI], fl[BFL_NEG], b->cond.last, b->cond.mp);
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

bool batch_ls_begin_sync(pgf_batch b) {
  const bool search = b->ls.pending;
  b->ls.pending = false;
  if (search) {
    ++b->ls.host_waits;
    b->ls.have_stats = true;
  }
  return search;
}

hipError_t batch_chain_off(pgf_batch b, int i) {
  hipError_t e = hipMemsetAsync(b->out.flags + BFL_STRIDE * (size_t)b->B, 0, sizeof(int), b->stream);
  ldlt_chain_helpers_off();
  ldlt_chain_set_enabled(false);
  for (int k = i < 0 ? 0 : i; k < (i < 0 ? b->B : i + 1); ++k) {
    DenseLdlt &f = b->hs[k]->fac;
    const hipError_t ek =
        hipMemsetAsync(f.xpub, 0xff, 2 * (size_t)f.chain_stride * 64 * sizeof(double), b->stream);
    if (e == hipSuccess) e = ek;
  }
  return e;
}

int pgf_batch_sync(pgf_batch b, int *status, int *n_neg, double *diff) {
  if (!b) return PGF_INVALID;
  if (!b->step_pending) return bfail(b, PGF_NOT_READY, "no step pending");
  b->step_pending = false;
  (void)hipSetDevice(b->device);
  if (b->band.on) return band_batch_sync(b, status, n_neg, diff);
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  const bool search = batch_ls_begin_sync(b);
  bool all_ok = true, any_repaired = false;
  for (int i = 0; i < b->B; ++i) {
    int *fl = b->out.h_flags + BFL_STRIDE * i;
    // bit 2 alone: the factorisation went through but the sampled residual of the solve is too
    // large (element growth): repaired on the instance's handle where the reference's pivoted LU
    // would simply have solved -- only an instance that cannot be repaired
    // reports a failed step
    if (fl[BFL_BAD] == 4) {
      double d = 0.0;
      const int rrc = batch_repair_instance(b, i, &d, search);
      if (rrc == PGF_OK || (search && rrc == PGF_LINE_SEARCH)) {
        fl[BFL_BAD] = 0;
        b->out.h_diff[i] = d;
        b->eval_fresh = false;  // the instance moved after the evaluation made ahead
        ++b->dbg.repaired;
        any_repaired = true;
      }
    }
    const bool bad = fl[BFL_BAD] != 0;
    // bit 1: the instance's chain helpers failed a hand-over check (kb_step_final): the step is
    // reported like a failed factorisation -- the controllers reject and repeat it -- and the
    // helpers are off from here on
    // (or one of its chained solves: those go off too, and the publication halves of the
    // instance's handle get their sentinels back)
    if (fl[BFL_BAD] & 2) (void)batch_chain_off(b, i);
    all_ok = all_ok && !bad;
    if (status) status[i] = bad ? PGF_SINGULAR : PGF_OK;
    if (n_neg) n_neg[i] = fl[BFL_NEG] + (b->cond.last ? b->m : 0);  // (+ the m pivots -delta)
    if (diff) diff[i] = b->out.h_diff[i];
    // (the Globalized policy: the instance's search decides its status and the length of its step)
    if (search && !bad) batch_ls_report(b, i, status, diff);
  }
  // a repaired instance holds no factor the batch can reuse (its ctl[1] is 0): a following
  // Simplified step must not skip the factor launch, or it would solve with the bare matrix
  b->all_factored = all_ok && !any_repaired;
  return PGF_OK;
}
