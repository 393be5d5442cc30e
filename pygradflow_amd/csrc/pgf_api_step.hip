// The Newton step of the dense Symmetric handle (newton_core_async, pgf_newton_solve,
// pgf_residual) and the device-resident LQ mode: pgf_qp_set_* ... pgf_qp_sync with the speculative
// step and its two redo paths, pgf_qp_step, pgf_qp_residual_norm, pgf_qp_measures.  The switches
// of the step (eval_ahead, step_fused, step_spec, step_handback, unbounded_front) and the wait of the
// hand-back (hb_wait) are here too.  Host code only.
#include <chrono>
#include <cmath>
#include <cstring>
#include <thread>

#include "pgf_api_internal.h"
#include "pgf_env.h"
#include "pgf_kernels.h"
#include "pgf_unsym.h"

// PGF_EVAL_AHEAD=0: g and c at the new point are evaluated at the start of the next step, not
// ahead of the host synchronisation of this one (newton_core_async, enqueue_qp_step, pgf_batch_step_async)
bool eval_ahead() { static const bool ahead = env_on("PGF_EVAL_AHEAD"); return ahead; }

// PGF_STEP_FUSED=0: the launches in front of and behind the factorisation of a qp step as before --
// k_mask_compact + k_residual_rhs; k_cond_y, k_step_update, the J and H row passes, k_sum_partials2,
// k_kkt_residual; three launches in pgf_qp_advance_outer -- instead of the fused ones (same values)
static bool step_fused() { static const bool on = env_on("PGF_STEP_FUSED"); return on; }

// PGF_STEP_SPEC=0: a step waits for the sizes of its index sets (one more host synchronisation
// per step) instead of running with the last known ones
bool step_spec() { static const bool on = env_on("PGF_STEP_SPEC"); return on; }

// PGF_STEP_HANDBACK=0: the tail's last launch leaves neither the new point's residual norm nor the
// status block in host memory -- k_unscaled_res_norm, the two copies and hipStreamSynchronize as before
static bool step_handback() { static const bool on = env_on("PGF_STEP_HANDBACK"); return on; }

// PGF_UNBOUNDED_FRONT=0: a handle without a finite bound takes the mask, the compaction and the mask
// difference like any other
static bool unbounded_front() { static const bool on = env_on("PGF_UNBOUNDED_FRONT"); return on; }

// ---------------------------------------------------------------- the hand-back's wait
static double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static inline void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
  __builtin_ia32_pause();
#else
  std::this_thread::yield();
#endif
}
// The spin is bounded by wall-clock time: HB_SPIN_FACTOR times what the handle's previous step
// took from its enqueueing to its word plus HB_SPIN_FLOOR_S (a step after a change of sizes or a
// first Gram build is longer than its predecessor), never more than HB_SPIN_CAP_S, which is also the
// bound of a handle's first step.  pgf_debug_handback_spin_bound overrides it (0: no spin at all).
static const double HB_SPIN_FACTOR = 16.0, HB_SPIN_FLOOR_S = 0.02, HB_SPIN_CAP_S = 2.0;

// The one wait of a dense qp step (the only user): for the sequence word the step's last launch
// stores behind the status block in h_stat -- no runtime call -- or, for a step that does not end in
// such a launch, when the bound expires or after a fault (the word never comes; the error surfaces
// here), hipStreamSynchronize.  A wait already taken for the same word returns at once.  *by_word
// (may be null): everything enqueued was seen complete without the runtime.
static int hb_wait(pgf_handle h, bool *by_word = nullptr) {
  if (by_word) *by_word = false;
  if (!h->hb.armed) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PGF_OK;
  }
  const unsigned long long want = h->hb.issued;
  if (h->hb.seen == want) {
    if (by_word) *by_word = true;
    return PGF_OK;
  }
  const unsigned long long *word = reinterpret_cast<const unsigned long long *>(h->h_stat + STAT_COPY);
  double bound = HB_SPIN_CAP_S;
  if (h->hb.last_step_s >= 0.0) bound = std::fmin(bound, HB_SPIN_FLOOR_S + HB_SPIN_FACTOR * h->hb.last_step_s);
  if (h->hb.bound_override >= 0.0) bound = h->hb.bound_override;
  bool got = false;
  if (bound > 0.0) {
    const double t0 = now_s();
    do {
      for (int k = 0; k < 64 && !got; ++k) {
        got = __atomic_load_n(word, __ATOMIC_ACQUIRE) >= want;
        if (!got) cpu_relax();
      }
    } while (!got && now_s() - t0 < bound);
  }
  if (got) {
    ++h->dbg.stat_hb_word;
    h->hb.last_step_s = now_s() - h->hb.t_enqueued;
  } else {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ++h->dbg.stat_hb_fallback;
  }
  h->hb.seen = want;
  if (by_word) *by_word = got;
  return PGF_OK;
}

// (expand: also the residual check's expansion of the solution into rs_v, rs_lv and the zeroing of
// its maxima, launch_residual_and_eval(..., prepared = true))
void enqueue_step_update(pgf_handle h, bool expand, const StepCondY *cy) {
  DenseLdlt &f = h->fac;
  const int bits = f.status_words;  // deferred status words go to the status block
  f.status_words = 0;
  h->flight.stat_bits |= bits;
  launch_step_update(h->stream, h->n, h->m, h->nI, h->fact, h->rho, h->x, h->y, h->lb, h->ub,
                     h->mask, h->pos, h->b0full, h->F, h->sol, h->dx, h->dy, h->xn, h->yn, h->red,
                     h->scal, h->ticket, h->lamb, expand ? h->guard.rs_v : nullptr, expand ? h->guard.rs_lv : nullptr,
                     expand ? h->guard.rs_red : nullptr, (bits & 1) ? f.flags : nullptr,
                     (bits & 2) ? f.chain + 2 * f.chain_stride + 1 : nullptr,
                     reinterpret_cast<int *>(h->stat + 14), cy && cy->partial ? cy : nullptr);
}
// after the host synchronisation of a step with deferred status words: to DenseLdlt::h_flags,
// in the order the two separate copies would have left them
static void absorb_status(pgf_handle h) {
  const int *w = reinterpret_cast<const int *>(h->h_stat + 14);
  if (h->flight.stat_bits & 1)
    for (int k = 0; k < 4; ++k) h->fac.h_flags[k] = w[k];
  else if (h->flight.stat_bits & 2)
    h->fac.h_flags[3] = w[3];
  h->flight.stat_bits = 0;
}

// residual + reduced rhs for the point in (h->x, h->y, h->g, h->c), then solve and update.
// Everything is enqueued; returns without syncing.  factored_out tells whether a factor
// was enqueued (its flags then need checking at the sync).
static int newton_core_async(pgf_handle h, bool *did_factor) {
  hipStream_t s = h->stream;
  h->flight.fused_eval_done = false;
  h->flight.fused_norm_done = false;
  h->flight.forget_factor();  // (set by factor_async, if this step factorises)
  if (h->sparse) return band_step_async(h, did_factor);
  const bool front_done = h->flight.front_done;
  h->flight.front_done = false;
  if (front_done) {
    // (qp_refresh_mask: F, b0full and rhs came with the compaction's launch)
  } else if (h->nA == 0) {  // the residual and the reduced right-hand side in one launch
    launch_residual_rhs(s, h->n, h->m, h->nI, h->lamb, h->dt, h->fact, h->xhat, h->yhat, h->x, h->y, h->g,
                        h->c, h->slb, h->sub, h->mask, h->idxI, h->F, h->b0full, h->rhs);
  } else {
    launch_residual(s, h->n, h->m, h->lamb, h->dt, h->xhat, h->yhat, h->x, h->y, h->g, h->c, h->slb,
                    h->sub, h->mask, h->F, h->b0full);
    launch_reduced_rhs(s, h->n, h->m, h->nI, h->nA, h->fact, h->F, h->idxI, h->idxA, h->H, h->ldh, h->J,
                       h->ldj, h->b0full, h->partial, PGF_GEMVT_PARTS, h->rhs);
  }
  *did_factor = false;
  h->guard.rs_skipped = h->fac.factored && h->guard.factor_clean;  // (a step that factorises is always checked)
  // the tail of a qp step in fewer launches (same values): s_y in the step update, the row passes
  // over J and H in one launch, the sums, the H pass's epilogue and the residual in another
  // (a step with PGF_STEP_LINE_SEARCH: the point after it is not x - d, nothing is evaluated ahead)
  const bool ahead = eval_ahead() && h->qp_mode && h->guard.refine_mode && !h->guard.rs_skipped && !h->ls.want;
  const bool fused_tail = ahead && step_fused();
  StepCondY cy{nullptr, nullptr, nullptr, 0.0, 0};
  if (!h->fac.factored) {
    int rc;
    if ((rc = factor_async(h, true))) return rc;
    *did_factor = true;
    h->flight.last_solve = 1;
    h->guard.lu_active = false;
    HIPCHK(h, kkt_backsolve_async(h, h->sol, fused_tail ? &cy : nullptr));
  } else {
    h->flight.last_solve = 2;
    if (h->guard.lu_active)
      HIPCHK(h, lu_solve_async(h->guard.lu, h->rhs, h->sol, 0));
    else
      HIPCHK(h, kkt_solve_async(h, h->rhs, h->sol));
  }
  // Device-resident mode: the residual check of this solve and g, c at the point the step update
  // produces read the same matrices -- one pass over H and two over J for both
  // (launch_residual_and_eval) instead of two and four.  (PGF_EVAL_AHEAD=0: separately, the
  // evaluation at the start of the next step.)
  h->flight.fused_eval_done = false;
  if (ahead) {
    enqueue_step_update(h, /*expand=*/true, &cy);
    ++(fused_tail ? h->dbg.stat_tail_fused : h->dbg.stat_tail_plain);
    if (fused_tail) {
      // a qp step (enqueue_qp_step; it swaps the point right behind): the combine launch besides leaves
      // the new point's residual norm in the status block and the block in h_stat (pgf_solver::hb)
      const bool hand = step_handback() && h->fac.defer_status && h->n + h->m > 0;
      const TailHandback th{h->dt, h->xhat, h->yhat, h->xn, h->yn, h->c, h->lb, h->ub, h->red, h->scal + 1,
                            h->ticket + 1, h->stat, STAT_COPY, h->hb.dev, hand ? ++h->hb.issued : 0ull};
      launch_residual_and_eval_fused(s, h->n, h->m, h->nI, h->delta, h->H, h->ldh, h->J, h->ldj, h->pos, h->mask,
                                     h->rhs, h->sol, h->guard.rs_v, h->guard.rs_lv, h->guard.rs_u, h->guard.rs_wy, h->partial,
                                     PGF_GEMVT_PARTS, h->guard.rs_r, h->guard.rs_red, h->xn, h->yn, h->b, h->q, h->rho, h->c,
                                     h->w, h->tmpn, h->g, hand ? &th : nullptr);
      h->flight.fused_norm_done = hand;
    } else
      launch_residual_and_eval(s, h->n, h->m, h->nI, h->lamb, h->delta, h->H, h->ldh, h->J, h->ldj, h->idxI,
                               h->pos, h->mask, h->rhs, h->sol, h->guard.rs_v, h->guard.rs_lv, h->guard.rs_u, h->guard.rs_wy, h->partial,
                               PGF_GEMVT_PARTS, h->guard.rs_r, h->guard.rs_red, h->xn, h->yn, h->b, h->q, h->rho, h->c, h->w,
                               h->tmpn, h->g, /*prepared=*/true);
    // (a qp step reads the maxima with its whole status block)
    if (!h->fac.defer_status)
      (void)hipMemcpyAsync(h->guard.h_rs, h->guard.rs_red, 3 * sizeof(double), hipMemcpyDeviceToHost, s);
    h->flight.fused_eval_done = true;
    return PGF_OK;
  }
  enqueue_residual(h, !*did_factor);
  enqueue_step_update(h);
  return PGF_OK;
}

int pgf_newton_solve(pgf_handle h, const double *x, const double *y, const double *g,
                     const double *c, int inertia_check, double *dx, double *dy, double *xn,
                     double *yn, double *diff) {
  if (!h) return PGF_INVALID;
  int rc;
  if ((rc = check_ready(h))) return rc;
  if ((h->n && (!x || !g)) || (h->m && (!y || !c))) return fail(h, PGF_INVALID, "null argument");
  (void)hipSetDevice(h->device);
  if ((rc = up(h, h->x, x, h->n * sizeof(double)))) return rc;
  if ((rc = up(h, h->y, y, h->m * sizeof(double)))) return rc;
  if ((rc = up(h, h->g, g, h->n * sizeof(double)))) return rc;
  if ((rc = up(h, h->c, c, h->m * sizeof(double)))) return rc;
  h->eval_fresh = false;
  drop_norm(h);
  if (h->unsym.form) {
    if (inertia_check) return fail(h, PGF_INVALID, "no inertia with an unsymmetric formulation (LU)");
    if ((rc = unsym_step_core(h))) return rc;
    if ((rc = down(h, h->h_scal, h->scal, sizeof(double)))) return rc;
    if (dx && (rc = down(h, dx, h->dx, h->n * sizeof(double)))) return rc;
    if (dy && (rc = down(h, dy, h->dy, h->m * sizeof(double)))) return rc;
    if (xn && (rc = down(h, xn, h->xn, h->n * sizeof(double)))) return rc;
    if (yn && (rc = down(h, yn, h->yn, h->m * sizeof(double)))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (diff) *diff = h->h_scal[0];
    return PGF_OK;
  }
  bool did_factor;
  for (int attempt = 0;; ++attempt) {
    if ((rc = newton_core_async(h, &did_factor))) return rc;
    // (a banded step has enqueued the copy of its own status: band_step_async)
    if (!h->sparse && (rc = down(h, h->h_scal, h->scal, sizeof(double)))) return rc;
    if (did_factor) {
      rc = factor_finish(h);
      if (rc == PGF_RETRY_FACTOR) {  // once more, without the chain's helper workgroups
        if (attempt == 0) continue;
        return fail(h, PGF_HIP_ERROR, k_helper_msg);
      }
      if (rc) return rc;
    } else {
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    break;
  }
  if ((rc = chain_recover(h, false))) return rc;
  if ((rc = refine_if_needed(h, false))) return rc;
  if (inertia_check && h->fac.n_neg != h->m) return fail(h, PGF_INERTIA, "Invalid matrix inertia");
  if (dx && (rc = down(h, dx, h->dx, h->n * sizeof(double)))) return rc;
  if (dy && (rc = down(h, dy, h->dy, h->m * sizeof(double)))) return rc;
  if (xn && (rc = down(h, xn, h->xn, h->n * sizeof(double)))) return rc;
  if (yn && (rc = down(h, yn, h->yn, h->m * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (diff) *diff = h->h_scal[0];
  return PGF_OK;
}

int pgf_residual(pgf_handle h, const double *x, const double *y, const double *g, const double *c,
                 const uint8_t *mask, double *F_out) {
  if (!h) return PGF_INVALID;
  if (!h->outer_set) return fail(h, PGF_NOT_READY, "pgf_set_outer first");
  if ((h->n && (!x || !g)) || (h->m && (!y || !c)) || !F_out)
    return fail(h, PGF_INVALID, "null argument");
  (void)hipSetDevice(h->device);
  int rc;
  // scratch: xn / yn / tmpn / w hold the point so the solver state is untouched
  if ((rc = up(h, h->xn, x, h->n * sizeof(double)))) return rc;
  if ((rc = up(h, h->yn, y, h->m * sizeof(double)))) return rc;
  if ((rc = up(h, h->tmpn, g, h->n * sizeof(double)))) return rc;
  if ((rc = up(h, h->w, c, h->m * sizeof(double)))) return rc;
  if (mask) {
    if ((rc = up(h, h->mask_new, mask, h->n))) return rc;
  } else if (h->unsym.form == PGF_FORM_STANDARD) {
    unsym_mask(h, NAN, h->xn, h->tmpn, h->mask_new);
  } else {
    launch_active_set(h->stream, h->n, 0, h->lamb, 0, 0, 0, h->xhat, h->xn, h->tmpn, h->slb,
                      h->sub, h->mask_new);
  }
  if (h->unsym.form == PGF_FORM_STANDARD) {  // the unscaled residual (ImplicitFunc.value_at)
    launch_unsym_residual_rhs(h->stream, h->unsym.form, h->n, h->m, h->lamb, h->dt, h->fact, h->xhat, h->yhat,
                              h->xn, h->yn, h->tmpn, h->w, h->lb, h->ub, h->mask_new, nullptr, nullptr,
                              h->sol, nullptr);
  } else {
    launch_residual(h->stream, h->n, h->m, h->lamb, h->dt, h->xhat, h->yhat, h->xn, h->yn, h->tmpn,
                    h->w, h->slb, h->sub, h->mask_new, h->sol, nullptr);
  }
  if ((rc = down(h, F_out, h->sol, (size_t)(h->n + h->m) * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PGF_OK;
}

int pgf_qp_set_vectors(pgf_handle h, const double *q, const double *b) {
  if (!h) return PGF_INVALID;
  if ((h->n && !q) || (h->m && !b)) return fail(h, PGF_INVALID, "null argument");
  (void)hipSetDevice(h->device);
  int rc;
  if ((rc = up(h, h->q, q, h->n * sizeof(double)))) return rc;
  if ((rc = up(h, h->b, b, h->m * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->qp_mode = true;
  h->ls.hat_fresh = false;
  drop_norm(h);
  h->unsym.h_has_lag_only = true;
  return PGF_OK;
}

// ---------------------------------------------------------------- device-resident LQ mode
int pgf_qp_set_problem(pgf_handle h, const double *Q, int64_t ldq, const double *q,
                       const double *A, int64_t lda, const double *b, int loc) {
  if (!h) return PGF_INVALID;
  if ((h->n && !q) || (h->m && !b)) return fail(h, PGF_INVALID, "null argument");
  int rc;
  if ((rc = pgf_set_derivs_dense(h, Q, ldq, A, lda, loc))) return rc;
  if (loc == PGF_DEVICE) {
    HIPCHK(h, hipMemcpyAsync(h->q, q, h->n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (h->m)
      HIPCHK(h, hipMemcpyAsync(h->b, b, h->m * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  } else {
    if ((rc = up(h, h->q, q, h->n * sizeof(double)))) return rc;
    if ((rc = up(h, h->b, b, h->m * sizeof(double)))) return rc;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->qp_mode = true;
  h->ls.hat_fresh = false;
  drop_norm(h);
  h->unsym.h_has_lag_only = true;
  return PGF_OK;
}

int pgf_qp_set_point(pgf_handle h, const double *x, const double *y) {
  if (!h) return PGF_INVALID;
  if ((h->n && !x) || (h->m && !y)) return fail(h, PGF_INVALID, "null argument");
  if (h->step_pending && h->ls.active) return fail(h, PGF_NOT_READY, "pgf_qp_sync the line-search step first");
  (void)hipSetDevice(h->device);
  int rc;
  if ((rc = up(h, h->x, x, h->n * sizeof(double)))) return rc;
  if ((rc = up(h, h->y, y, h->m * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->point_set = true;
  h->eval_fresh = false;
  drop_norm(h);
  return PGF_OK;
}

// a read of the point while a speculative step is in flight: the step is settled first (one wait,
// off the production path), so that the point read is never that of a discarded step
static int settle_spec(pgf_handle h, bool *redone);
static int settle_before_read(pgf_handle h) {
  // (a step with PGF_STEP_LINE_SEARCH in flight: the handle's vectors name the outer point's)
  if (h->step_pending && h->ls.active) return fail(h, PGF_NOT_READY, "pgf_qp_sync the line-search step first");
  if (!h->step_pending || !h->flight.spec_pending) return PGF_OK;  // (never speculative on a banded handle)
  HIPCHK(h, hipStreamSynchronize(h->stream));
  bool redone;
  return settle_spec(h, &redone);
}

int pgf_qp_get_point(pgf_handle h, double *x, double *y) {
  if (!h) return PGF_INVALID;
  if (!h->point_set) return fail(h, PGF_NOT_READY, "pgf_qp_set_point first");
  (void)hipSetDevice(h->device);
  int rc;
  if ((rc = settle_before_read(h))) return rc;
  if (x && (rc = down(h, x, h->x, h->n * sizeof(double)))) return rc;
  if (y && (rc = down(h, y, h->y, h->m * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PGF_OK;
}

int pgf_qp_get_mask(pgf_handle h, uint8_t *mask) {
  if (!h || !mask) return PGF_INVALID;
  if (!h->mask_set) return fail(h, PGF_NOT_READY, "no active set");
  (void)hipSetDevice(h->device);
  int rc;
  if ((rc = down(h, mask, h->mask, h->n))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PGF_OK;
}

int pgf_qp_get_direction(pgf_handle h, double *dx, double *dy) {
  if (!h) return PGF_INVALID;
  if (!h->point_set) return fail(h, PGF_NOT_READY, "pgf_qp_set_point first");
  if (h->step_pending) return fail(h, PGF_NOT_READY, "pgf_qp_sync the step first");
  (void)hipSetDevice(h->device);
  int rc;
  if (dx && (rc = down(h, dx, h->dx, h->n * sizeof(double)))) return rc;
  if (dy && (rc = down(h, dy, h->dy, h->m * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PGF_OK;
}

// c = A x - b ; w = rho c + y ; g = Q x + (q + A' w)   at the device point
void qp_eval(pgf_handle h) {
  if (h->eval_fresh) return;
  h->eval_fresh = true;
  if (h->sparse) return band_eval(h);
  hipStream_t s = h->stream;
  launch_gemv_rows(s, h->m, h->n, h->J, h->ldj, h->x, h->b, -1.0, h->c);
  launch_mult_vec(s, h->m, h->rho, h->c, h->y, h->w);
  launch_gemvT(s, h->m, h->n, h->J, h->ldj, h->w, h->q, h->partial, PGF_GEMVT_PARTS, h->tmpn);
  launch_gemv_rows(s, h->n, h->n, h->H, h->ldh, h->x, h->tmpn, 1.0, h->g);
}

static int qp_ready(pgf_handle h) {
  if (!h->qp_mode) return fail(h, PGF_NOT_READY, "pgf_qp_set_problem first");
  if (!h->outer_set) return fail(h, PGF_NOT_READY, "pgf_set_outer first");
  if (!h->point_set) return fail(h, PGF_NOT_READY, "pgf_qp_set_point first");
  return PGF_OK;
}

// mask at the device point -> mask_new; adopt it if it differs (or none yet).  in_step: a step is
// being enqueued (its index-set sizes may be speculative, refresh_index_sets).
static int qp_refresh_mask(pgf_handle h, double tau, bool force, int *changed_out, bool in_step) {
  int use_tau;
  double f_x, f_x0, f_d;
  tau_factors(h, tau, &use_tau, &f_x, &f_x0, &f_d);
  hipStream_t s = h->stream;
  if (!h->sparse && h->unb.no_finite_bound && unbounded_front()) {
    // No finite bound: the mask at ANY point is empty (active_flag compares with -inf and +inf; a
    // NaN compares false).  It, the identity lists and the counts are on the device from the first
    // such call on; the sizes are exact, so the step is never speculative and never redone for them,
    // and its residual and reduced rhs take the multi-workgroup launch (newton_core_async, |A| = 0).
    const bool same = h->mask_set && h->unb.lists_ready;
    if (!h->unb.lists_ready) {
      launch_unbounded_sets(s, h->n, h->mask, h->idxI, h->pos, h->counts);
      h->unb.lists_ready = true;
      h->nI = h->n;
      h->nA = 0;
      h->N = h->n + h->m;
      h->counts_known = true;
    }
    if (changed_out) *changed_out = (force || !same) ? 1 : 0;
    ++h->dbg.stat_unb_fronts;
    if (force || !same) {  // (what adopt_index_sets does for a mask that was re-set)
      h->mask_set = true;
      invalidate_factor(h);
    }
    return PGF_OK;
  }
  ++h->dbg.stat_compactions;
  h->unb.lists_ready = false;
  if (force && !h->sparse) {
    // the mask, straight into h->mask, and its compaction in one launch
    const bool spec = in_step && h->counts_known && step_spec();
    if (changed_out) *changed_out = 1;
    // a step enqueued with |A| = 0: its residual and reduced rhs in the same launch (newton_core_async
    // then enqueues neither; a step that is discarded and redone takes the launches of its own)
    h->flight.front_done = spec && h->nA == 0 && step_fused() && !h->ls.want;  // (its rhs reads the outer point)
    if (h->flight.front_done)
      launch_mask_compact_rhs(s, h->n, h->m, h->nI, use_tau, h->lamb, f_x, f_x0, f_d, h->dt, h->fact, h->xhat,
                              h->yhat, h->x, h->y, h->g, h->c, h->slb, h->sub, h->mask, h->idxI, h->idxA, h->pos,
                              h->counts, h->nI, h->F, h->b0full, h->rhs);
    else
      launch_mask_compact(s, h->n, use_tau, h->lamb, f_x, f_x0, f_d, h->xhat, h->x, h->g, h->slb, h->sub,
                          h->mask, h->idxI, h->idxA, h->pos, h->counts, spec ? h->nI : -1);
    return adopt_index_sets(h, spec);
  }
  launch_active_set(s, h->n, use_tau, h->lamb, f_x, f_x0, f_d, h->xhat, h->x, h->g, h->slb, h->sub,
                    h->mask_new);
  int changed = 1;
  if (h->mask_set && !force) {
    HIPCHK(h, hipMemsetAsync(h->counts + 2, 0, sizeof(int), s));
    launch_mask_diff(s, h->n, h->mask, h->mask_new, h->counts + 2);
    int rc;
    if ((rc = down(h, h->h_counts + 2, h->counts + 2, sizeof(int)))) return rc;
    HIPCHK(h, hipStreamSynchronize(s));
    if (in_step) ++h->dbg.stat_host_syncs;
    changed = h->h_counts[2] != 0;
  }
  if (changed_out) *changed_out = changed;
  if (changed) {
    launch_copy_u8(s, h->mask, h->mask_new, h->n);
    if (h->sparse) {  // full-size banded system: no index sets to rebuild
      h->mask_set = true;
      invalidate_factor(h);
      return PGF_OK;
    }
    return refresh_index_sets(h, in_step);
  }
  return PGF_OK;
}

int pgf_qp_update_active_set(pgf_handle h, double tau, int *changed) {
  if (!h) return PGF_INVALID;
  int rc;
  if ((rc = qp_ready(h))) return rc;
  (void)hipSetDevice(h->device);
  qp_eval(h);
  if (h->unsym.form) return unsym_refresh_mask(h, tau, false, changed, true);
  return qp_refresh_mask(h, tau, false, changed, false);
}

int pgf_qp_advance_outer(pgf_handle h, double dt, double rho) {
  if (!h) return PGF_INVALID;
  int rc;
  if ((rc = qp_ready(h))) return rc;
  if (!(dt > 0.0) || !(rho > 0.0)) return fail(h, PGF_INVALID, "dt and rho must be positive");
  if (h->step_pending && h->ls.active) return fail(h, PGF_NOT_READY, "pgf_qp_sync the line-search step first");
  (void)hipSetDevice(h->device);
  const bool one = step_fused() && !h->sparse;  // the copies and the scaling in one launch
  if (!one) {
    launch_copy(h->stream, h->xhat, h->x, h->n);
    launch_copy(h->stream, h->yhat, h->y, h->m);
  }
  if (rho != h->rho) h->eval_fresh = false;  // g depends on rho
  drop_norm(h);                              // (the norm on the outer point and dt besides)
  set_outer_scalars(h, dt, rho);
  if (one)
    launch_advance_outer(h->stream, h->n, h->m, h->lamb, h->x, h->y, h->lb, h->ub, h->xhat, h->yhat, h->slb,
                         h->sub);
  else
    launch_scale_bounds(h->stream, h->n, h->lamb, h->lb, h->ub, h->slb, h->sub);
  h->mask_set = false;
  h->ls.hat_fresh = false;
  invalidate_factor(h);
  return PGF_OK;
}

// newton_core_async at the device point, (x, y) <- (xn, yn), and the read-back of the step's status:
// dense, ONE copy of the status block (the factorisation's and the chained solve's status words
// are gathered into it by the step update, DenseLdlt::defer_status).
static int enqueue_qp_step(pgf_handle h) {
  h->hb.armed = false;
  drop_norm(h);
  h->hb.t_enqueued = now_s();
  qp_eval(h);
  bool did_factor;
  const bool armed = h->fac.inject_helper_failure != 0;
  h->fac.defer_status = true;  // (read by the dense factorisation and solves only)
  int rc = newton_core_async(h, &did_factor);
  h->fac.defer_status = false;
  h->flight.step_took_inject = armed && !h->fac.inject_helper_failure;
  if (rc) return rc;
  // (PGF_STEP_LINE_SEARCH: the point moves behind the line search, ls_search; g, c stay current)
  if (h->ls.want) return h->sparse ? PGF_OK : down(h, h->h_stat, h->stat, STAT_COPY * sizeof(double));
  swap_point(h);  // (x, y) <- (xn, yn)
  h->eval_fresh = false;
  // g and c at the new point, enqueued NOW: the next step needs them first thing, and behind the
  // step's host synchronisation the four small launches would wait for the host one by one
  // (~35 us of gaps at config 2).  Whatever moves the point afterwards (refinement, a repeated
  // step, pgf_qp_set_point, a new rho) clears eval_fresh again.
  if (h->sparse) return PGF_OK;  // (nothing ahead; band_step_async has enqueued the copy of its status)
  if (h->flight.fused_eval_done) {  // (newton_core_async did it beside the residual check)
    h->eval_fresh = true;
    h->flight.fused_eval_done = false;
  } else if (eval_ahead()) {
    qp_eval(h);
  }
  if (h->flight.fused_norm_done) {  // (the combine launch hands the block back: no copy, hb_wait spins)
    h->flight.fused_norm_done = false;
    h->hb.armed = h->hb.norm_fresh = true;
    return PGF_OK;
  }
  return down(h, h->h_stat, h->stat, STAT_COPY * sizeof(double));
}

// What the two redo paths share (settle_spec: index-set sizes mismatched; pgf_qp_sync: the chain's
// helpers failed their hand-over): the step in flight is discarded and enqueued again from the
// point it started at.  Each path does the bookkeeping of its own in front of this.
static int redo_step(pgf_handle h) {
  if (!h->ls.want) swap_point(h);
  h->eval_fresh = false;  // (g, c were evaluated ahead at the point that is discarded)
  drop_norm(h);
  return enqueue_qp_step(h);
}

// A step in flight that was enqueued with speculative index-set sizes, after a host
// synchronisation that brought its status block: if the compaction found other sizes, the step
// ran with the previous |I|, |A| and its factor, flags and point are garbage (every index it read
// was in range).  Nothing of it is reported or acted on -- no PGF_SINGULAR, no refinement, no
// change of condensed_veto, no switching off of the chain helpers or the chained solves (a
// chained solve's half-published state is only reset) -- and it is enqueued again from the
// point it started at, with the true sizes.  *redone: it was.  (For a step that is pending only:
// pgf_qp_sync has just cleared that, settle_before_read and pgf_qp_residual_norm test it.)
static int settle_spec(pgf_handle h, bool *redone) {
  *redone = false;
  if (!h->flight.spec_pending) return PGF_OK;  // (never speculative on a banded handle)
  h->flight.spec_pending = false;
  if (!h->h_counts[3]) return PGF_OK;
  ++h->dbg.stat_redone;
  const int *w = reinterpret_cast<const int *>(h->h_stat + 14);
  ldlt_chain_discard(h->fac, (h->flight.stat_bits & 2) ? w[3] : 0);
  h->flight.stat_bits = 0;  // (the discarded step's status words are not read)
  // a test hook's injected helper failure belongs to the step that is kept
  if (h->flight.step_took_inject) h->fac.inject_helper_failure = 1;
  gram_uncount(h);
  h->fac.factored = false;
  h->guard.lu_active = false;
  adopt_counts(h);
  int rc;
  if ((rc = redo_step(h))) return rc;
  *redone = true;
  return PGF_OK;
}

int pgf_qp_step_async(pgf_handle h, unsigned policy, double tau) {
  if (!h) return PGF_INVALID;
  int rc;
  if ((rc = qp_ready(h))) return rc;
  if (h->step_pending) return fail(h, PGF_NOT_READY, "pgf_qp_sync the previous step first");
  (void)hipSetDevice(h->device);
  const bool ls = (policy & PGF_STEP_LINE_SEARCH) != 0;
  if (ls && (policy & ~PGF_STEP_LINE_SEARCH) != (PGF_STEP_RECOMPUTE_MASK | PGF_STEP_REFACTOR))
    return fail(h, PGF_INVALID,
                "PGF_STEP_LINE_SEARCH goes with PGF_STEP_RECOMPUTE_MASK | PGF_STEP_REFACTOR only");
  if (ls && h->unsym.form)
    return fail(h, PGF_INVALID, "PGF_STEP_LINE_SEARCH: the Symmetric formulation only");
  if (h->unsym.form) return unsym_qp_step_async(h, policy, tau);
  // an error on the way: the handle's vectors are its own again, no step carries the bit
  auto drop = [h](int code) {
    ls_leave(h);
    h->ls.want = false;
    return code;
  };
  h->ls.want = ls;
  h->flight.front_done = false;
  qp_eval(h);
  if (policy & PGF_STEP_RECOMPUTE_MASK) {
    // Full (newton.py:83-89), Globalized (:239-242): the mask is always re-set, which drops the
    // factor; ActiveSet (:203-215): only when it differs elementwise.
    const bool force = (policy & PGF_STEP_REFACTOR) != 0;
    if ((rc = qp_refresh_mask(h, tau, force, nullptr, true))) return drop(rc);
  }
  if (!h->mask_set) return drop(fail(h, PGF_NOT_READY, "no active set: pgf_qp_update_active_set first"));
  if (policy & PGF_STEP_REFACTOR) invalidate_factor(h);
  if (ls && (rc = ls_enter(h))) return drop(rc);
  if ((rc = enqueue_qp_step(h))) return drop(rc);
  h->step_pending = true;
  return PGF_OK;
}

// the Newton step in flight, settled: its status, the redo paths, the accuracy guard
static int qp_sync_step(pgf_handle h, int *n_neg, double *diff) {
  if (!h) return PGF_INVALID;
  if (!h->step_pending) return fail(h, PGF_NOT_READY, "no step pending");
  h->step_pending = false;
  (void)hipSetDevice(h->device);
  if (h->unsym.form) return unsym_qp_sync(h, n_neg, diff);
  hipError_t e;
  int rc;
  bool awaited = false;
  if ((rc = band_status_sync(h))) return rc;
  if (!h->sparse) {
    // the step's one wait: its status block (hb_wait: none, if pgf_qp_residual_norm has taken it)
    if ((rc = hb_wait(h, &awaited))) return rc;
    ++h->dbg.stat_host_syncs;
    bool redone;
    if ((rc = settle_spec(h, &redone))) return rc;
    if (redone) {
      if ((rc = hb_wait(h, &awaited))) return rc;
      ++h->dbg.stat_host_syncs;
    }
    absorb_status(h);
  }
  int st = finish_factor_state(h, &e, awaited);  // flags are only rewritten by a factor launch
  if (st == 2) {
    // the chain's helper workgroups failed their checks (off now): the step is computed again
    // from the point it started at
    if ((rc = redo_step(h))) return rc;
    if (!h->sparse) {
      if ((rc = hb_wait(h, &awaited))) return rc;
      ++h->dbg.stat_host_syncs;
      absorb_status(h);
    }
    st = finish_factor_state(h, &e, awaited);
    if (st == 2) return fail(h, PGF_HIP_ERROR, k_helper_msg);
  }
  if (st < 0) return hip_fail(h, e, "step");
  if (st == 1) {
    // large border: the discarded step's point goes back (its solve phase ran on a factor of S that
    // does not exist; the other routes leave the new point, as they always have)
    if (h->sparse && sp_border_large(h->sp) && !h->ls.want) {
      swap_point(h);
      h->eval_fresh = false;
    }
    return fail(h, PGF_SINGULAR, "zero or non-finite pivot in LDL^T of the KKT matrix");
  }
  // (swapped: (x, y) is already the new point -- not with PGF_STEP_LINE_SEARCH, whose point moves later)
  if ((rc = chain_recover(h, !h->ls.want))) return rc;
  if ((rc = refine_if_needed(h, !h->ls.want))) return rc;
  if (n_neg) *n_neg = h->fac.n_neg;
  if (diff) *diff = h->h_scal[0];
  return PGF_OK;
}

// With PGF_STEP_LINE_SEARCH the settled step is the direction: the line-search launches follow it
// and one further wait brings their block -- a fixed number of waits whatever the trial count.
int pgf_qp_sync(pgf_handle h, int *n_neg, double *diff) {
  const bool ls = h && h->step_pending && h->ls.want;
  int rc = qp_sync_step(h, n_neg, diff);
  if (!ls) return rc;
  ls_leave(h);
  h->ls.want = false;
  if (rc) return rc;
  return ls_search(h, diff);
}

int pgf_qp_step(pgf_handle h, unsigned policy, double tau, int inertia_check, int *n_neg,
                double *diff) {
  int rc;
  if (h && h->unsym.form && inertia_check)
    return fail(h, PGF_INVALID, "no inertia with an unsymmetric formulation (LU)");
  if ((rc = pgf_qp_step_async(h, policy, tau))) return rc;
  if ((rc = pgf_qp_sync(h, n_neg, diff))) return rc;
  if (!h->unsym.form && inertia_check && h->fac.n_neg != h->m)
    return fail(h, PGF_INERTIA, "Invalid matrix inertia");
  return PGF_OK;
}

int pgf_qp_residual_norm(pgf_handle h, double *norm_out, double *norm_out_dev) {
  if (!h) return PGF_INVALID;
  int rc;
  if ((rc = qp_ready(h))) return rc;
  if (h->step_pending && h->ls.active) return fail(h, PGF_NOT_READY, "pgf_qp_sync the line-search step first");
  (void)hipSetDevice(h->device);
  qp_eval(h);
  // (the norm also reaches norm_out_dev from the launch itself).  Between pgf_qp_step_async and
  // pgf_qp_sync the point is that of the step in flight; if that step turns out to have run with
  // stale index-set sizes (settle_spec), it is redone and the norm taken again at its new point.
  for (int pass = 0; pass < 2; ++pass) {
    if (h->hb.norm_fresh) {
      // The tail's last launch left this point's norm in the status block (bit for bit what the
      // launch below gives) and the block in h_stat.  A device slot: one workgroup stores the norm
      // there and hands the block back again behind it -- the slot is written before the word the
      // host waits for, so another stream may read it as soon as this returns.
      if (norm_out_dev)
        launch_handback_store(h->stream, h->stat, STAT_COPY, STAT_NORM, h->hb.dev, ++h->hb.issued, norm_out_dev);
      if ((rc = hb_wait(h))) return rc;
      bool redone = false;
      if (h->step_pending && (rc = settle_spec(h, &redone))) return rc;
      if (!redone) break;
      qp_eval(h);
      continue;
    }
    launch_unscaled_res_norm(h->stream, h->n, h->m, h->dt, h->xhat, h->yhat, h->x, h->y, h->g, h->c,
                             h->lb, h->ub, h->red, h->scal + 1, norm_out_dev, h->ticket + 1);
    if ((rc = down(h, h->h_scal + 1, h->scal + 1, sizeof(double)))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    bool redone = false;
    if (h->step_pending && (rc = settle_spec(h, &redone))) return rc;
    if (!redone) break;
    qp_eval(h);
  }
  if (norm_out) *norm_out = h->h_scal[1];
  return PGF_OK;
}

int pgf_qp_measures(pgf_handle h, double active_tol, double *out) {
  if (!h || !out) return PGF_INVALID;
  if (!h->qp_mode || !h->point_set || !h->bounds_set)
    return fail(h, PGF_NOT_READY, "pgf_set_bounds, pgf_qp_set_problem, pgf_qp_set_point first");
  (void)hipSetDevice(h->device);
  int rc0;
  if ((rc0 = settle_before_read(h))) return rc0;
  hipStream_t s = h->stream;
  const int n = h->n, m = h->m;
  // c = A x - b and r = Q x + q + A'y (no rho term: iterate.py:141, 176)
  launch_copy(s, h->w, h->y, m);
  if (h->sparse) {
    band_measures_eval(h);
  } else {
    launch_gemv_rows(s, m, n, h->J, h->ldj, h->x, h->b, -1.0, h->c);
    launch_gemvT(s, m, n, h->J, h->ldj, h->w, h->q, h->partial, PGF_GEMVT_PARTS, h->tmpn);
    launch_gemv_rows(s, n, n, h->H, h->ldh, h->x, h->tmpn, 1.0, h->F);
  }
  const int nb = (n + m + 255) / 256;
  double *res = h->meas + 4 * nb;
  launch_measures(s, n, m, active_tol, h->x, h->y, h->F, h->c, h->lb, h->ub, h->meas, res);
  int rc;
  if ((rc = down(h, h->h_meas, res, 4 * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(s));
  std::memcpy(out, h->h_meas, 4 * sizeof(double));
  return PGF_OK;
}
