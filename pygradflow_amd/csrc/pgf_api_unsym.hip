// The unsymmetric formulations behind the C ABI: their entry points and the halves of the step,
// factor and mask functions of the dense handle's files that run when pgf_set_formulation chose one
// (pgf_api_internal.h lists them).
#include <cmath>
#include <utility>

#include "pgf_api_internal.h"
#include "pgf_kernels.h"
#include "pgf_unsym.h"

// ---------------------------------------------------------------- unsymmetric formulations
// Standard / Extended / Asymmetric (pgf_set_formulation): the same Newton step through the
// (n + m) x (n + m) matrix of the reference's alternative step solvers, assembled in HBM from the
// resident H, J, mask and index lists (pgf_unsym.hip) straight into the array the pivoted LU
// factorises in place.  The system always has n + m rows: no size depends on |I|, the kernels read
// |A| on the device, so a step needs no host synchronisation for the index sets -- the one wait
// inside a factorising step is lu_factor's own (it reads its pivots).  No LDL^T, no inertia
// (n_neg = -1, LUSolver.num_neg_eigvals() is None), no accuracy guard: the LU pivots.
static const double *unsym_lo(pgf_handle h) { return h->unsym.form == PGF_FORM_STANDARD ? h->lb : h->slb; }
static const double *unsym_hi(pgf_handle h) { return h->unsym.form == PGF_FORM_STANDARD ? h->ub : h->sub; }

// Device-resident Standard linearises with aug_lag_deriv_xx(rho) = H + rho J^T J: the Gram matrix
// the condensed LDL^T keeps per derivative upload (gram_build) -- never rebuilt per step.
static int unsym_gram(pgf_handle h, const double **G) {
  *G = nullptr;
  if (h->unsym.form != PGF_FORM_STANDARD || !h->unsym.h_has_lag_only || h->m == 0 || h->n == 0) return PGF_OK;
  if (!h->cond.gram_valid) {
    HIPCHK(h, condensed_reserve(h));
    if (h->cond.gram_off || !gram_build(h))
      return fail(h, PGF_HIP_ERROR, "Standard formulation: the Gram matrix J^T J could not be built");
  }
  *G = h->cond.G;
  return PGF_OK;
}

static int unsym_assemble(pgf_handle h, double *M, int64_t ld) {
  const double *G;
  int rc;
  if ((rc = unsym_gram(h, &G))) return rc;
  launch_assemble_unsym(h->stream, h->unsym.form, M, ld, h->n, h->m, h->H, h->ldh, h->J, h->ldj, G, h->cond.ldg,
                        h->rho, h->mask, h->idxI, h->idxA, h->counts, h->dt, h->lamb, h->delta);
  return PGF_OK;
}

// assemble + factorise (waits: lu_factor reads its pivots)
int unsym_factor(pgf_handle h) {
  const int Nf = h->n + h->m;
  if (!h->unsym.ulu.A) {
    const hipError_t ea = lu_alloc(h->unsym.ulu, Nf, h->stream);
    if (ea != hipSuccess) {
      lu_free(h->unsym.ulu);  // (nothing half allocated stays behind)
      return hip_fail(h, ea, "lu_alloc");
    }
  }
  h->unsym.ulu_ok = false;
  int rc;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (h->prof.enabled) {
    e0 = prof_event(&h->prof);
    e1 = prof_event(&h->prof);
    (void)hipEventRecord(e0, h->stream);
  }
  rc = unsym_assemble(h, h->unsym.ulu.A, h->unsym.ulu.ld);
  if (e0) (void)hipEventRecord(e1, h->stream);
  hipError_t e = hipSuccess;
  const int st = rc ? 0 : lu_factor(h->unsym.ulu, &e);  // (waits for the stream)
  if (e0) {
    float ms = 0.f;
    if (!rc && st >= 0 && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) {
      h->unsym.acc_unsym_asm_ms += ms;
      ++h->unsym.acc_unsym_asm_launches;
    }
    h->prof.pool.push_back(e0);
    h->prof.pool.push_back(e1);
  }
  if (rc) return rc;
  ++h->dbg.stat_unsym_asm;
  if (st < 0) return hip_fail(h, e, "LU of the Newton matrix");
  ++h->dbg.stat_unsym_lu;
  if (st == 1) return fail(h, PGF_SINGULAR, "zero or non-finite pivot in the LU of the Newton matrix");
  h->unsym.ulu_ok = true;
  return PGF_OK;
}

// the mask at (x, g) into `out' (Standard: unscaled)
void unsym_mask(pgf_handle h, double tau, const double *x, const double *g, uint8_t *out) {
  int use_tau;
  double f_x, f_x0, f_d;
  tau_factors(h, tau, &use_tau, &f_x, &f_x0, &f_d);
  if (h->unsym.form == PGF_FORM_STANDARD)
    launch_unscaled_active_set(h->stream, h->n, use_tau, h->dt, use_tau ? 1.0 - tau * h->lamb : 0.0,
                               use_tau ? tau * h->lamb : 0.0, use_tau ? tau : 0.0, h->xhat, x, g, h->lb,
                               h->ub, out);
  else
    launch_active_set(h->stream, h->n, use_tau, h->lamb, f_x, f_x0, f_d, h->xhat, x, g, h->slb, h->sub, out);
}

// residual, right-hand side, (factorisation,) solve and step update for the point in
// (h->x, h->y, h->g, h->c); scal[0] <- the step length.  Enqueued, except for lu_factor's wait.
int unsym_step_core(pgf_handle h) {
  hipStream_t s = h->stream;
  h->flight.fused_eval_done = false;
  launch_unsym_residual_rhs(s, h->unsym.form, h->n, h->m, h->lamb, h->dt, h->fact, h->xhat, h->yhat, h->x, h->y,
                            h->g, h->c, unsym_lo(h), unsym_hi(h), h->mask, h->pos, h->counts, h->F, h->rhs);
  int rc;
  if (!h->unsym.ulu_ok && (rc = unsym_factor(h))) return rc;
  HIPCHK(h, lu_solve_async(h->unsym.ulu, h->rhs, h->sol, 0));
  launch_unsym_step_update(s, h->unsym.form, h->n, h->m, h->fact, h->rho, h->x, h->y, h->lb, h->ub, h->F, h->sol,
                           h->dx, h->dy, h->xn, h->yn, h->red);
  launch_final_reduce(s, h->red, (h->n + h->m + 255) / 256, h->scal, 1);
  return PGF_OK;
}

// mask at the device point; adopted (index lists rebuilt, factor dropped) when forced, when there
// is none yet, or when it differs.  The sizes of the index sets are not awaited (wait_counts: they
// are, outside a step).
int unsym_refresh_mask(pgf_handle h, double tau, bool force, int *changed_out, bool wait_counts) {
  hipStream_t s = h->stream;
  unsym_mask(h, tau, h->x, h->g, h->mask_new);
  int changed = 1;
  int rc;
  if (h->mask_set && !force) {
    HIPCHK(h, hipMemsetAsync(h->counts + 2, 0, sizeof(int), s));
    launch_mask_diff(s, h->n, h->mask, h->mask_new, h->counts + 2);
    if ((rc = down(h, h->h_counts + 2, h->counts + 2, sizeof(int)))) return rc;
    HIPCHK(h, hipStreamSynchronize(s));
    if (!wait_counts) ++h->dbg.stat_host_syncs;
    changed = h->h_counts[2] != 0;
  }
  if (changed_out) *changed_out = changed;
  if (!changed) return PGF_OK;
  launch_copy_u8(s, h->mask, h->mask_new, h->n);
  launch_compact(s, h->n, h->mask, h->idxI, h->idxA, h->pos, h->counts, -1);
  h->mask_set = true;
  invalidate_factor(h);
  if (wait_counts) {
    if ((rc = down(h, h->h_counts, h->counts, 2 * sizeof(int)))) return rc;
    HIPCHK(h, hipStreamSynchronize(s));
    adopt_counts(h);
  } else {
    h->counts_known = false;  // (they arrive with the step's status block, pgf_qp_sync)
  }
  return PGF_OK;
}

int unsym_qp_step_async(pgf_handle h, unsigned policy, double tau) {
  int rc;
  qp_eval(h);
  if (policy & PGF_STEP_RECOMPUTE_MASK) {
    const bool force = (policy & PGF_STEP_REFACTOR) != 0;
    if ((rc = unsym_refresh_mask(h, tau, force, nullptr, false))) return rc;
  }
  if (!h->mask_set) return fail(h, PGF_NOT_READY, "no active set: pgf_qp_update_active_set first");
  if (policy & PGF_STEP_REFACTOR) invalidate_factor(h);
  if ((rc = unsym_step_core(h))) return rc;
  swap_point(h);
  h->eval_fresh = false;
  drop_norm(h);
  if ((rc = down(h, h->h_stat, h->stat, STAT_COPY * sizeof(double)))) return rc;
  h->step_pending = true;
  return PGF_OK;
}

int unsym_qp_sync(pgf_handle h, int *n_neg, double *diff) {
  HIPCHK(h, hipStreamSynchronize(h->stream));
  ++h->dbg.stat_host_syncs;
  adopt_counts(h);
  if (n_neg) *n_neg = -1;
  if (diff) *diff = h->h_scal[0];
  return PGF_OK;
}

int pgf_set_formulation(pgf_handle h, int form) {
  if (!h) return PGF_INVALID;
  if (h->sparse) return fail(h, PGF_INVALID, "pgf_set_formulation: dense handles only");
  if (form < PGF_FORM_SYMMETRIC || form > PGF_FORM_ASYMMETRIC)
    return fail(h, PGF_INVALID, "pgf_set_formulation: unknown formulation");
  if (h->step_pending) return fail(h, PGF_NOT_READY, "pgf_qp_sync the step in flight first");
  h->unsym.form = form;
  invalidate_factor(h);
  h->unb.lists_ready = false;  // (the unsymmetric steps write the mask and the lists their own way)
  drop_norm(h);
  // a handle that goes back to Symmetric gives the (n + m) x ld array of its LU back
  if (form == PGF_FORM_SYMMETRIC && h->unsym.ulu.A) {
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    lu_free(h->unsym.ulu);
  }
  return PGF_OK;
}

int pgf_get_newton_matrix(pgf_handle h, double *M_out, int64_t ld) {
  if (!h) return PGF_INVALID;
  if (!h->unsym.form) return fail(h, PGF_INVALID, "pgf_get_newton_matrix: pgf_set_formulation first");
  int rc;
  if ((rc = check_ready(h))) return rc;
  const int Nf = h->n + h->m;
  if (Nf == 0) return PGF_OK;
  if (!M_out || ld < Nf) return fail(h, PGF_INVALID, "bad output matrix");
  (void)hipSetDevice(h->device);
  double *tmp = nullptr;
  HIPCHK(h, dalloc(&tmp, (size_t)Nf * Nf));
  rc = unsym_assemble(h, tmp, Nf);
  hipError_t e = hipSuccess;
  if (!rc) {
    e = hipMemcpy2DAsync(M_out, (size_t)ld * sizeof(double), tmp, (size_t)Nf * sizeof(double),
                         (size_t)Nf * sizeof(double), Nf, hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  } else {
    (void)hipStreamSynchronize(h->stream);
  }
  (void)hipFree(tmp);
  if (rc) return rc;
  if (e != hipSuccess) return hip_fail(h, e, "pgf_get_newton_matrix");
  return PGF_OK;
}

int pgf_debug_unsym_stats(pgf_handle h, int *assemblies, int *lu_factorisations,
                          int64_t *matrix_bytes_from_host) {
  if (!h) return PGF_INVALID;
  if (assemblies) *assemblies = h->dbg.stat_unsym_asm;
  if (lu_factorisations) *lu_factorisations = h->dbg.stat_unsym_lu;
  if (matrix_bytes_from_host) *matrix_bytes_from_host = h->dbg.stat_unsym_bytes;
  return PGF_OK;
}

int pgf_debug_unsym_note_upload(pgf_handle h, int64_t bytes) {
  if (!h || bytes < 0) return PGF_INVALID;
  h->dbg.stat_unsym_bytes += bytes;
  return PGF_OK;
}
