// The Globalized policy on the device-resident LQ handles (PGF_STEP_LINE_SEARCH; reference
// newton.py:218-304): what pgf_qp_step_async and pgf_qp_sync (pgf_api_step.hip) do in front of and
// behind the Newton step they share with the Full policy.  The step's residual, right-hand side
// and update read the OUTER point (step_solver.solve(self.orig_iterate), newton.py:248): while
// such a step is in flight the handle's (x, y, g, c) name the outer point's vectors (ls_enter /
// ls_leave), so the dense and the banded step, their guard and their redo paths run unchanged.
// Behind the settled step: the direction's images, k_ls_ladder, k_ls_finish and one wait for the
// line search's block.  Host code only.
#include <cstring>

#include "pgf_api_internal.h"
#include "pgf_kernels.h"
#include "pgf_line_search.h"

// the line search's vectors, on the first Globalized step of the handle (or when it joins a batch
// created with PGF_BATCH_LINE_SEARCH)
int ls_reserve(pgf_handle h) {
  auto &ls = h->ls;
  if (ls.blk) return PGF_OK;
  const int n = h->n, m = h->m, nb = (n + m + 255) / 256;
  HIPCHK(h, dalloc(&ls.ghat, (size_t)n));
  HIPCHK(h, dalloc(&ls.chat, (size_t)m));
  HIPCHK(h, dalloc(&ls.v, (size_t)n));
  HIPCHK(h, dalloc(&ls.u, (size_t)m));
  HIPCHK(h, dalloc(&ls.zero, (size_t)(n > m ? n : m)));
  HIPCHK(h, dalloc(&ls.red, (size_t)LS_TERMS * (nb + 1)));
  HIPCHK(h, hipHostMalloc((void **)&ls.h_blk, LS_COPY * sizeof(double)));
  HIPCHK(h, hipMemsetAsync(ls.zero, 0, (size_t)(n > m ? n : m) * sizeof(double), h->stream));
  HIPCHK(h, dalloc(&ls.blk, (size_t)LS_ALLOC));
  HIPCHK(h, hipMemsetAsync(ls.blk, 0, LS_ALLOC * sizeof(double), h->stream));  // (the tickets start at zero)
  std::memset(ls.h_blk, 0, LS_COPY * sizeof(double));
  return PGF_OK;
}

void ls_free(pgf_handle h) {
  auto &ls = h->ls;
  for (double *p : {ls.ghat, ls.chat, ls.v, ls.u, ls.zero, ls.red, ls.blk})
    if (p) (void)hipFree(p);
  if (ls.h_blk) (void)hipHostFree(ls.h_blk);
  if (ls.ev0) (void)hipEventDestroy(ls.ev0);
  if (ls.ev1) (void)hipEventDestroy(ls.ev1);
}

// (x, y, g, c) of the handle <-> the outer point's vectors
static void ls_exchange(pgf_handle h) {
  auto &ls = h->ls;
  std::swap(h->x, ls.ox);
  std::swap(h->y, ls.oy);
  std::swap(h->g, ls.og);
  std::swap(h->c, ls.oc);
}

// In front of enqueue_qp_step (g, c at the device point and its mask are enqueued): g, c at the
// outer point -- once per outer step, qp_eval's own launches on the exchanged vectors -- and the
// exchange.
void ls_enter_names(pgf_handle h) {
  auto &ls = h->ls;
  ls.ox = h->xhat;
  ls.oy = h->yhat;
  ls.og = ls.ghat;
  ls.oc = ls.chat;
  ls_exchange(h);
  ls.active = true;
}

int ls_enter(pgf_handle h) {
  int rc;
  if ((rc = ls_reserve(h))) return rc;
  auto &ls = h->ls;
  ls_enter_names(h);
  if (!ls.hat_fresh) {
    h->eval_fresh = false;
    drop_norm(h);
    qp_eval(h);
    ls.hat_fresh = true;
  }
  h->eval_fresh = true;  // (both pairs are current; qp_eval inside the step has nothing to do)
  return PGF_OK;
}

void ls_leave(pgf_handle h) {
  if (!h->ls.active) return;
  ls_exchange(h);
  h->ls.active = false;
}

// Behind a settled step (its direction in h->dx, h->dy, the clipped one against the outer point):
// u = A dx, v = Q dx + A'(rho u + dy) -- qp_eval's / band_measures_eval's products with zero q and
// b, one pass over H --, the ladder, the new point, one wait.  On PGF_OK (x, y) <- (xn, yn).
int ls_search(pgf_handle h, double *diff) {
  auto &ls = h->ls;
  hipStream_t s = h->stream;
  const int n = h->n, m = h->m;
  qp_eval(h);  // (a no-op unless the guard recomputed the step: g, c at the device point)
  // while profiling is enabled: the device time of the stage (pgf_debug_line_search_ms)
  const bool timed = h->prof.enabled;
  if (timed && !ls.ev0) {
    HIPCHK(h, hipEventCreate(&ls.ev0));
    HIPCHK(h, hipEventCreate(&ls.ev1));
  }
  if (timed) (void)hipEventRecord(ls.ev0, s);
  if (h->sparse) {
    const SparseDev &sp = h->sp;
    sp_launch_spmv(s, m, sp.pat.Jptr, sp.pat.Jcol, sp.pat.Jval, h->dx, ls.zero, 1.0, ls.u);
    launch_mult_vec(s, m, h->rho, ls.u, h->dy, h->w);
    sp_launch_spmvT(s, n, sp.pat.JTptr, sp.pat.JTrow, sp.pat.JTmap, sp.pat.Jval, h->w, ls.zero, h->tmpn);
    sp_launch_spmv(s, n, sp.pat.Hptr, sp.pat.Hcol, sp.pat.Hval, h->dx, h->tmpn, 1.0, ls.v);
  } else {
    launch_gemv_rows(s, m, n, h->J, h->ldj, h->dx, ls.zero, 1.0, ls.u);
    launch_mult_vec(s, m, h->rho, ls.u, h->dy, h->w);
    launch_gemvT(s, m, n, h->J, h->ldj, h->w, ls.zero, h->partial, PGF_GEMVT_PARTS, h->tmpn);
    launch_gemv_rows(s, n, n, h->H, h->ldh, h->dx, h->tmpn, 1.0, ls.v);
  }
  launch_ls_ladder(s, n, m, h->lamb, ls.newton_tol, h->x, h->y, h->xhat, h->yhat, h->dx, h->dy, h->g, h->c,
                   ls.v, ls.u, h->slb, h->sub, ls.red, ls.blk);
  launch_ls_finish(s, n, m, h->xhat, h->yhat, h->dx, h->dy, h->lb, h->ub, h->xn, h->yn, ls.red, ls.blk);
  if (timed) (void)hipEventRecord(ls.ev1, s);
  int rc;
  if ((rc = down(h, ls.h_blk, ls.blk, LS_COPY * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(s));
  ++h->dbg.stat_host_syncs;
  float ms = 0.f;
  if (timed && hipEventElapsedTime(&ms, ls.ev0, ls.ev1) == hipSuccess) ls.stage_ms = ms;
  if (n + m == 0) ls.h_blk[LS_ALPHA] = 1.0;
  ls.have_stats = true;
  if (ls.h_blk[LS_STATUS] != 0.0) return fail(h, PGF_LINE_SEARCH, "Line search failed to converge");
  swap_point(h);
  h->eval_fresh = false;
  drop_norm(h);
  h->h_scal[0] = ls.h_blk[LS_DIFF];
  if (diff) *diff = ls.h_blk[LS_DIFF];
  return PGF_OK;
}

extern "C" {

int pgf_qp_set_line_search(pgf_handle h, double newton_tol) {
  if (!h) return PGF_INVALID;
  if (!(newton_tol >= 0.0)) return fail(h, PGF_INVALID, "newton_tol must not be negative");
  h->ls.newton_tol = newton_tol;
  return PGF_OK;
}

int pgf_qp_line_search_stats(pgf_handle h, double *alpha, int *trials, double *merit0, double *slope,
                             double *trial_merits) {
  if (!h) return PGF_INVALID;
  if (!h->ls.have_stats) return fail(h, PGF_NOT_READY, "no step with PGF_STEP_LINE_SEARCH yet");
  const double *b = h->ls.h_blk;
  if (alpha) *alpha = b[LS_ALPHA];
  if (trials) *trials = (int)b[LS_NTRIALS];
  if (merit0) *merit0 = b[LS_MERIT0];
  if (slope) *slope = b[LS_SLOPE];
  if (trial_merits) std::memcpy(trial_merits, b + LS_MERITS, LS_TRIALS * sizeof(double));
  return PGF_OK;
}

int pgf_debug_line_search_ms(pgf_handle h, double *ms) {
  if (!h || !ms) return PGF_INVALID;
  *ms = h->ls.stage_ms;
  return PGF_OK;
}

}  // extern "C"
