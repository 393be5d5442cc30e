// The accuracy guard of the dense Symmetric handle: the residual of every solve, its measure,
// iterative refinement, the pivoted LU that takes over when refinement does not converge
// (refine_if_needed), and the recovery from a chained solve that failed its checks
// (chain_recover); pgf_set_refinement and pgf_refinement_stats.  Host code only.
#include <cmath>

#include "pgf_api_internal.h"
#include "pgf_kernels.h"

// r = rhs - K s of the solve just enqueued, with K applied from H, J and the mask (the factor
// overwrote the assembled matrix); the three maxima reach the host with the next sync
void enqueue_residual(pgf_handle h, bool may_skip) {
  if (!h->guard.refine_mode) return;
  h->guard.rs_skipped = may_skip && h->guard.factor_clean;
  if (h->guard.rs_skipped) return;
  launch_kkt_residual(h->stream, h->n, h->m, h->nI, h->lamb, h->delta, h->H, h->ldh, h->J, h->ldj,
                      h->idxI, h->pos, h->mask, h->rhs, h->sol, h->guard.rs_v, h->guard.rs_lv, h->guard.rs_u, h->guard.rs_wy,
                      h->partial, PGF_GEMVT_PARTS, h->guard.rs_r, h->guard.rs_red);
  (void)hipMemcpyAsync(h->guard.h_rs, h->guard.rs_red, 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream);
}

// The measure of a solve: max |rhs - K s| against max |rhs| -- and, once the matrices' norms are
// known (residual_norms), against ||K|| max |s| + max |rhs|: the normwise backward error.  A
// backward-stable solve only guarantees |r| <~ eps ||K|| ||s||, which is eps cond(K) ||rhs||: at
// cond(K) ~ 1e5 and beyond the first form alone would send good solves into refinement, and at
// ~1e9 not even the pivoted LU could meet it -- the reference's splu accepts those solves
// (lu_solver.py:14-21).  ||K||_inf <= max(||H||_inf + lambda + ||J||_1, ||J||_inf + delta): the
// reduced matrix is a principal submatrix of that one.
static double residual_rel(pgf_handle h) {
  const double r = h->guard.h_rs[0], b = h->guard.h_rs[1], sn = h->guard.h_rs[2];
  if (!(r == r) || !(r <= 1.79e308)) return HUGE_VAL;
  double den = b;
  if (h->guard.norms_valid) {
    const double nK = std::max(h->guard.h_rs[4] + h->lamb + h->guard.h_rs[6], h->guard.h_rs[5] + h->delta);
    if (sn == sn && sn <= 1.79e308) den += nK * sn;
  }
  return r / (den > 0.0 ? den : 1.0);
}
// the norms of H and J in HBM (one pass over both, one synchronisation; cached until the next
// pgf_set_derivs_*)
int residual_norms(pgf_handle h) {
  if (h->guard.norms_valid) return PGF_OK;
  launch_matrix_norms(h->stream, h->n, h->m, h->H, h->ldh, h->J, h->ldj, h->guard.rs_red + 4);
  HIPCHK(h, hipMemcpyAsync(h->guard.h_rs + 4, h->guard.rs_red + 4, 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->guard.norms_valid = true;
  return PGF_OK;
}

// After a host synchronisation (and chain_recover): the unpivoted LDL^T is backward stable only
// while the reduced KKT matrix is quasi-definite and not too ill-conditioned -- with an
// indefinite H[I,I] + lambda I (non-convex problems at large dt) element growth is unbounded,
// and the reference's pivoted LU (lu_solver.py:14) has no such limit.  The residual of every
// solve is therefore checked, max |rhs - K s| <= refine_tol max |rhs|; beyond that up to two
// steps of iterative refinement with the same factor, and if they do not get below
// refine_fail either, the reduced matrix is assembled once more and factorised by the LU with
// partial pivoting of pgf_lu.hip (kept for the back-solve steps that follow).  Only when that
// fails too does the call report PGF_SINGULAR -> LinearSolverError -> the step controller's
// reject-and-halve path.
int refine_if_needed(pgf_handle h, bool swapped, bool with_step) {
  if (h->sparse) return band_refine(h, swapped, with_step);
  if (!h->guard.refine_mode || h->N == 0 || h->guard.rs_skipped) return PGF_OK;
  double rel = residual_rel(h);
  int rc;
  if (rel > h->guard.refine_tol && !h->guard.norms_valid) {
    // missed against max |rhs| alone: take the size of K and of the solution into account
    if ((rc = residual_norms(h))) return rc;
    rel = residual_rel(h);
  }
  h->guard.stat_last_rel = rel;
  if (h->flight.last_solve == 1) h->guard.factor_clean = rel <= 1e-3 * h->guard.refine_tol;
  if (rel <= h->guard.refine_tol) return PGF_OK;
  hipStream_t s = h->stream;
  auto unswap = [&]() { if (swapped) swap_point(h); };
  auto finish_round = [&]() -> int {
    enqueue_residual(h);
    h->eval_fresh = false;  // the point moves: what pgf_qp_step_async evaluated ahead is stale
    drop_norm(h);
    if (with_step) {
      unswap();
      enqueue_step_update(h);
      unswap();
      HIPCHK(h, hipMemcpyAsync(h->h_scal, h->scal, sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(h, hipStreamSynchronize(s));
    if (ldlt_chain_check(h->fac)) return fail(h, PGF_HIP_ERROR, k_chain_msg);
    return PGF_OK;
  };
  for (int it = 0; it < 2 && rel > h->guard.refine_tol && rel < 1.0 && !h->guard.lu_active; ++it) {
    HIPCHK(h, kkt_solve_async(h, h->guard.rs_r, h->guard.rs_d));
    launch_axpy1(s, h->N, h->guard.rs_d, h->sol);
    if ((rc = finish_round())) return rc;
    ++h->guard.stat_refined;
    const double now = residual_rel(h);
    if (!(now < rel)) {  // not contracting: leave it to the pivoted factorisation
      rel = now;
      break;
    }
    rel = now;
  }
  h->guard.stat_last_rel = rel;
  if (rel <= h->guard.refine_fail) return PGF_OK;
  // pivoted LU of the reduced matrix
  if (!h->guard.lu_active) {
    if (!h->guard.lu.A || h->guard.lu.N != h->N) {
      lu_free(h->guard.lu);
      HIPCHK(h, lu_alloc(h->guard.lu, h->N, s));
    }
    HIPCHK(h, hipMemsetAsync(h->guard.lu.A, 0, (size_t)h->guard.lu.N * h->guard.lu.ld * sizeof(double), s));
    assemble(h, h->guard.lu.A, h->guard.lu.ld);
    launch_symmetrize(s, h->guard.lu.A, h->guard.lu.ld, h->N);
    hipError_t e;
    const int st = lu_factor(h->guard.lu, &e);
    if (st < 0) return hip_fail(h, e, "LU fallback");
    if (st == 1) return fail(h, PGF_SINGULAR, "reduced KKT matrix is singular (LDL^T unstable, LU failed)");
    h->guard.lu_active = true;
    ++h->guard.stat_lu;
  }
  HIPCHK(h, lu_solve_async(h->guard.lu, h->rhs, h->sol, 0));
  if ((rc = finish_round())) return rc;
  rel = residual_rel(h);
  h->guard.stat_last_rel = rel;
  if (!(rel <= h->guard.refine_fail))
    return fail(h, PGF_SINGULAR, "reduced KKT system could not be solved to a small residual");
  return PGF_OK;
}

// After a host synchronisation: a chained triangular solve that failed its own checks
// (placement, timeout) has left garbage in h->sol and whatever was derived from it.  The
// chain is off from now on (ldlt_chain_check); the solve and the step update are enqueued
// again with the per-super-block kernels and awaited, so that the caller never sees the
// failure.  swapped: the caller has already exchanged (x, y) with (xn, yn) (pgf_qp_step_async).
int chain_recover(pgf_handle h, bool swapped) {
  if (!ldlt_chain_check(h->fac)) return PGF_OK;  // (0 on a banded handle: it has no chain)
  h->eval_fresh = false;  // the point is computed again
  drop_norm(h);
  if (swapped) swap_point(h);
  if (h->flight.last_solve == 1)
    HIPCHK(h, kkt_backsolve_async(h, h->sol));
  else
    HIPCHK(h, kkt_solve_async(h, h->rhs, h->sol));
  enqueue_residual(h);
  enqueue_step_update(h);
  if (swapped) swap_point(h);
  HIPCHK(h, hipMemcpyAsync(h->h_scal, h->scal, sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (ldlt_chain_check(h->fac)) return fail(h, PGF_HIP_ERROR, k_chain_msg);
  return PGF_OK;
}

int pgf_set_refinement(pgf_handle h, int mode, double tol, double fail_tol) {
  if (!h || mode < 0 || mode > 1) return PGF_INVALID;
  h->guard.refine_mode = mode;
  if (tol > 0.0) h->guard.refine_tol = tol;
  if (fail_tol > 0.0) h->guard.refine_fail = fail_tol;
  return PGF_OK;
}

int pgf_refinement_stats(pgf_handle h, int *refined, int *lu_fallbacks, double *last_rel_residual) {
  if (!h) return PGF_INVALID;
  if (refined) *refined = h->guard.stat_refined;
  if (lu_fallbacks) *lu_fallbacks = h->guard.stat_lu;
  if (last_rel_residual) *last_rel_residual = h->guard.stat_last_rel;
  return PGF_OK;
}
