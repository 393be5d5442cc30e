// The banded solve driver behind the C ABI: the banded halves of the step, factor, refinement,
// linear-solve and evaluation functions of the dense handle's files (pgf_api_internal.h lists them;
// the pgf_sparse_* setters and SparseDev's lifetimes: pgf_api_band_setup.hip).  The system keeps its
// full size n + m (an active variable is an identity row) and is
// solved by block cyclic reduction: B = 8 (pgf_sparse.hip), B = 16, 32, 64 (pgf_band_wide.hip),
// or the bordered band on top of either (pgf_border.hip).  The reduction leaves the assembled band
// intact, so every solve can be followed by its residual (the accuracy guard).  A wide reduction
// also keeps its factors (SparseDev::blk.kept): further solves on the same matrix run its solve phase.
#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#include "pgf_api_internal.h"
#include "pgf_kernels.h"

// Wide band without a border: against the kept factors when there are some (sp.blk.kept == 2),
// otherwise the fused KEEP reduction, which solves as ever and leaves the factors.  Its pivot
// flags reach the host with the caller's next synchronisation; band_kept_resolve then decides.
static void sp_cyclic_solve(hipStream_t s, SparseDev &sp, int N, int *flags, bool guard) {
  if (sp.bor.bk)  // bordered band: the solve phase against the kept Y and factor of S (pgf_border.hip)
    sp_border_solve(s, sp, flags, guard);
  else if (sp.blk.B > 8 && sp.blk.split && sp.blk.bMr && N > 0) {
    if (sp.blk.kept == 2) {
      sp_launch_bw_backsolve(s, sp, N, flags, guard);
    } else {
      sp_launch_bw_solve(s, sp, N, flags, guard, /*keep=*/true);
      sp.blk.kept = 1;
    }
  } else if (sp.blk.B > 8)
    sp_launch_bw_solve(s, sp, N, flags, guard);
  else
    sp_launch_bcr_solve(s, sp, N, flags, guard);
}

// after a host synchronisation that brought the pivot flags of every reduction enqueued so far to
// fac.h_flags: a KEEP reduction with clean flags leaves a kept factor, a bad pivot never does
void band_kept_resolve(pgf_handle h) {
  SparseDev &sp = h->sp;
  if (sp.blk.kept == 1) sp.blk.kept = h->fac.h_flags[0] ? 0 : 2;
}
static void sp_cyclic_residual(hipStream_t s, const SparseDev &sp, int N, const int *flags) {
  if (sp.bor.bk)
    sp_border_residual(s, sp, flags);
  else if (sp.blk.B > 8)
    sp_launch_bw_residual(s, sp, N, flags);
  else
    sp_launch_band_residual(s, sp, N, flags);
}

// A profile span around a phase on the handle's stream, while profiling is enabled: opened at the
// end of `spans`, closed there
typedef std::vector<std::pair<hipEvent_t, hipEvent_t>> Spans;
static void span_open(pgf_handle h, Spans &spans) {
  if (!h->prof.enabled) return;
  spans.emplace_back(prof_event(&h->prof), prof_event(&h->prof));
  (void)hipEventRecord(spans.back().first, h->stream);
}
static void span_close(pgf_handle h, Spans &spans) {
  if (h->prof.enabled) (void)hipEventRecord(spans.back().second, h->stream);
}

// the four pivot flags on their way to fac.h_flags
static int band_flags_down(pgf_handle h) { return down(h, h->fac.h_flags, h->fac.flags, 4 * sizeof(int)); }

// after the wait that brought them: settle the kept factors, refuse a bad pivot, adopt the inertia
static int band_flags_adopt(pgf_handle h) {
  band_kept_resolve(h);
  if (h->fac.h_flags[0]) return fail(h, PGF_SINGULAR, k_band_zero_pivot);
  h->fac.n_neg = h->fac.h_flags[1];
  return PGF_OK;
}

// assemble the banded matrix for the current mask; with a border also its factor phase (Y = inv(B) C
// and the factor of the Schur complement S, kept until the matrix is assembled again)
static void sp_assemble(pgf_handle h) {
  h->sp.blk.kept = 0;  // new matrix: the wide band's kept factors are stale
  if (h->sp.bor.bk) {
    sp_border_assemble(h->stream, h->sp, h->n, h->m, h->mask, h->lamb, h->delta);
    span_open(h, h->prof.factor_spans);  // the factor phase as factor_ms
    sp_border_factor(h->stream, h->sp, h->fac.flags);
    span_close(h, h->prof.factor_spans);
    return;
  }
  sp_launch_assemble(h->stream, h->sp, h->n, h->m, h->mask, h->lamb, h->delta);
}

// enqueue the band assembly and one reduction (on whatever right-hand side is there) only to
// obtain the pivot flags / inertia: the reduction keeps the assembled band intact
int band_factor_async(pgf_handle h) {
  sp_assemble(h);
  sp_cyclic_solve(h->stream, h->sp, h->n + h->m, h->fac.flags, /*guard=*/false);
  h->fac.factored = false;
  return band_flags_down(h);
}

// a guarded banded step's status block (band_step_async): after the stream has drained, the
// pivot flags and the step length take their usual places
int band_status_sync(pgf_handle h) {
  SparseDev &sp = h->sp;
  if (!h->sparse || !sp.vec.stat_pending) return PGF_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  sp.vec.stat_pending = false;
  const int nr = sp.vec.nred;
  double sum = 0.0;
  for (int i = 0; i < nr; ++i) sum += sp.vec.h_bred[2 * nr + i];
  h->h_scal[0] = sqrt(sum);
  for (int k = 0; k < 4; ++k) h->fac.h_flags[k] = (int)sp.vec.h_bred[3 * nr + k];
  return PGF_OK;
}

// The accuracy guard of the banded path (block cyclic reduction inverts its pivot blocks
// without pivoting, which is only safe while K is quasi-definite): after a host
// synchronisation, max |rhs - K s| of the guarded solve (k_band_residual, K read from the intact
// band) against refine_tol max |rhs|; beyond that up to two refinement steps -- one more
// reduction on the residual each -- and PGF_SINGULAR when the residual stays above refine_fail:
// the step controller then rejects the step and doubles lambda, which is what makes the
// matrix quasi-definite again (the reference's own recovery path, step_control.py:80-107).
double band_residual_rel_of(const double *pairs, int nred) {
  double r = 0.0, b = 0.0;
  for (int i = 0; i < nred; ++i) {
    const double ri = pairs[2 * i];
    if (!(ri == ri) || !(ri <= 1.79e308)) return HUGE_VAL;
    r = std::max(r, ri);
    b = std::max(b, pairs[2 * i + 1]);
  }
  return r / (b > 0.0 ? b : 1.0);
}
static double sparse_residual_rel(pgf_handle h) { return band_residual_rel_of(h->sp.vec.h_bred, h->sp.vec.nred); }

int band_refine(pgf_handle h, bool swapped, bool with_step) {
  if (!h->guard.refine_mode || !h->sp.vec.guarded) return PGF_OK;
  const int Nf = h->n + h->m;
  if (Nf == 0) return PGF_OK;
  double rel = sparse_residual_rel(h);
  h->guard.stat_last_rel = rel;
  if (rel <= h->guard.refine_tol) return PGF_OK;
  hipStream_t s = h->stream;
  SparseDev &sp = h->sp;
  auto unswap = [&]() { if (swapped) swap_point(h); };
  for (int it = 0; it < 2 && rel > h->guard.refine_tol && rel < 1.0; ++it) {
    HIPCHK(h, hipMemcpyAsync(sp.vec.bsol, sp.vec.brhs, (size_t)Nf * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(sp.vec.brhs, sp.vec.bres, (size_t)Nf * sizeof(double), hipMemcpyDeviceToDevice, s));
    sp_cyclic_solve(s, sp, Nf, h->fac.flags, /*guard=*/false);
    sp_launch_band_axpy(s, Nf, sp.vec.bsol, sp.vec.brhs);
    sp_cyclic_residual(s, sp, Nf, h->fac.flags);
    HIPCHK(h, hipMemcpyAsync(sp.vec.h_bred, sp.vec.bred, (size_t)2 * sp.vec.nred * sizeof(double), hipMemcpyDeviceToHost, s));
    if (with_step) {
      unswap();
      sp_launch_step_update(s, sp, h->n, h->m, h->fact, h->rho, h->x, h->y, h->lb, h->ub, h->F, h->dx,
                            h->dy, h->xn, h->yn, h->red);
      launch_final_reduce(s, h->red, (h->n + h->m + 255) / 256, h->scal, 1);
      unswap();
      HIPCHK(h, hipMemcpyAsync(h->h_scal, h->scal, sizeof(double), hipMemcpyDeviceToHost, s));
    }
    HIPCHK(h, hipStreamSynchronize(s));
    ++h->guard.stat_refined;
    const double now = sparse_residual_rel(h);
    if (!(now < rel)) {
      rel = now;
      break;
    }
    rel = now;
  }
  h->guard.stat_last_rel = rel;
  if (!(rel <= h->guard.refine_fail))
    return fail(h, PGF_SINGULAR,
                "banded KKT system could not be solved to a small residual (unpivoted block cyclic reduction)");
  return PGF_OK;
}

// residual + right-hand side for the point in (h->x, h->y, h->g, h->c), then solve and update,
// and the copy that brings the step's status to the host.  Everything is enqueued; returns
// without syncing.  *did_factor is always set: the solve's pivot flags need checking at the sync.
int band_step_async(pgf_handle h, bool *did_factor) {
  hipStream_t s = h->stream;
  SparseDev &sp = h->sp;
  const int Nf = h->n + h->m;
  launch_residual(s, h->n, h->m, h->lamb, h->dt, h->xhat, h->yhat, h->x, h->y, h->g, h->c, h->slb,
                  h->sub, h->mask, h->F, h->b0full);
  sp_launch_rhs(s, sp, h->n, h->m, h->mask, h->F, h->b0full, h->fact, sp.pat.Hb0, sp.pat.Jb0);
  // assemble (only when the mask / derivatives changed) and solve in log2(N/B) parallel levels;
  // the band itself is left untouched, so a back-solve step runs the reduction again on the same
  // band (B = 8, borders at B = 8) or the solve phase against the factors a wide reduction kept
  if (!h->fac.factored) sp_assemble(h);
  span_open(h, h->prof.update_spans);
  const bool solve_phase = !sp.bor.bk && sp.blk.kept == 2;
  sp_cyclic_solve(s, sp, Nf, h->fac.flags, h->guard.refine_mode != 0);
  const bool keep_red = sp.blk.kept == 1;
  sp.vec.guarded = h->guard.refine_mode != 0;
  span_close(h, h->prof.update_spans);
  if (h->prof.enabled) {
    // algorithmic bytes of one cyclic-reduction solve: every block (D, L, U, inv D:
    // 4 x 8 B^2, rhs + solution 16 B) is written once and read about twice; a KEEP reduction
    // writes two more blocks (the multipliers); a solve phase against kept factors reads five
    // blocks (Mr, Ml, L, U, inv D) once and f twice, and writes f and x
    const double Bk = (double)sp.blk.B, nblk = (double)((Nf + sp.blk.B - 1) / sp.blk.B);
    if (solve_phase)
      h->prof.update_flops.push_back(nblk * (5 * 8 * Bk * Bk + 32 * Bk));
    else
      h->prof.update_flops.push_back(3.0 * nblk * (4 * 8 * Bk * Bk + 16 * Bk) + (keep_red ? nblk * 16 * Bk * Bk : 0.0));
  }
  *did_factor = true;
  if (sp.vec.guarded) {
    // ONE status block for the host: residual pairs, the step update's partial sums (summed
    // on the host: no reduction kernel) and the pivot flags -- one copy instead of three
    sp_launch_step_update(s, sp, h->n, h->m, h->fact, h->rho, h->x, h->y, h->lb, h->ub, h->F,
                          h->dx, h->dy, h->xn, h->yn, sp.vec.bred + 2 * sp.vec.nred);
    sp.vec.stat_pending = true;
    return down(h, sp.vec.h_bred, sp.vec.bred, band_stat_stride(sp.vec.nred) * sizeof(double));
  }
  int rc;
  if ((rc = band_flags_down(h))) return rc;
  sp_launch_step_update(s, sp, h->n, h->m, h->fact, h->rho, h->x, h->y, h->lb, h->ub, h->F,
                        h->dx, h->dy, h->xn, h->yn, h->red);
  launch_final_reduce(s, h->red, (h->n + h->m + 255) / 256, h->scal, 1);
  return down(h, h->h_scal, h->scal, sizeof(double));
}

// rhs / sol have n + m entries in the order [variables; constraints]; entries of active
// variables pass through (sol = rhs there)
int band_linear_solve(pgf_handle h, const double *rhs, double *sol) {
  const int Nf = h->n + h->m;
  if (Nf && (!rhs || !sol)) return fail(h, PGF_INVALID, "null argument");
  (void)hipSetDevice(h->device);
  SparseDev &sp = h->sp;
  int rc;
  if ((rc = up(h, h->rhs, rhs, (size_t)Nf * sizeof(double)))) return rc;
  sp_launch_permute(h->stream, sp, Nf, h->rhs, sp.vec.brhs, 0);
  // cyclic reduction keeps the assembled band intact: (re)assemble only when stale
  if (!h->fac.factored) sp_assemble(h);
  sp_cyclic_solve(h->stream, sp, Nf, h->fac.flags, h->guard.refine_mode != 0);
  sp.vec.guarded = h->guard.refine_mode != 0;
  if (sp.vec.guarded)
    HIPCHK(h, hipMemcpyAsync(sp.vec.h_bred, sp.vec.bred, (size_t)2 * sp.vec.nred * sizeof(double),
                             hipMemcpyDeviceToHost, h->stream));
  if ((rc = band_flags_down(h))) return rc;
  if (sp.vec.guarded) {  // residual check (and refinement) before the solution leaves
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if ((rc = band_flags_adopt(h))) return rc;
    if ((rc = band_refine(h, false, false))) return rc;
    h->fac.h_flags[0] = 0;  // (a refinement round's reductions have overwritten the pinned flags)
    h->fac.h_flags[1] = h->fac.n_neg;
  }
  sp_launch_permute(h->stream, sp, Nf, sp.vec.brhs, h->sol, 1);
  if ((rc = down(h, sol, h->sol, (size_t)Nf * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if ((rc = band_flags_adopt(h))) return rc;
  h->fac.factored = true;
  return PGF_OK;
}

// Several right-hand sides at once on a wide band without a border (split on): the factors of one
// factor-only KEEP reduction (or those a step left), then per chunk of at most 64 columns one
// panel solve on the matrix pipes.  Every column's residual is checked by k_bw_residual; one
// above refine_tol is solved again through the guarded single right-hand side path.
bool band_multi_panel(pgf_handle h) {
  const SparseDev &sp = h->sp;
  return h->sparse && sp.active && !sp.bor.bk && sp.blk.B > 8 && sp.blk.split && sp.blk.bMr && h->n + h->m > 0;
}

int band_linear_solve_multi(pgf_handle h, const double *rhs, int nrhs, int64_t ld, double *sol) {
  const int Nf = h->n + h->m;
  (void)hipSetDevice(h->device);
  hipStream_t s = h->stream;
  SparseDev &sp = h->sp;
  const size_t Bk = (size_t)sp.blk.B, prows = (size_t)sp.blk.bstride * Bk;
  const size_t pairs = band_stat_stride(sp.vec.nred);
  int rc;
  if ((rc = band_panel_reserve(h))) return rc;
  double *R = sp.pan.bP + prows * 64;  // the right-hand sides as they came (natural order)
  if (!h->fac.factored) sp_assemble(h);
  if (sp.blk.kept != 2) {
    sp_launch_bw_factor(s, sp, Nf, h->fac.flags);
    sp.blk.kept = 1;
    if ((rc = band_flags_down(h))) return rc;
    HIPCHK(h, hipStreamSynchronize(s));
    if ((rc = band_flags_adopt(h))) return rc;
    h->fac.factored = true;
  }
  const bool guard = h->guard.refine_mode != 0;
  const int nb = (Nf + sp.blk.B - 1) / sp.blk.B;
  double worst = 0.0;
  for (int c0 = 0; c0 < nrhs; c0 += 64) {
    const int nc = std::min(64, nrhs - c0), kp = (nc + 15) / 16 * 16;
    HIPCHK(h, hipMemsetAsync(sp.pan.bP, 0, (size_t)nb * Bk * kp * sizeof(double), s));
    for (int j = 0; j < nc; ++j) {
      double *Rj = R + (size_t)j * Nf;
      if ((rc = up(h, Rj, rhs + (int64_t)(c0 + j) * ld, (size_t)Nf * sizeof(double)))) return rc;
      sp_launch_bw_panel_put(s, sp, Nf, Rj, sp.pan.bP, kp, j);
    }
    sp_launch_bw_panel_solve(s, sp, Nf, sp.pan.bP, kp);
    for (int j = 0; j < nc; ++j) {
      sp_launch_bw_panel_get(s, Nf, sp.pan.bP, kp, j, sp.vec.brhs);
      if (guard) {
        sp_launch_permute(s, sp, Nf, R + (size_t)j * Nf, sp.vec.brhs0, 0);
        sp_launch_bw_residual_to(s, sp, Nf, h->fac.flags, sp.pan.bredm + (size_t)j * pairs);
      }
      sp_launch_permute(s, sp, Nf, sp.vec.brhs, h->sol, 1);
      if ((rc = down(h, sol + (int64_t)(c0 + j) * ld, h->sol, (size_t)Nf * sizeof(double)))) return rc;
    }
    if (guard)
      HIPCHK(h, hipMemcpyAsync(sp.pan.h_bredm, sp.pan.bredm, (size_t)nc * pairs * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (!guard) continue;
    for (int j = 0; j < nc; ++j) {
      const double rel = band_residual_rel_of(sp.pan.h_bredm + (size_t)j * pairs, sp.vec.nred);
      if (rel > h->guard.refine_tol) {  // this column once more, guarded and refined
        if ((rc = band_linear_solve(h, rhs + (int64_t)(c0 + j) * ld, sol + (int64_t)(c0 + j) * ld))) return rc;
        worst = std::max(worst, h->guard.stat_last_rel);
      } else {
        worst = std::max(worst, rel);
      }
    }
  }
  if (guard) h->guard.stat_last_rel = worst;
  return PGF_OK;
}

// c = A x - b ; w = rho c + y ; g = Q x + (q + A' w)   at the device point
void band_eval(pgf_handle h) {
  sp_launch_eval(h->stream, h->sp, h->n, h->m, h->x, h->y, h->b, h->q, h->rho, h->c, h->w, h->g);
}

// c = A x - b and F = Q x + q + A' w for the termination measures (w holds y: no rho term)
void band_measures_eval(pgf_handle h) {
  hipStream_t s = h->stream;
  const SparseDev &sp = h->sp;
  sp_launch_spmv(s, h->m, sp.pat.Jptr, sp.pat.Jcol, sp.pat.Jval, h->x, h->b, -1.0, h->c);
  sp_launch_spmvT(s, h->n, sp.pat.JTptr, sp.pat.JTrow, sp.pat.JTmap, sp.pat.Jval, h->w, h->q, h->tmpn);
  sp_launch_spmv(s, h->n, sp.pat.Hptr, sp.pat.Hcol, sp.pat.Hval, h->x, h->tmpn, 1.0, h->F);
}
