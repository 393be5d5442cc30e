// The banded driver behind the C ABI: the pgf_sparse_* entry points and the banded halves of the
// step, factor, refinement and linear-solve functions of the dense handle's files (pgf_api_internal.h lists
// them).  The system keeps its full size n + m (an active variable is an identity row) and is
// solved by block cyclic reduction: B = 8 (pgf_sparse.hip), B = 16, 32, 64 (pgf_band_wide.hip),
// or the bordered band on top of either (pgf_border.hip).  The reduction leaves the assembled band
// intact, so every solve can be followed by its residual (the accuracy guard).  A wide reduction
// also keeps its factors (SparseDev::kept): further solves on the same matrix run its solve phase.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <new>
#include <utility>

#include "pgf_api_internal.h"
#include "pgf_env.h"
#include "pgf_kernels.h"

// PGF_BW_SPLIT=0: new handles start with the wide band's factor / solve split off
bool band_split_default() { static const bool on = env_on("PGF_BW_SPLIT"); return on; }

// Wide band without a border: against the kept factors when there are some (sp.kept == 2),
// otherwise the fused KEEP reduction, which solves as ever and leaves the factors.  Its pivot
// flags reach the host with the caller's next synchronisation; band_kept_resolve then decides.
static void sp_cyclic_solve(hipStream_t s, SparseDev &sp, int N, int *flags, bool guard) {
  if (sp.bk)  // bordered band: the solve phase against the kept Y and factor of S (pgf_border.hip)
    sp_border_solve(s, sp, flags, guard);
  else if (sp.B > 8 && sp.split && sp.bMr && N > 0) {
    if (sp.kept == 2) {
      sp_launch_bw_backsolve(s, sp, N, flags, guard);
    } else {
      sp_launch_bw_solve(s, sp, N, flags, guard, /*keep=*/true);
      sp.kept = 1;
    }
  } else if (sp.B > 8)
    sp_launch_bw_solve(s, sp, N, flags, guard);
  else
    sp_launch_bcr_solve(s, sp, N, flags, guard);
}

// after a host synchronisation that brought the pivot flags of every reduction enqueued so far to
// fac.h_flags: a KEEP reduction with clean flags leaves a kept factor, a bad pivot never does
void band_kept_resolve(pgf_handle h) {
  SparseDev &sp = h->sp;
  if (sp.kept == 1) sp.kept = h->fac.h_flags[0] ? 0 : 2;
}
static void sp_cyclic_residual(hipStream_t s, const SparseDev &sp, int N, const int *flags) {
  if (sp.bk)
    sp_border_residual(s, sp, flags);
  else if (sp.B > 8)
    sp_launch_bw_residual(s, sp, N, flags);
  else
    sp_launch_band_residual(s, sp, N, flags);
}

// assemble the banded matrix for the current mask; with a border also its factor phase (Y = inv(B) C
// and the factor of the Schur complement S, kept until the matrix is assembled again)
static void sp_assemble(pgf_handle h) {
  h->sp.kept = 0;  // new matrix: the wide band's kept factors are stale
  if (h->sp.bk) {
    sp_border_assemble(h->stream, h->sp, h->n, h->m, h->mask, h->lamb, h->delta);
    PgfProfile *p = h->prof.enabled ? &h->prof : nullptr;  // the factor phase as factor_ms
    if (p) {
      p->factor_spans.emplace_back(prof_event(p), prof_event(p));
      (void)hipEventRecord(p->factor_spans.back().first, h->stream);
    }
    sp_border_factor(h->stream, h->sp, h->fac.flags);
    if (p) (void)hipEventRecord(p->factor_spans.back().second, h->stream);
    return;
  }
  sp_launch_assemble(h->stream, h->sp, h->n, h->m, h->mask, h->lamb, h->delta);
}

// enqueue the band assembly and one reduction (on whatever right-hand side is there) only to
// obtain the pivot flags / inertia: the reduction keeps the assembled band intact
int band_factor_async(pgf_handle h) {
  sp_assemble(h);
  sp_cyclic_solve(h->stream, h->sp, h->n + h->m, h->fac.flags, /*guard=*/false);
  HIPCHK(h, hipMemcpyAsync(h->fac.h_flags, h->fac.flags, 4 * sizeof(int), hipMemcpyDeviceToHost,
                           h->stream));
  h->fac.factored = false;
  return PGF_OK;
}

// a guarded banded step's status block (band_step_async): after the stream has drained, the
// pivot flags and the step length take their usual places
int band_status_sync(pgf_handle h) {
  SparseDev &sp = h->sp;
  if (!h->sparse || !sp.stat_pending) return PGF_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  sp.stat_pending = false;
  const int nr = sp.nred;
  double sum = 0.0;
  for (int i = 0; i < nr; ++i) sum += sp.h_bred[2 * nr + i];
  h->h_scal[0] = sqrt(sum);
  for (int k = 0; k < 4; ++k) h->fac.h_flags[k] = (int)sp.h_bred[3 * nr + k];
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
static double sparse_residual_rel(pgf_handle h) { return band_residual_rel_of(h->sp.h_bred, h->sp.nred); }

int band_refine(pgf_handle h, bool swapped, bool with_step) {
  if (!h->guard.refine_mode || !h->sp.guarded) return PGF_OK;
  const int Nf = h->n + h->m;
  if (Nf == 0) return PGF_OK;
  double rel = sparse_residual_rel(h);
  h->guard.stat_last_rel = rel;
  if (rel <= h->guard.refine_tol) return PGF_OK;
  hipStream_t s = h->stream;
  SparseDev &sp = h->sp;
  auto unswap = [&]() { if (swapped) swap_point(h); };
  for (int it = 0; it < 2 && rel > h->guard.refine_tol && rel < 1.0; ++it) {
    HIPCHK(h, hipMemcpyAsync(sp.bsol, sp.brhs, (size_t)Nf * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPCHK(h, hipMemcpyAsync(sp.brhs, sp.bres, (size_t)Nf * sizeof(double), hipMemcpyDeviceToDevice, s));
    sp_cyclic_solve(s, sp, Nf, h->fac.flags, /*guard=*/false);
    sp_launch_band_axpy(s, Nf, sp.bsol, sp.brhs);
    sp_cyclic_residual(s, sp, Nf, h->fac.flags);
    HIPCHK(h, hipMemcpyAsync(sp.h_bred, sp.bred, (size_t)2 * sp.nred * sizeof(double), hipMemcpyDeviceToHost, s));
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
  sp_launch_rhs(s, sp, h->n, h->m, h->mask, h->F, h->b0full, h->fact, sp.Hb0, sp.Jb0);
  // assemble (only when the mask / derivatives changed) and solve in log2(N/B) parallel levels;
  // the band itself is left untouched, so a back-solve step runs the reduction again on the same
  // band (B = 8, borders at B = 8) or the solve phase against the factors a wide reduction kept
  if (!h->fac.factored) sp_assemble(h);
  PgfProfile *p = h->prof.enabled ? &h->prof : nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  if (p) {
    e0 = prof_event(p);
    e1 = prof_event(p);
    (void)hipEventRecord(e0, s);
  }
  const bool solve_phase = !sp.bk && sp.kept == 2;
  sp_cyclic_solve(s, sp, Nf, h->fac.flags, h->guard.refine_mode != 0);
  const bool keep_red = sp.kept == 1;
  sp.guarded = h->guard.refine_mode != 0;
  if (p) {
    (void)hipEventRecord(e1, s);
    p->update_spans.emplace_back(e0, e1);
    // algorithmic bytes of one cyclic-reduction solve: every block (D, L, U, inv D:
    // 4 x 8 B^2, rhs + solution 16 B) is written once and read about twice; a KEEP reduction
    // writes two more blocks (the multipliers); a solve phase against kept factors reads five
    // blocks (Mr, Ml, L, U, inv D) once and f twice, and writes f and x
    const double Bk = (double)sp.B, nblk = (double)((Nf + sp.B - 1) / sp.B);
    if (solve_phase)
      p->update_flops.push_back(nblk * (5 * 8 * Bk * Bk + 32 * Bk));
    else
      p->update_flops.push_back(3.0 * nblk * (4 * 8 * Bk * Bk + 16 * Bk) + (keep_red ? nblk * 16 * Bk * Bk : 0.0));
  }
  *did_factor = true;
  if (sp.guarded) {
    // ONE status block for the host: residual pairs, the step update's partial sums (summed
    // on the host: no reduction kernel) and the pivot flags -- one copy instead of three
    sp_launch_step_update(s, sp, h->n, h->m, h->fact, h->rho, h->x, h->y, h->lb, h->ub, h->F,
                          h->dx, h->dy, h->xn, h->yn, sp.bred + 2 * sp.nred);
    HIPCHK(h, hipMemcpyAsync(sp.h_bred, sp.bred, ((size_t)3 * sp.nred + 4) * sizeof(double),
                             hipMemcpyDeviceToHost, s));
    sp.stat_pending = true;
    return PGF_OK;
  }
  HIPCHK(h, hipMemcpyAsync(h->fac.h_flags, h->fac.flags, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
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
  sp_launch_permute(h->stream, sp, Nf, h->rhs, sp.brhs, 0);
  // cyclic reduction keeps the assembled band intact: (re)assemble only when stale
  if (!h->fac.factored) sp_assemble(h);
  sp_cyclic_solve(h->stream, sp, Nf, h->fac.flags, h->guard.refine_mode != 0);
  sp.guarded = h->guard.refine_mode != 0;
  if (sp.guarded)
    HIPCHK(h, hipMemcpyAsync(sp.h_bred, sp.bred, (size_t)2 * sp.nred * sizeof(double),
                             hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(h->fac.h_flags, h->fac.flags, 4 * sizeof(int), hipMemcpyDeviceToHost,
                           h->stream));
  if (sp.guarded) {  // residual check (and refinement) before the solution leaves
    HIPCHK(h, hipStreamSynchronize(h->stream));
    band_kept_resolve(h);
    if (h->fac.h_flags[0]) return fail(h, PGF_SINGULAR, "zero or non-finite pivot in the banded KKT factorisation");
    const int nneg = h->fac.h_flags[1];
    if ((rc = band_refine(h, false, false))) return rc;
    h->fac.h_flags[0] = 0;
    h->fac.h_flags[1] = nneg;
  }
  sp_launch_permute(h->stream, sp, Nf, sp.brhs, h->sol, 1);
  if ((rc = down(h, sol, h->sol, (size_t)Nf * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  band_kept_resolve(h);
  if (h->fac.h_flags[0]) return fail(h, PGF_SINGULAR, "zero or non-finite pivot in the banded KKT factorisation");
  h->fac.n_neg = h->fac.h_flags[1];
  h->fac.factored = true;
  return PGF_OK;
}

// Several right-hand sides at once on a wide band without a border (split on): the factors of one
// factor-only KEEP reduction (or those a step left), then per chunk of at most 64 columns one
// panel solve on the matrix pipes.  Every column's residual is checked by k_bw_residual; one
// above refine_tol is solved again through the guarded single right-hand side path.
bool band_multi_panel(pgf_handle h) {
  const SparseDev &sp = h->sp;
  return h->sparse && sp.active && !sp.bk && sp.B > 8 && sp.split && sp.bMr && h->n + h->m > 0;
}

int band_linear_solve_multi(pgf_handle h, const double *rhs, int nrhs, int64_t ld, double *sol) {
  const int Nf = h->n + h->m;
  (void)hipSetDevice(h->device);
  hipStream_t s = h->stream;
  SparseDev &sp = h->sp;
  const size_t Bk = (size_t)sp.B, nbk = (size_t)sp.bstride, prows = nbk * Bk;
  const size_t pairs = (size_t)3 * sp.nred + 4;
  if (!sp.bP) {  // the panel and, behind it, the right-hand sides as they came (natural order)
    HIPCHK(h, dalloc(&sp.bP, prows * 64 + (size_t)64 * Nf));
    HIPCHK(h, dalloc(&sp.bredm, 64 * pairs));
    HIPCHK(h, hipHostMalloc((void **)&sp.h_bredm, 64 * pairs * sizeof(double)));
  }
  double *R = sp.bP + prows * 64;
  if (!h->fac.factored) sp_assemble(h);
  if (sp.kept != 2) {
    sp_launch_bw_factor(s, sp, Nf, h->fac.flags);
    sp.kept = 1;
    HIPCHK(h, hipMemcpyAsync(h->fac.h_flags, h->fac.flags, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    band_kept_resolve(h);
    if (h->fac.h_flags[0])
      return fail(h, PGF_SINGULAR, "zero or non-finite pivot in the banded KKT factorisation");
    h->fac.n_neg = h->fac.h_flags[1];
    h->fac.factored = true;
  }
  const bool guard = h->guard.refine_mode != 0;
  const int nb = (Nf + sp.B - 1) / sp.B;
  int rc;
  double worst = 0.0;
  for (int c0 = 0; c0 < nrhs; c0 += 64) {
    const int nc = std::min(64, nrhs - c0), kp = (nc + 15) / 16 * 16;
    HIPCHK(h, hipMemsetAsync(sp.bP, 0, (size_t)nb * Bk * kp * sizeof(double), s));
    for (int j = 0; j < nc; ++j) {
      double *Rj = R + (size_t)j * Nf;
      if ((rc = up(h, Rj, rhs + (int64_t)(c0 + j) * ld, (size_t)Nf * sizeof(double)))) return rc;
      sp_launch_bw_panel_put(s, sp, Nf, Rj, sp.bP, kp, j);
    }
    sp_launch_bw_panel_solve(s, sp, Nf, sp.bP, kp);
    for (int j = 0; j < nc; ++j) {
      sp_launch_bw_panel_get(s, Nf, sp.bP, kp, j, sp.brhs);
      if (guard) {
        sp_launch_permute(s, sp, Nf, R + (size_t)j * Nf, sp.brhs0, 0);
        sp_launch_bw_residual_to(s, sp, Nf, h->fac.flags, sp.bredm + (size_t)j * pairs);
      }
      sp_launch_permute(s, sp, Nf, sp.brhs, h->sol, 1);
      if ((rc = down(h, sol + (int64_t)(c0 + j) * ld, h->sol, (size_t)Nf * sizeof(double)))) return rc;
    }
    if (guard)
      HIPCHK(h, hipMemcpyAsync(sp.h_bredm, sp.bredm, (size_t)nc * pairs * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (!guard) continue;
    for (int j = 0; j < nc; ++j) {
      const double rel = band_residual_rel_of(sp.h_bredm + (size_t)j * pairs, sp.nred);
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
  sp_launch_spmv(s, h->m, sp.Jptr, sp.Jcol, sp.Jval, h->x, h->b, -1.0, h->c);
  sp_launch_spmvT(s, h->n, sp.JTptr, sp.JTrow, sp.JTmap, sp.Jval, h->w, h->q, h->tmpn);
  sp_launch_spmv(s, h->n, sp.Hptr, sp.Hcol, sp.Hval, h->x, h->tmpn, 1.0, h->F);
}

// ---------------------------------------------------------------- pattern, border, block size
// bw <= 8: 8 x 8 cyclic reduction; 9 .. 64: the smallest of 16, 32, 64 that holds the band
static int auto_block_size(int bw) { return bw <= 8 ? 8 : bw <= 16 ? 16 : bw <= 32 ? 32 : 64; }

// work arrays of the cyclic reduction for block size B.  B = 8 keeps two block sets
// (k_bcr_level2 reads one and writes the other); the wide kernels use one.
static int sp_alloc_blocks(pgf_handle h, int B) {
  SparseDev &sp = h->sp;
  for (double **q : {&sp.bD, &sp.bL, &sp.bU, &sp.bDinv, &sp.bF, &sp.bMr, &sp.bMl, &sp.bP, &sp.bredm})
    if (*q) {
      (void)hipFree(*q);
      *q = nullptr;
    }
  if (sp.bneg) {
    (void)hipFree(sp.bneg);
    sp.bneg = nullptr;
  }
  if (sp.h_bredm) {
    (void)hipHostFree(sp.h_bredm);
    sp.h_bredm = nullptr;
  }
  sp.kept = 0;
  sp.B = B;
  sp.bX = sp.brhs;  // the back-substitution writes the solution where the step update reads it
  const int N = h->n + h->m;
  const size_t nsets = (B == 8) ? 2 : 1, Bk = (size_t)B;
  const size_t nbk = ((size_t)N + Bk - 1) / Bk + 1;
  HIPCHK(h, dalloc(&sp.bD, nsets * nbk * Bk * Bk));
  HIPCHK(h, dalloc(&sp.bL, nsets * nbk * Bk * Bk));
  HIPCHK(h, dalloc(&sp.bU, nsets * nbk * Bk * Bk));
  HIPCHK(h, dalloc(&sp.bDinv, nbk * Bk * Bk));
  HIPCHK(h, dalloc(&sp.bF, nsets * nbk * Bk));
  sp.bstride = (int64_t)nbk;
  HIPCHK(h, dalloc(&sp.bneg, nbk));
  if (B > 8 && sp.split) {  // the kept forward multipliers of the wide reduction
    HIPCHK(h, dalloc(&sp.bMr, nbk * Bk * Bk));
    HIPCHK(h, dalloc(&sp.bMl, nbk * Bk * Bk));
  }
  return PGF_OK;
}

static void sp_border_free(SparseDev &sp) {
  for (double **q : {&sp.bY, &sp.bS, &sp.bpart, &sp.bpartv, &sp.brb, &sp.bz})
    if (*q) {
      (void)hipFree(*q);
      *q = nullptr;
    }
  if (sp.bsflags) {
    (void)hipFree(sp.bsflags);
    sp.bsflags = nullptr;
  }
  if (sp.bG) {  // large border: the kept C' Y and the dense factor of S
    (void)hipFree(sp.bG);
    sp.bG = nullptr;
  }
  if (sp.blf) {
    ldlt_free(*sp.blf);
    delete sp.blf;
    sp.blf = nullptr;
  }
  sp.bgrows = sp.bgchunks = 0;
  sp.bgram_ready = false;
  sp.bk = sp.bkp = sp.Nb = sp.bnchunk = 0;
  sp.bC = sp.bDd = nullptr;
  sp.stat_bfactor = sp.stat_bsolve = 0;
}

// the residual pairs, the step update's partial sums and the pivot flags (SparseDev::bred) and
// their pinned mirror, for nred pairs
static int sp_alloc_bred(pgf_handle h, int nred) {
  SparseDev &sp = h->sp;
  if (sp.bred) {
    (void)hipFree(sp.bred);
    sp.bred = nullptr;
  }
  if (sp.h_bred) {
    (void)hipHostFree(sp.h_bred);
    sp.h_bred = nullptr;
  }
  sp.nred = nred;
  HIPCHK(h, dalloc(&sp.bred, (size_t)3 * nred + 4));
  HIPCHK(h, hipHostMalloc((void **)&sp.h_bred, ((size_t)3 * nred + 4) * sizeof(double)));
  return PGF_OK;
}

void band_free(pgf_handle h) {
  SparseDev &sp = h->sp;
  if (sp.h_bred) (void)hipHostFree(sp.h_bred);
  if (sp.h_bredm) (void)hipHostFree(sp.h_bredm);
  void *sps[] = {sp.pos, sp.Hptr, sp.Hrow, sp.Hcol, sp.Hslot, sp.Jptr, sp.Jcol, sp.Jslot, sp.JTptr,
                 sp.JTrow, sp.JTmap, sp.Hval, sp.Jval, sp.band, sp.brhs, sp.Hb0, sp.Jb0,
                 sp.bD, sp.bL, sp.bU, sp.bDinv, sp.bF, sp.bneg, sp.brhs0, sp.bres, sp.bsol,
                 sp.bred, sp.bMr, sp.bMl, sp.bP, sp.bredm, sp.bY, sp.bS, sp.bpart, sp.bpartv, sp.brb, sp.bz, sp.bsflags,
                 sp.bG};
  for (void *q : sps)
    if (q) (void)hipFree(q);
  if (sp.blf) {
    ldlt_free(*sp.blf);
    delete sp.blf;
  }
}

extern "C" {

int pgf_sparse_pattern_hash(int n, int m, int bw, const int *pos, int nnzH, const int *Hptr,
                            const int *Hrow, const int *Hcol, const int *Hslot, int nnzJ,
                            const int *Jptr, const int *Jcol, const int *Jslot, const int *JTptr,
                            const int *JTrow, const int *JTmap, uint64_t *hash_out) {
  if (!hash_out || n < 0 || m < 0 || nnzH < 0 || nnzJ < 0 || !pos || !Hptr || !Jptr || !JTptr ||
      (nnzH && (!Hrow || !Hcol || !Hslot)) || (nnzJ && (!Jcol || !Jslot || !JTrow || !JTmap)))
    return PGF_INVALID;
  uint64_t hsh = 1469598103934665603ull;  // FNV-1a, 64 bit
  auto eat = [&](const int *a, size_t count) {
    const unsigned char *p = reinterpret_cast<const unsigned char *>(a);
    for (size_t k = 0; k < count * sizeof(int); ++k) hsh = (hsh ^ p[k]) * 1099511628211ull;
  };
  const int head[5] = {n, m, bw, nnzH, nnzJ};
  eat(head, 5);
  eat(pos, (size_t)n + m);
  eat(Hptr, (size_t)n + 1);
  eat(Hrow, (size_t)nnzH);
  eat(Hcol, (size_t)nnzH);
  eat(Hslot, (size_t)nnzH);
  eat(Jptr, (size_t)m + 1);
  eat(Jcol, (size_t)nnzJ);
  eat(Jslot, (size_t)nnzJ);
  eat(JTptr, (size_t)n + 1);
  eat(JTrow, (size_t)nnzJ);
  eat(JTmap, (size_t)nnzJ);
  *hash_out = hsh;
  return PGF_OK;
}

int pgf_sparse_set_pattern(pgf_handle h, int bw, const int *pos, int nnzH, const int *Hptr,
                           const int *Hrow, const int *Hcol, const int *Hslot, int nnzJ,
                           const int *Jptr, const int *Jcol, const int *Jslot, const int *JTptr,
                           const int *JTrow, const int *JTmap) {
  if (!h) return PGF_INVALID;
  if (!h->sparse) return fail(h, PGF_NOT_READY, "handle was not created with PGF_CREATE_SPARSE");
  if (bw < 0 || bw > 64) return fail(h, PGF_INVALID, "bandwidth must be 0..64 in this version");
  if (nnzH < 0 || nnzJ < 0 || !pos || !Hptr || !Jptr || !JTptr)
    return fail(h, PGF_INVALID, "null pattern");
  (void)hipSetDevice(h->device);
  SparseDev &sp = h->sp;
  const int n = h->n, m = h->m, N = n + m;
  sp.bw = bw;
  sp.ldb = ((bw + 1) + 1) / 2 * 2;
  sp.nnzH = nnzH;
  sp.nnzJ = nnzJ;
  int rc;
  if ((rc = up_new(h, &sp.pos, pos, (size_t)N))) return rc;
  if ((rc = up_new(h, &sp.Hptr, Hptr, (size_t)n + 1))) return rc;
  if ((rc = up_new(h, &sp.Hrow, Hrow, (size_t)nnzH))) return rc;
  if ((rc = up_new(h, &sp.Hcol, Hcol, (size_t)nnzH))) return rc;
  if ((rc = up_new(h, &sp.Hslot, Hslot, (size_t)nnzH))) return rc;
  if ((rc = up_new(h, &sp.Jptr, Jptr, (size_t)m + 1))) return rc;
  if ((rc = up_new(h, &sp.Jcol, Jcol, (size_t)nnzJ))) return rc;
  if ((rc = up_new(h, &sp.Jslot, Jslot, (size_t)nnzJ))) return rc;
  if ((rc = up_new(h, &sp.JTptr, JTptr, (size_t)n + 1))) return rc;
  if ((rc = up_new(h, &sp.JTrow, JTrow, (size_t)nnzJ))) return rc;
  if ((rc = up_new(h, &sp.JTmap, JTmap, (size_t)nnzJ))) return rc;
  for (double **q : {&sp.Hval, &sp.Jval, &sp.band, &sp.brhs, &sp.Hb0, &sp.Jb0, &sp.brhs0, &sp.bres, &sp.bsol})
    if (*q) {
      (void)hipFree(*q);
      *q = nullptr;
    }
  HIPCHK(h, dalloc(&sp.Hval, (size_t)nnzH));
  HIPCHK(h, dalloc(&sp.Jval, (size_t)nnzJ));
  HIPCHK(h, dalloc(&sp.band, (size_t)(N + 1) * sp.ldb));
  HIPCHK(h, dalloc(&sp.brhs, (size_t)N + 64));  // whole B-row blocks: the cyclic reduction's X
  HIPCHK(h, dalloc(&sp.brhs0, (size_t)N + 1));
  HIPCHK(h, dalloc(&sp.bres, (size_t)N + 1));
  HIPCHK(h, dalloc(&sp.bsol, (size_t)N + 1));
  if ((rc = sp_alloc_bred(h, (N + 255) / 256))) return rc;
  HIPCHK(h, dalloc(&sp.Hb0, (size_t)n + 1));
  HIPCHK(h, dalloc(&sp.Jb0, (size_t)m + 1));
  sp_border_free(sp);  // (a border is declared after the pattern: pgf_sparse_set_border)
  if ((rc = sp_alloc_blocks(h, auto_block_size(bw)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  // (what a banded batch compares: its instances share one pattern)
  if (pgf_sparse_pattern_hash(n, m, bw, pos, nnzH, Hptr, Hrow, Hcol, Hslot, nnzJ, Jptr, Jcol, Jslot, JTptr,
                              JTrow, JTmap, &sp.pat_hash) != PGF_OK)
    return fail(h, PGF_INVALID, "null pattern");
  sp.active = true;
  sp.values_set = false;
  invalidate_factor(h);
  return PGF_OK;
}

int pgf_sparse_set_border(pgf_handle h, int k) {
  if (!h) return PGF_INVALID;
  if (!h->sparse) return fail(h, PGF_INVALID, "pgf_sparse_set_border: banded handles only");
  if (k < 0 || k > 64) return fail(h, PGF_INVALID, "border size must be 0..64");
  if (!h->sp.active) return fail(h, PGF_NOT_READY, "pgf_sparse_set_pattern first");
  const int N = h->n + h->m;
  if (k > 0 && k >= N) return fail(h, PGF_INVALID, "the border must leave at least one band row");
  (void)hipSetDevice(h->device);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  SparseDev &sp = h->sp;
  const bool had = sp.bk > 0;
  sp_border_free(sp);
  invalidate_factor(h);
  if (k == 0 && !had) return PGF_OK;
  const int Nb = N - k, kp = (k + 15) / 16 * 16;
  const size_t band_doubles = (size_t)(Nb + 1) * sp.ldb;
  // band, C and D in one array: the plan's slots index it as a whole
  (void)hipFree(sp.band);
  sp.band = nullptr;
  if (k == 0) {
    HIPCHK(h, dalloc(&sp.band, (size_t)(N + 1) * sp.ldb));
    return PGF_OK;
  }
  if (band_doubles + (size_t)Nb * kp + (size_t)kp * kp > (size_t)INT32_MAX)
    return fail(h, PGF_INVALID, "band and border store exceed 2^31 entries");
  HIPCHK(h, dalloc(&sp.band, band_doubles + (size_t)Nb * kp + (size_t)kp * kp));
  sp.bk = k;
  sp.bkp = kp;
  sp.Nb = Nb;
  sp.bC = sp.band + band_doubles;
  sp.bDd = sp.bC + (size_t)Nb * kp;
  sp.bnchunk = (Nb + SP_BORDER_CHUNK - 1) / SP_BORDER_CHUNK;
  HIPCHK(h, dalloc(&sp.bY, ((size_t)Nb + 64) * kp));
  HIPCHK(h, dalloc(&sp.bS, (size_t)kp * kp));
  HIPCHK(h, dalloc(&sp.bpart, (size_t)sp.bnchunk * kp * kp));
  HIPCHK(h, dalloc(&sp.bpartv, (size_t)sp.bnchunk * 3 * kp));
  HIPCHK(h, dalloc(&sp.brb, (size_t)kp));
  HIPCHK(h, dalloc(&sp.bz, (size_t)kp));
  HIPCHK(h, hipMalloc((void **)&sp.bsflags, 4 * sizeof(int)));
  HIPCHK(h, hipMemsetAsync(sp.brb, 0, (size_t)kp * sizeof(double), h->stream));  // padding stays zero
  // the residual pairs: one per 256 band rows and one for the border rows
  int rc;
  if ((rc = sp_alloc_bred(h, std::max((N + 255) / 256, (Nb + 255) / 256 + 1)))) return rc;
  HIPCHK(h, hipMemsetAsync(sp.bred, 0, ((size_t)3 * sp.nred + 4) * sizeof(double), h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PGF_OK;
}

int pgf_debug_border_stats(pgf_handle h, int *k, int *border_factorisations, int *border_solves) {
  if (!h) return PGF_INVALID;
  if (k) *k = h->sp.bk;
  if (border_factorisations) *border_factorisations = h->sp.stat_bfactor;
  if (border_solves) *border_solves = h->sp.stat_bsolve;
  return PGF_OK;
}

int pgf_sparse_set_border_large(pgf_handle h, int k) {
  if (!h) return PGF_INVALID;
  if (!h->sparse) return fail(h, PGF_INVALID, "pgf_sparse_set_border_large: banded handles only");
  if (k < 65 || k > 1024) return fail(h, PGF_INVALID, "large border size must be 65..1024");
  if (!h->sp.active) return fail(h, PGF_NOT_READY, "pgf_sparse_set_pattern first");
  const int N = h->n + h->m;
  if (k >= N) return fail(h, PGF_INVALID, "the border must leave at least one band row");
  SparseDev &sp = h->sp;
  if (sp.B <= 8) return fail(h, PGF_INVALID, "a large border needs a wide remainder (block size 16, 32 or 64)");
  if (!(sp.split && sp.bMr)) return fail(h, PGF_INVALID, "a large border needs the factor / solve split");
  (void)hipSetDevice(h->device);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  sp_border_free(sp);
  invalidate_factor(h);
  const int Nb = N - k, kp = (k + 63) / 64 * 64;
  const size_t band_doubles = (size_t)(Nb + 1) * sp.ldb;
  // band, C and D in one array: the plan's slots index it as a whole
  (void)hipFree(sp.band);
  sp.band = nullptr;
  if (band_doubles + (size_t)Nb * kp + (size_t)kp * kp > (size_t)INT32_MAX)
    return fail(h, PGF_INVALID, "band and border store exceed 2^31 entries");
  HIPCHK(h, dalloc(&sp.band, band_doubles + (size_t)Nb * kp + (size_t)kp * kp));
  sp.bk = k;
  sp.bkp = kp;
  sp.Nb = Nb;
  sp.bC = sp.band + band_doubles;
  sp.bDd = sp.bC + (size_t)Nb * kp;
  sp.bnchunk = (Nb + SP_BORDER_CHUNK - 1) / SP_BORDER_CHUNK;
  sp_borderL_gram_plan(Nb, kp, &sp.bgrows, &sp.bgchunks);
  const size_t ntiles = (size_t)(kp / 64) * (kp / 64 + 1) / 2;
  HIPCHK(h, dalloc(&sp.bY, ((size_t)Nb + 64) * kp));
  HIPCHK(h, dalloc(&sp.bS, (size_t)kp));  // here: the right-hand side of the solve with S
  HIPCHK(h, dalloc(&sp.bpart, (size_t)sp.bgchunks * ntiles * 4096));
  HIPCHK(h, dalloc(&sp.bpartv, (size_t)sp.bnchunk * 3 * kp));
  HIPCHK(h, dalloc(&sp.brb, (size_t)kp));
  HIPCHK(h, dalloc(&sp.bz, (size_t)kp));
  HIPCHK(h, dalloc(&sp.bG, (size_t)kp * kp));
  HIPCHK(h, hipMalloc((void **)&sp.bsflags, 4 * sizeof(int)));
  HIPCHK(h, hipMemsetAsync(sp.bsflags, 0, 4 * sizeof(int), h->stream));
  HIPCHK(h, hipMemsetAsync(sp.brb, 0, (size_t)kp * sizeof(double), h->stream));  // padding stays zero
  sp.blf = new (std::nothrow) DenseLdlt();
  if (!sp.blf) return fail(h, PGF_INVALID, "out of memory");
  HIPCHK(h, ldlt_alloc(*sp.blf, kp, h->stream));
  sp.blf->chain_solves = false;  // (no host synchronisation of its own behind a solve phase)
  HIPCHK(h, hipMemsetAsync(sp.blf->K, 0, ((size_t)kp + 1 + PGF_NB) * sp.blf->ldk * sizeof(double), h->stream));
  // the residual pairs: one per 256 band rows and one per 256 border rows
  int rc;
  if ((rc = sp_alloc_bred(h, std::max((N + 255) / 256, (Nb + 255) / 256 + (k + 255) / 256)))) return rc;
  HIPCHK(h, hipMemsetAsync(sp.bred, 0, ((size_t)3 * sp.nred + 4) * sizeof(double), h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PGF_OK;
}

int pgf_debug_border_gram(pgf_handle h, double *Cout, double *Yout, double *Gout) {
  if (!h) return PGF_INVALID;
  const SparseDev &sp = h->sp;
  if (!h->sparse || !sp_border_large(sp)) return fail(h, PGF_INVALID, "pgf_debug_border_gram: no large border");
  if (!sp.bgram_ready) return fail(h, PGF_NOT_READY, "no factor phase has run on this border yet");
  (void)hipSetDevice(h->device);
  const size_t panel = (size_t)sp.Nb * sp.bkp * sizeof(double);
  int rc;
  if (Cout && (rc = down(h, Cout, sp.bC, panel))) return rc;
  if (Yout && (rc = down(h, Yout, sp.bY, panel))) return rc;
  if (Gout && (rc = down(h, Gout, sp.bG, (size_t)sp.bkp * sp.bkp * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PGF_OK;
}

int pgf_debug_border_gram_plan(pgf_handle h, int *rows, int *chunks, int *tiles) {
  if (!h) return PGF_INVALID;
  const SparseDev &sp = h->sp;
  if (!h->sparse || !sp_border_large(sp)) return fail(h, PGF_INVALID, "pgf_debug_border_gram_plan: no large border");
  if (rows) *rows = sp.bgrows;
  if (chunks) *chunks = sp.bgchunks;
  if (tiles) *tiles = (sp.bkp / 64) * (sp.bkp / 64 + 1) / 2;
  return PGF_OK;
}

int pgf_debug_border_gram_time(pgf_handle h, int reps, double *ms_mfma, double *ms_fma) {
  if (!h || !ms_mfma || !ms_fma || reps < 1) return PGF_INVALID;
  const SparseDev &sp = h->sp;
  if (!h->sparse || !sp.bk || sp.bkp % 64) return fail(h, PGF_INVALID, "pgf_debug_border_gram_time: a border with kp a multiple of 64");
  if (!sp.stat_bfactor) return fail(h, PGF_NOT_READY, "no factor phase has run on this border yet");
  (void)hipSetDevice(h->device);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, sp_borderL_gram_time(h->stream, sp, reps, ms_mfma, ms_fma));
  return PGF_OK;
}

int pgf_sparse_set_factor_split(pgf_handle h, int on) {
  if (!h) return PGF_INVALID;
  if (!h->sparse) return fail(h, PGF_INVALID, "pgf_sparse_set_factor_split: banded handles only");
  SparseDev &sp = h->sp;
  const bool want = on != 0;
  if (want == sp.split) return PGF_OK;
  if (!want && sp_border_large(sp))
    return fail(h, PGF_INVALID, "a large border needs the factor / solve split");
  (void)hipSetDevice(h->device);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  sp.split = want;
  sp.kept = 0;
  invalidate_factor(h);  // (a bordered band's factor phase depends on the route too)
  for (double **q : {&sp.bMr, &sp.bMl})
    if (*q) {
      (void)hipFree(*q);
      *q = nullptr;
    }
  if (want && sp.active && sp.B > 8) {
    const size_t Bk = (size_t)sp.B, nbk = (size_t)sp.bstride;
    HIPCHK(h, dalloc(&sp.bMr, nbk * Bk * Bk));
    HIPCHK(h, dalloc(&sp.bMl, nbk * Bk * Bk));
  }
  return PGF_OK;
}

int pgf_debug_band_stats(pgf_handle h, int *reductions, int *solve_phases, int *panel_solves) {
  if (!h) return PGF_INVALID;
  if (reductions) *reductions = h->sp.stat_bw_reduce;
  if (solve_phases) *solve_phases = h->sp.stat_bw_solve;
  if (panel_solves) *panel_solves = h->sp.stat_bw_panel;
  return PGF_OK;
}

int pgf_sparse_set_block_size(pgf_handle h, int B) {
  if (!h) return PGF_INVALID;
  if (!h->sparse || !h->sp.active) return fail(h, PGF_NOT_READY, "pgf_sparse_set_pattern first");
  if (B != 0 && B != 8 && B != 16 && B != 32 && B != 64)
    return fail(h, PGF_INVALID, "block size must be 0 (automatic), 8, 16, 32 or 64");
  if (B != 0 && B < h->sp.bw)
    return fail(h, PGF_INVALID, "block size is smaller than the half-bandwidth");
  (void)hipSetDevice(h->device);
  const int want = B ? B : auto_block_size(h->sp.bw);
  if (want == h->sp.B) return PGF_OK;
  if (want == 8 && sp_border_large(h->sp))
    return fail(h, PGF_INVALID, "a large border needs a wide remainder (block size 16, 32 or 64)");
  int rc;
  if ((rc = sp_alloc_blocks(h, want))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  invalidate_factor(h);
  return PGF_OK;
}

int pgf_sparse_set_values(pgf_handle h, const double *Hval, const double *Jval) {
  if (!h) return PGF_INVALID;
  if (!h->sparse || !h->sp.active) return fail(h, PGF_NOT_READY, "pgf_sparse_set_pattern first");
  if ((h->sp.nnzH && !Hval) || (h->sp.nnzJ && !Jval)) return fail(h, PGF_INVALID, "null values");
  (void)hipSetDevice(h->device);
  int rc;
  if ((rc = up(h, h->sp.Hval, Hval, (size_t)h->sp.nnzH * sizeof(double)))) return rc;
  if ((rc = up(h, h->sp.Jval, Jval, (size_t)h->sp.nnzJ * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->sp.values_set = true;
  h->ls.hat_fresh = false;
  h->derivs_set = true;
  invalidate_factor(h);
  return PGF_OK;
}

}  // extern "C"
