// The Globalized policy on a device batch (PGF_BATCH_LINE_SEARCH; reference newton.py:218-304): what
// pgf_batch_step_async and pgf_batch_sync do in front of and behind the batched Newton step they
// share with the Full policy, for dense and banded batches alike.  The single handle renames its own
// (x, y, g, c) while such a step is in flight (ls_enter, pgf_api_line_search.hip); a batch's kernels
// read their vectors from per-instance tables, so the batch keeps a second table that names the
// OUTER point's vectors (otab / obtab) for the residual, the right-hand side and the step update, and
// a third (itab / ibtab) on which the batch's own evaluation launches form the direction's images.
// Behind the step update: images, kb_ls_ladder, kb_ls_finish -- a fixed number of launches for the
// whole batch -- and the copy of the instances' blocks, all in front of the step's one wait.
// Host code only.
#include <cstring>
#include <vector>

#include "pgf_api_internal.h"
#include "pgf_kernels.h"

static const char *const k_no_flag = "batch: created without PGF_BATCH_LINE_SEARCH";

int batch_ls_attach(pgf_batch b) {
  auto &ls = b->ls;
  const size_t cnt = (size_t)b->B;
  const int n = b->n, m = b->m, nb = (n + m + 255) / 256;
  const bool band = b->band.on;
  (void)hipSetDevice(b->device);
  for (pgf_handle h : b->hs) {
    if (int rc = ls_reserve(h)) return bfail(b, rc, pgf_last_error(h));
    h->ls.hat_fresh = false;  // (the batch evaluates into the handle's ghat, chat from here on)
    BHIPCHK(b, hipStreamSynchronize(h->stream));
  }
  hipError_t e = hipSuccess;
  batch_alloc(b, &e, &ls.ltab, cnt);
  batch_alloc(b, &e, &ls.blk, cnt * LSB_STRIDE, BA_ZERO);  // (the tickets start at zero)
  batch_alloc(b, &e, &ls.red, cnt * LS_TERMS * ((size_t)nb + 1));
  batch_alloc(b, &e, &ls.h_blk, cnt * LSB_STRIDE, BA_PINNED | BA_ZERO);
  if (band) {
    batch_alloc(b, &e, &ls.guard, cnt * 2, BA_ZERO);
    batch_alloc(b, &e, &ls.h_guard, cnt * 2, BA_PINNED);
  }
  // the tables that name the outer point's vectors and the direction with its images: the same
  // renaming for the BInst and the BandInst of an instance
  const std::vector<BInst> &tab = b->htab;
  auto outer = [&](auto &o, size_t i) {
    const pgf_handle h = b->hs[i];
    o.x = tab[i].xhat;
    o.y = tab[i].yhat;
    o.g = h->ls.ghat;
    o.c = h->ls.chat;
  };
  auto images = [&](auto &d, size_t i) {
    const pgf_handle h = b->hs[i];
    d.x = tab[i].dx;
    d.y = tab[i].dy;
    d.c = h->ls.u;
    d.g = h->ls.v;
    d.q = h->ls.zero;
    d.b = h->ls.zero;
  };
  batch_renamed_table(b, &e, &ls.otab, tab, outer);
  if (band) {
    batch_renamed_table(b, &e, &ls.obtab, b->band.htab, outer);
    batch_renamed_table(b, &e, &ls.ibtab, b->band.htab, images);
  } else {
    batch_renamed_table(b, &e, &ls.itab, tab, images);
  }
  BHIPCHK(b, e);
  std::vector<LsInst> lt(cnt);
  for (size_t i = 0; i < cnt; ++i) {
    const pgf_handle h = b->hs[i];
    const BInst &t = tab[i];
    LsInst &l = lt[i];
    l.x = t.x;
    l.y = t.y;
    l.xhat = t.xhat;
    l.yhat = t.yhat;
    l.dx = t.dx;
    l.dy = t.dy;
    l.g = t.g;
    l.c = t.c;
    l.v = h->ls.v;
    l.u = h->ls.u;
    l.slb = t.slb;
    l.sub = t.sub;
    l.lb = t.lb;
    l.ub = t.ub;
    l.red = ls.red + i * LS_TERMS * ((size_t)nb + 1);
    l.blk = ls.blk + i * LSB_STRIDE;
    l.ctl = t.ctl;
    l.ps = t.ps;
    // dense: the instance's word of out.flags, which kb_step_final has written by then (pivot,
    // hand-over and sampled-residual bits); band: its pivot flags, final behind the reduction
    l.bad = band ? h->fac.flags : b->out.flags + BFL_STRIDE * i + BFL_BAD;
    l.stat = band ? b->band.stat + i * band_stat_stride(b->band.sh) : nullptr;
    l.guard = band ? ls.guard + 2 * i : nullptr;
  }
  BHIPCHK(b, hipMemcpy(ls.ltab, lt.data(), cnt * sizeof(LsInst), hipMemcpyHostToDevice));
  ls.on = true;
  return PGF_OK;
}

void batch_ls_eval_outer(pgf_batch b) {
  auto &ls = b->ls;
  if (ls.hat_fresh) return;
  if (b->band.on)
    bandb_launch_eval(b->stream, ls.obtab, b->B, b->band.sh);
  else
    batch_launch_eval(b->stream, ls.otab, b->B, b->sc, PGF_GEMVT_PARTS);
  ls.hat_fresh = true;
}

// u = A dx, v = Q dx + A'(rho u + dy): the batch's evaluation on the image table (zero q and b), one
// pass over every H; then the two launches of the search.  The launches are counted as they are
// made: their number follows from n and m alone.
int batch_ls_enqueue_stage(pgf_batch b) {
  auto &ls = b->ls;
  hipStream_t s = b->stream;
  const int n = b->n, m = b->m;
  int launches = 0;
  if (b->band.on) {
    // (the guard's setting of every handle as it stands now, for the instances that sit the stage
    // out above their tolerance; the pinned pair is free: the last step was awaited)
    for (int i = 0; i < b->B; ++i) {
      ls.h_guard[2 * i] = b->hs[i]->guard.refine_mode ? 1.0 : 0.0;
      ls.h_guard[2 * i + 1] = b->hs[i]->guard.refine_tol;
    }
    BHIPCHK(b, hipMemcpyAsync(ls.guard, ls.h_guard, (size_t)b->B * 2 * sizeof(double), hipMemcpyHostToDevice, s));
    bandb_launch_eval(s, ls.ibtab, b->B, b->band.sh);
    launches += (m ? 1 : 0) + (n ? 1 : 0);
  } else if (n) {
    batch_launch_eval(s, ls.itab, b->B, b->sc, PGF_GEMVT_PARTS);
    launches += m ? 5 : 2;
  }
  batch_launch_ls_ladder(s, ls.ltab, b->B, n, m, b->band.on ? b->band.sh.nred : 0, ls.newton_tol);
  batch_launch_ls_finish(s, ls.ltab, b->B, n, m);
  if (n + m) launches += 2;
  ls.stage_launches = launches;
  ls.host_waits = 0;
  ls.pending = true;
  BHIPCHK(b, hipMemcpyAsync(ls.h_blk, ls.blk, (size_t)b->B * LSB_STRIDE * sizeof(double), hipMemcpyDeviceToHost, s));
  return PGF_OK;
}

void batch_ls_handle_enter(pgf_batch b, int i) { ls_enter_names(b->hs[i]); }

// The handle is in its own state again (ls_leave), its direction repaired, its point where the step
// found it: the stage sat the instance out.  ls_search evaluates g, c at that point afresh, forms the
// images, runs the single handle's ladder and finish and waits; on PGF_OK it has swapped the
// handle's point with (xn, yn), which the batch's tables cannot follow: swapped back, and copied.
int batch_ls_handle_search(pgf_batch b, int i, double *diff) {
  pgf_handle h = b->hs[i];
  auto &ls = b->ls;
  h->ls.newton_tol = ls.newton_tol;
  h->eval_fresh = false;
  drop_norm(h);
  const int before = h->dbg.stat_host_syncs;
  double d = 0.0;
  const int rc = ls_search(h, &d);
  ls.host_waits += h->dbg.stat_host_syncs - before;
  if (rc != PGF_OK && rc != PGF_LINE_SEARCH) return rc;
  double *blk = ls.h_blk + (size_t)LSB_STRIDE * i;
  std::memcpy(blk, h->ls.h_blk, LS_COPY * sizeof(double));
  blk[LSB_SAT_OUT] = 0.0;
  if (rc == PGF_OK) {
    swap_point(h);
    launch_copy(h->stream, h->x, h->xn, h->n);
    launch_copy(h->stream, h->y, h->yn, h->m);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ++ls.host_waits;
  }
  if (diff) *diff = rc == PGF_OK ? d : 0.0;
  return rc;
}

void batch_ls_report(pgf_batch b, int i, int *status, double *diff) {
  const double *blk = b->ls.h_blk + (size_t)LSB_STRIDE * i;
  if (blk[LSB_SAT_OUT] != 0.0) return;  // frozen, or a failed direction: reported by the step
  const bool failed = blk[LS_STATUS] != 0.0;
  if (failed) b->hs[i]->err = "Line search failed to converge";
  if (status) status[i] = failed ? PGF_LINE_SEARCH : PGF_OK;
  if (diff) diff[i] = failed ? 0.0 : blk[LS_DIFF];
}

extern "C" {

int pgf_batch_set_line_search(pgf_batch b, double newton_tol) {
  if (!b) return PGF_INVALID;
  if (!b->ls.on) return bfail(b, PGF_INVALID, k_no_flag);
  if (!(newton_tol >= 0.0)) return bfail(b, PGF_INVALID, "newton_tol must not be negative");
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  b->ls.newton_tol = newton_tol;
  for (pgf_handle h : b->hs) h->ls.newton_tol = newton_tol;
  return PGF_OK;
}

int pgf_batch_line_search_stats(pgf_batch b, double *alpha, int *trials, double *merit0, double *slope,
                                double *trial_merits) {
  if (!b) return PGF_INVALID;
  if (!b->ls.on) return bfail(b, PGF_INVALID, k_no_flag);
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  if (!b->ls.have_stats) return bfail(b, PGF_NOT_READY, "no step with PGF_STEP_LINE_SEARCH yet");
  for (int i = 0; i < b->B; ++i) {
    const double *blk = b->ls.h_blk + (size_t)LSB_STRIDE * i;
    if (alpha) alpha[i] = blk[LS_ALPHA];
    if (trials) trials[i] = (int)blk[LS_NTRIALS];
    if (merit0) merit0[i] = blk[LS_MERIT0];
    if (slope) slope[i] = blk[LS_SLOPE];
    if (trial_merits) std::memcpy(trial_merits + (size_t)LS_TRIALS * i, blk + LS_MERITS, LS_TRIALS * sizeof(double));
  }
  return PGF_OK;
}

int pgf_batch_debug_line_search_stats(pgf_batch b, int *stage_launches, int *host_waits) {
  if (!b) return PGF_INVALID;
  if (stage_launches) *stage_launches = b->ls.stage_launches;
  if (host_waits) *host_waits = b->ls.host_waits;
  return PGF_OK;
}

}  // extern "C"
