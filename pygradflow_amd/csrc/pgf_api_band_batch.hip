// The banded half of the batch driver: pgf_batch_* for banded handles of one sparsity pattern, all
// on the narrow route -- with (PGF_BATCH_BORDER) one size of border or none -- or
// (PGF_BATCH_WIDE_BAND) all on the wide one, there with one size of border only under
// PGF_BATCH_WIDE_BORDER (pgf_api_batch.hip hands over in one line each;
// pgf_api_internal.h lists what is shared).  One launch sequence per Newton step for
// every instance -- the batched twins of the banded kernels (pgf_sparse.hip, pgf_band_wide.hip for
// the wide reduction, pgf_border.hip for a border) around the vector kernels the dense batch
// already has -- one host synchronisation per step (pgf_batch_sync) and one status copy for the whole
// batch.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>

#include "pgf_api_internal.h"
#include "pgf_kernels.h"

static const char *const k_zero_pivot = "zero or non-finite pivot in the banded KKT factorisation";

int band_batch_create(const pgf_handle *handles, int count, unsigned flags, pgf_batch *out) {
  const bool wide_ok = (flags & PGF_BATCH_WIDE_BAND) != 0;
  const bool border_ok = (flags & PGF_BATCH_BORDER) != 0;
  // (pgf_batch_create_ex has seen to it that the bit comes with the other two)
  const bool wide_border_ok = (flags & PGF_BATCH_WIDE_BORDER) != 0;
  const pgf_handle h0 = handles[0];
  // the reason goes to the offending handle and to the first one, where a caller of
  // pgf_batch_create looks for it
  auto fail = [&](pgf_handle h, int code, const char *msg) {
    h0->err = msg;
    return ::fail(h, code, msg);
  };
  for (int i = 0; i < count; ++i) {
    const pgf_handle h = handles[i];
    if (!h) return PGF_INVALID;
    if (!h->sparse || !h0->sparse)
      return fail(h, PGF_INVALID, "batch: dense and banded handles cannot share a batch");
    if (h->n != h0->n || h->m != h0->m || h->device != h0->device)
      return fail(h, PGF_INVALID, "batch: instances must share n, m and the device");
    if (h->unsym.form) return fail(h, PGF_INVALID, "batch: the Symmetric formulation only");
    const SparseDev &sp = h->sp;
    if (!sp.active || !sp.values_set)
      return fail(h, PGF_NOT_READY, "batch: pgf_sparse_set_pattern and pgf_sparse_set_values first");
    if (sp.bk && !border_ok) return fail(h, PGF_INVALID, "batch: a bordered band cannot join a device batch");
    if (sp.bk != h0->sp.bk) return fail(h, PGF_INVALID, "batch: banded instances must share the border size");
    if (sp.bk && sp.B != 8 && !wide_border_ok)
      return fail(h, PGF_INVALID,
                  "batch: a bordered band joins a device batch on the narrow route only (block size 8)");
    // (pgf_batch_create_ex has seen to it that PGF_BATCH_BORDER_CTL comes with the other two)
    if (sp.bk && (flags & PGF_BATCH_BAND_CTL) && !(flags & PGF_BATCH_BORDER_CTL))
      return fail(h, PGF_INVALID, "batch: the device-resident controller does not drive a bordered band batch");
    // (the wide border's phases are those of the handle under wide_kept, pgf_border.hip: B factorised
    // once, every solve against the kept factors)
    if (sp.bk && sp.B != 8 && !(sp.split && sp.bMr))
      return fail(h, PGF_INVALID, "batch: a bordered wide band needs the factor / solve split");
    if (sp.B != 8 && !wide_ok)
      return fail(h, PGF_INVALID, "batch: a wide band (block size above 8) cannot join a device batch");
    const SparseDev &s0 = h0->sp;
    if (sp.pat_hash != s0.pat_hash || sp.bw != s0.bw || sp.ldb != s0.ldb || sp.nnzH != s0.nnzH ||
        sp.nnzJ != s0.nnzJ)
      return fail(h, PGF_INVALID, "batch: banded instances must share one sparsity pattern");
    // (the split matters on the wide route only, and is in force only where the multipliers are
    // allocated: sp_cyclic_solve)
    if (sp.B != s0.B || (sp.B > 8 && (sp.split != s0.split || (sp.bMr != nullptr) != (s0.bMr != nullptr))))
      return fail(h, PGF_INVALID, "batch: banded instances must share the block size and the factor / solve split");
    if (!h->qp_mode || !h->bounds_set || !h->point_set)
      return fail(h, PGF_NOT_READY, "batch: pgf_set_bounds, pgf_qp_set_vectors, pgf_qp_set_point first");
    if (h->step_pending) return fail(h, PGF_NOT_READY, "batch: a step is pending");
  }
  pgf_batch b = new (std::nothrow) pgf_batch_s();
  if (!b) return PGF_INVALID;
  b->band = true;
  b->band_ctl = (flags & PGF_BATCH_BAND_CTL) != 0;
  b->ctl_refine = b->band_ctl && (flags & PGF_BATCH_CTL_REFINE) != 0;
  b->hs.assign(handles, handles + count);
  b->B = count;
  b->n = h0->n;
  b->m = h0->m;
  b->device = h0->device;
  b->sc.n = b->n;
  b->sc.m = b->m;
  b->frozen.assign(count, 0);
  b->last_neg.assign(count, 0);
  const int N = b->n + b->m;
  BandShape &sh = b->bsh;
  const SparseDev &s0 = h0->sp;
  // the sizes every instance shares, a border's included (bk was compared; bkp, Nb, bnchunk, nred
  // follow from it and N), the status block with the handle's own stride 3 nred + 4
  sh = band_shape_of(s0, N);
  sh.n = b->n;
  sh.m = b->m;
  const size_t cnt = (size_t)count, S = (size_t)3 * sh.nred + 4;
  (void)hipSetDevice(b->device);
  hipError_t e;
  if ((e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking)) != hipSuccess ||
      (e = hipMalloc((void **)&b->tab, cnt * sizeof(BInst))) != hipSuccess ||
      (e = hipMalloc((void **)&b->btab, cnt * sizeof(BandInst))) != hipSuccess ||
      (e = hipMalloc((void **)&b->ctl, cnt * 4 * sizeof(int))) != hipSuccess ||
      (e = hipMalloc((void **)&b->wcnt, cnt * 2 * sizeof(int))) != hipSuccess ||
      (e = hipMalloc((void **)&b->bcnt, cnt * 2 * sizeof(int))) != hipSuccess ||
      (e = hipMalloc((void **)&b->norm_out, cnt * sizeof(double))) != hipSuccess ||
      (e = hipMalloc((void **)&b->red4, cnt * 4 * ((size_t)(N + 255) / 256 + 1) * sizeof(double))) != hipSuccess ||
      (e = hipMalloc((void **)&b->meas_out, cnt * 4 * sizeof(double))) != hipSuccess ||
      (e = hipMalloc((void **)&b->ps, cnt * BPS_STRIDE * sizeof(double))) != hipSuccess ||
      (e = hipHostMalloc((void **)&b->h_ps, cnt * BPS_STRIDE * sizeof(double))) != hipSuccess ||
      (e = hipMalloc((void **)&b->bytes, cnt)) != hipSuccess ||
      (e = hipHostMalloc((void **)&b->h_bytes, cnt)) != hipSuccess ||
      (e = hipHostMalloc((void **)&b->h_meas, cnt * 4 * sizeof(double))) != hipSuccess ||
      (e = hipHostMalloc((void **)&b->h_flags, cnt * 3 * sizeof(int))) != hipSuccess ||
      (e = hipHostMalloc((void **)&b->h_norm, cnt * sizeof(double))) != hipSuccess ||
      (e = hipMalloc((void **)&b->bstat, cnt * S * sizeof(double))) != hipSuccess ||
      (e = hipHostMalloc((void **)&b->h_bstat, cnt * S * sizeof(double))) != hipSuccess) {
    pgf_batch_destroy(b);
    return PGF_HIP_ERROR + (int)e;
  }
  // what kbb_step_final writes for kb_dctl_mid / kb_dctl_end (zeroed: the guard is off and nothing
  // is counted until pgf_batch_ctl_init)
  if (b->band_ctl &&
      ((e = hipMalloc((void **)&b->flags_out, (cnt * 3 + 1) * sizeof(int))) != hipSuccess ||
       (e = hipMalloc((void **)&b->diff_out, cnt * sizeof(double))) != hipSuccess ||
       (e = hipMalloc((void **)&b->band_guard, cnt * BG_STRIDE * sizeof(double))) != hipSuccess ||
       (e = hipMalloc((void **)&b->band_rejects, cnt * 2 * sizeof(int))) != hipSuccess ||
       (e = hipMemset(b->flags_out, 0, (cnt * 3 + 1) * sizeof(int))) != hipSuccess ||
       (e = hipMemset(b->diff_out, 0, cnt * sizeof(double))) != hipSuccess ||
       (e = hipMemset(b->band_guard, 0, cnt * BG_STRIDE * sizeof(double))) != hipSuccess ||
       (e = hipMemset(b->band_rejects, 0, cnt * 2 * sizeof(int))) != hipSuccess)) {
    pgf_batch_destroy(b);
    return PGF_HIP_ERROR + (int)e;
  }
  // the refinement rounds' table, control words (written by each round's decision kernel before
  // anything reads them), measure and counters
  if (b->ctl_refine &&
      ((e = hipMalloc((void **)&b->rtab, cnt * sizeof(BandInst))) != hipSuccess ||
       (e = hipMalloc((void **)&b->rctl, cnt * 4 * sizeof(int))) != hipSuccess ||
       (e = hipMalloc((void **)&b->rcnt, cnt * 2 * sizeof(int))) != hipSuccess ||
       (e = hipMalloc((void **)&b->rrel, cnt * sizeof(double))) != hipSuccess ||
       (e = hipMemset(b->rctl, 0, cnt * 4 * sizeof(int))) != hipSuccess ||
       (e = hipMemset(b->rcnt, 0, cnt * 2 * sizeof(int))) != hipSuccess ||
       (e = hipMemset(b->rrel, 0, cnt * sizeof(double))) != hipSuccess)) {
    pgf_batch_destroy(b);
    return PGF_HIP_ERROR + (int)e;
  }
  std::memset(b->h_flags, 0, cnt * 3 * sizeof(int));
  std::vector<BInst> tab(count);
  std::vector<BandInst> btab(count);
  std::memset(tab.data(), 0, cnt * sizeof(BInst));
  for (int i = 0; i < count; ++i) {
    const pgf_handle h = handles[i];
    (void)hipStreamSynchronize(h->stream);
    const SparseDev &sp = h->sp;
    // what the vector kernels shared with the dense batch read (no dense matrix, no factor)
    BInst &t = tab[i];
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
    t.flags = h->fac.flags;
    BandInst &u = btab[i];
    u = band_inst_of(sp, h->fac.flags, b->bstat + S * i);
    u.wcnt = b->wcnt + 2 * i;
    u.bcnt = b->bcnt + 2 * i;
    u.lb = h->lb;
    u.ub = h->ub;
    u.q = h->q;
    u.b = h->b;
    u.x = h->x;
    u.y = h->y;
    u.xn = h->xn;
    u.yn = h->yn;
    u.g = h->g;
    u.c = h->c;
    u.w = h->w;
    u.F = h->F;
    u.b0full = h->b0full;
    u.dx = h->dx;
    u.dy = h->dy;
    u.tmpn = h->tmpn;
    u.mask = h->mask;
    u.counts = h->counts;
    u.ctl = b->ctl + 4 * i;
    u.ps = b->ps + (size_t)BPS_STRIDE * i;
    // the batch owns the device-side state of the handle from here on
    h->mask_set = false;
    h->eval_fresh = false;
    h->sp.stat_pending = false;
    h->sp.kept = 0;  // (the batch's reductions write the handle's block arrays)
    invalidate_factor(h);
  }
  std::memset(b->h_ps, 0, cnt * BPS_STRIDE * sizeof(double));
  if ((e = hipMemcpy(b->tab, tab.data(), cnt * sizeof(BInst), hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(b->btab, btab.data(), cnt * sizeof(BandInst), hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemset(b->ctl, 0, cnt * 4 * sizeof(int))) != hipSuccess ||
      (e = hipMemset(b->wcnt, 0, cnt * 2 * sizeof(int))) != hipSuccess ||
      (e = hipMemset(b->bcnt, 0, cnt * 2 * sizeof(int))) != hipSuccess ||
      (e = hipMemset(b->bstat, 0, cnt * S * sizeof(double))) != hipSuccess ||
      (e = hipMemcpy(b->ps, b->h_ps, cnt * BPS_STRIDE * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) {
    pgf_batch_destroy(b);
    return PGF_HIP_ERROR + (int)e;
  }
  if (b->ctl_refine) {
    for (int i = 0; i < count; ++i) btab[i].ctl = b->rctl + 4 * i;
    if ((e = hipMemcpy(b->rtab, btab.data(), cnt * sizeof(BandInst), hipMemcpyHostToDevice)) != hipSuccess) {
      pgf_batch_destroy(b);
      return PGF_HIP_ERROR + (int)e;
    }
  }
  *out = b;
  return PGF_OK;
}

void band_batch_free(pgf_batch b) {
  if (b->btab) (void)hipFree(b->btab);
  if (b->wcnt) (void)hipFree(b->wcnt);
  if (b->bcnt) (void)hipFree(b->bcnt);
  if (b->bstat) (void)hipFree(b->bstat);
  if (b->h_bstat) (void)hipHostFree(b->h_bstat);
  if (b->band_guard) (void)hipFree(b->band_guard);
  if (b->band_rejects) (void)hipFree(b->band_rejects);
  if (b->rtab) (void)hipFree(b->rtab);
  if (b->rctl) (void)hipFree(b->rctl);
  if (b->rcnt) (void)hipFree(b->rcnt);
  if (b->rrel) (void)hipFree(b->rrel);
}

// c = A x - b ; w = rho c + y ; g = Q x + (q + A' w) at every instance's point
void band_batch_eval(pgf_batch b) { bandb_launch_eval(b->stream, b->btab, b->B, b->bsh); }

// c = A x - b and F = Q x + q + A' y for the termination measures (no rho term)
void band_batch_measures_eval(pgf_batch b) { bandb_launch_measures_eval(b->stream, b->btab, b->B, b->bsh); }

// The step sequence of batch_enqueue_step for banded instances: eval, mask, rhs, assembly where
// needed, reduction, residual, step update, the evaluation made ahead of the sync, and the copy
// that brings the batch's status block to the host.  On the wide route the reduction is the launch
// sequence of pgf_band_wide.hip: extract, one invert + one reduce launch per level, last, one
// back launch per level, residual -- each instance in the phase its ctl[0] says.  With a border
// (either route) the assembly is the bordered one with its factor phase behind it -- Y, S and
// the factor of S, for the instances with ctl[0] != 0; on the wide route B is factorised there, once,
// by the factor-only KEEP reduction -- and the solve with B sits inside the solve phase, which every
// live instance runs: the 8 x 8 reduction, or on the wide route the solve against the kept factors
// (pgf_border.hip branches on the block size).
//
// band_batch_enqueue_step is the sequence up to the step update, for pgf_batch_step_async and for the
// device-resident controller's loop alike.  lean_allowed: the caller knows that every instance
// still live holds a clean factor of its band -- pgf_batch_step_async after a sync that found all
// instances good (all_factored), pgf_batch_ctl_iterate in front of the second step of an iteration.
void band_batch_enqueue_step(pgf_batch b, unsigned policy, double tau, bool lean_allowed) {
  const bool recompute = (policy & PGF_STEP_RECOMPUTE_MASK) != 0;
  const bool force = (policy & PGF_STEP_REFACTOR) != 0;
  // PGF_STEP_LINE_SEARCH (PGF_BATCH_LINE_SEARCH, no border): as in batch_enqueue_step -- g, c at the
  // outer points behind the evaluation, the mask from the current points, the residual and the step
  // update on the tables that name the outer points, nothing moved
  const bool search = (policy & PGF_STEP_LINE_SEARCH) != 0;
  hipStream_t s = b->stream;
  if (!b->eval_fresh) {
    band_batch_eval(b);
    b->eval_fresh = true;
  }
  if (search) batch_ls_eval_outer(b);
  batch_launch_mask(s, b->tab, b->B, b->sc, recompute ? (force ? 2 : 1) : 0, tau);
  b->have_mask = true;
  b->stepped = true;
  batch_launch_residual(s, search ? b->ls.otab : b->tab, b->B, b->sc);
  bandb_launch_rhs(s, b->btab, b->B, b->bsh);
  // instances whose band is still valid return at once (ctl[0] == 0); when the host knows that
  // none assembles (a Simplified step behind a good one), the launches are skipped
  if (b->bsh.bk) {
    // The factor phase's workgroups return at once where the band, Y and the factor of S are still
    // valid; when the host knows that no instance factors, all its launches are left out.
    if (recompute || !lean_allowed) {
      borderb_launch_factor(s, b->btab, b->B, b->bsh);
      ++b->stat_band_assemblies;
    } else {
      ++b->stat_band_lean;
    }
    borderb_launch_solve(s, b->btab, b->B, b->bsh);
    ++b->stat_band_reductions;
    bandb_launch_step_update(s, b->btab, b->B, b->bsh);
    b->eval_fresh = false;
    return;
  }
  if (recompute || !lean_allowed) {
    bandb_launch_assemble(s, b->btab, b->B, b->bsh);
    ++b->stat_band_assemblies;
  }
  if (b->bsh.B > 8) {
    // With the split on, an instance whose band is still valid solves against its kept factors.  When
    // the host knows that none reduces (a Simplified step behind a good one) the inversion launches
    // are left out: their workgroups would all return.
    const bool lean = b->bsh.split && !recompute && lean_allowed;
    bandb_launch_wide_solve(s, b->btab, b->B, b->bsh, lean);
    if (lean && b->bsh.N) ++b->stat_band_lean;
  } else {
    // (the 8 x 8 reduction keeps no factors: every step runs it, on the band as it stands)
    bandb_launch_solve(s, b->btab, b->B, b->bsh);
  }
  ++b->stat_band_reductions;
  bandb_launch_step_update(s, search ? b->ls.obtab : b->btab, b->B, b->bsh, /*move=*/!search);
  b->eval_fresh = false;
}

int band_batch_step_async(pgf_batch b, unsigned policy, double tau) {
  hipStream_t s = b->stream;
  band_batch_enqueue_step(b, policy, tau, b->all_factored);
  // (the Globalized policy: every instance's line search directly behind the step update)
  if (policy & PGF_STEP_LINE_SEARCH)
    if (int rc = batch_ls_enqueue_stage(b)) return rc;
  // g and c at the new points, ahead of the host synchronisation (as pgf_batch_step_async)
  if (eval_ahead()) {
    band_batch_eval(b);
    b->eval_fresh = true;
  }
  BHIPCHK(b, hipMemcpyAsync(b->h_bstat, b->bstat, (size_t)b->B * ((size_t)3 * b->bsh.nred + 4) * sizeof(double),
                            hipMemcpyDeviceToHost, s));
  BHIPCHK(b, hipGetLastError());
  b->step_pending = true;
  return PGF_OK;
}

// An instance whose normwise backward error misses refine_tol, on its own handle: the handle's
// buffers ARE the instance's, the band is intact, the solution is in sp.brhs and its residual in
// sp.bres.  The step update left the point the step started from in (xn, yn): it goes back, and
// band_refine corrects the solution and takes the step again from there.  The batch's stream is
// idle (band_batch_sync).  On the wide route with the split on, the handle holds the factors the
// batch's reduction left (the instance's flags were clean, or it would not be here): sp.kept says so
// for the length of the repair, and the corrections are solve phases against the instance's own
// multipliers, as the single handle's would be.  With a border, band_refine -> sp_cyclic_solve ->
// sp_border_solve and sp_cyclic_residual -> sp_border_residual run the solve phase against the
// handle's bY, bS and bsflags, which ARE the instance's and hold what the batch's factor phase left
// (valid: the instance's flags were clean); nothing on that path tests fac.factored or assembles
// again (read: band_refine, sp_cyclic_solve, sp_border_solve).  With a border on a wide remainder
// sp_cyclic_solve takes its sp.bk branch before it looks at sp.kept, and sp_border_solve takes
// wide_kept(sp) -- B > 8, split on, multipliers allocated: what band_batch_create admitted -- which
// puts the flags of B back from bsflags[2, 4) and runs sp_launch_bw_backsolve against bMr, bMl, bL,
// bU, bDinv: load, forward, x_0, backward, no inversion and no reduction of B (sp_launch_bw_factor
// is called from sp_border_factor alone, which only sp_assemble reaches, and band_refine never
// assembles).  All of these are the instance's arrays as the batch's factor phase left them.
// Returns 0 when the instance's step is good now.
//
// search (the step carried PGF_STEP_LINE_SEARCH): the step update moved nothing and the stage sat
// the instance out (kb_ls_ladder takes the same measure against the same tolerance), so the point is
// where the step found it and nothing goes back.  band_refine's corrections read the band, brhs and
// bres only; its step update reads the point, so the handle is in its entered state around it --
// (x, y) name the outer point's vectors, as while a single handle's Globalized step is in flight,
// where pgf_qp_sync calls the same band_refine -- and leaves the repaired clipped direction.  Then
// the handle's own ls_search, what pgf_qp_sync runs behind a settled step: PGF_LINE_SEARCH when it
// finds no trial.
static int band_batch_repair(pgf_batch b, int i, const double *st, double *diff_out, bool search) {
  pgf_handle h = b->hs[i];
  SparseDev &sp = h->sp;
  hipStream_t s = h->stream;
  const size_t S = (size_t)3 * sp.nred + 4;
  if (!search) {
    launch_copy(s, h->x, h->xn, h->n);
    launch_copy(s, h->y, h->yn, h->m);
  }
  std::memcpy(sp.h_bred, st, S * sizeof(double));
  sp.guarded = true;
  h->mask_set = true;
  sp.kept = b->bsh.split ? 2 : 0;
  if (search) batch_ls_handle_enter(b, i);
  const int refined = h->guard.stat_refined;
  int rc = band_refine(h, /*swapped=*/false, /*with_step=*/true);
  if (search) {
    ls_leave(h);
    b->ls.host_waits += h->guard.stat_refined - refined;  // (one wait per round)
  }
  sp.kept = 0;  // (outside a repair the handle's own view stays: no factors of its making)
  h->mask_set = false;
  if (rc) {
    (void)hipStreamSynchronize(s);  // (the point the step started from is back in place)
    return rc;
  }
  if (search) return batch_ls_handle_search(b, i, diff_out);
  launch_copy(s, h->x, h->xn, h->n);
  launch_copy(s, h->y, h->yn, h->m);
  HIPCHK(h, hipStreamSynchronize(s));
  *diff_out = h->h_scal[0];
  return PGF_OK;
}

int band_batch_sync(pgf_batch b, int *status, int *n_neg, double *diff) {
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  const bool search = b->ls.pending;
  b->ls.pending = false;
  if (search) {
    ++b->ls.host_waits;
    b->ls.have_stats = true;
  }
  const int nred = b->bsh.nred;
  const size_t S = (size_t)3 * nred + 4;
  bool all_ok = true;
  for (int i = 0; i < b->B; ++i) {
    pgf_handle h = b->hs[i];
    if (b->frozen[i]) {  // no step was taken
      all_ok = false;    // (whether its band is valid is the device's knowledge: ctl[1])
      if (status) status[i] = PGF_OK;
      if (n_neg) n_neg[i] = b->last_neg[i];
      if (diff) diff[i] = 0.0;
      continue;
    }
    const double *st = b->h_bstat + S * i;
    int rc = PGF_OK;
    double d = 0.0;
    if (b->bsh.N > 0) {
      const int bad = (int)st[3 * nred];
      b->last_neg[i] = (int)st[3 * nred + 1];
      if (bad) {
        rc = fail(h, PGF_SINGULAR, k_zero_pivot);  // (the step update left the point alone)
      } else {
        double sum = 0.0;
        for (int k = 0; k < nred; ++k) sum += st[2 * nred + k];
        d = std::sqrt(sum);
        const double rel = band_residual_rel_of(st, nred);
        h->guard.stat_last_rel = rel;
        if (h->guard.refine_mode && !(rel <= h->guard.refine_tol)) {
          rc = band_batch_repair(b, i, st, &d, search);
          b->eval_fresh = false;  // the instance moved after the evaluation made ahead
          if (search && rc == PGF_LINE_SEARCH) rc = PGF_OK;  // (repaired; its block says the rest)
          if (rc == PGF_OK) ++b->repaired;
          else if (rc != PGF_SINGULAR) return bfail(b, rc, pgf_last_error(h));
        }
      }
    }
    if (rc) all_ok = false;
    if (status) status[i] = rc ? PGF_SINGULAR : PGF_OK;
    if (n_neg) n_neg[i] = b->last_neg[i];
    if (diff) diff[i] = rc ? 0.0 : d;
    // (the Globalized policy: the instance's search decides its status and the length of its step)
    if (search && !rc) batch_ls_report(b, i, status, diff);
  }
  b->all_factored = all_ok;
  return PGF_OK;
}

// ---- the device-resident controller on a band batch (PGF_BATCH_BAND_CTL) ------------------------
// The loop itself is pgf_batch_ctl_iterate's; a banded step in it is band_batch_enqueue_step and,
// where band_batch_sync would finish the step on the host, kbb_step_final on the device.
void band_batch_enqueue_final(pgf_batch b) {
  bandb_launch_step_final(b->stream, b->btab, b->B, b->bsh, b->band_guard, b->diff_out, b->flags_out,
                          b->band_rejects, b->ctl_refine ? b->rctl : nullptr);
}

// PGF_BATCH_CTL_REFINE, between the step update and kbb_step_final: band_batch_sync ->
// band_batch_repair -> band_refine on the device, for the instances whose measure asks for it.  The
// host cannot know which: both rounds are enqueued, every launch of a round on the refinement table,
// whose ctl[3] the round's decision kernel has set for every instance that does not refine -- its
// workgroups return at once.  ctl[0] is 0 there: nothing assembles, a wide band with the split on
// solves against its kept factors (the step left them clean, or the instance would not refine), and
// the step update writes no ctl[1].  A round, per route, is band_refine's loop body: the copies,
// sp_cyclic_solve(guard = false), the axpy, sp_cyclic_residual, and the step taken again from the
// point it started from (which the load kernel has put back).  No factor phase is touched, so a
// lean second step stays lean; the round's solve counts as a solve phase in wcnt / bcnt (split off:
// as a reduction).
void band_batch_enqueue_refine(pgf_batch b) {
  hipStream_t s = b->stream;
  const BandShape &sh = b->bsh;
  const BandInst *rt = b->rtab;
  for (int round = 0; round < 2; ++round) {
    bandb_launch_refine_decide(s, b->btab, b->B, sh, b->band_guard, b->rctl, b->rrel, b->rcnt, round);
    bandb_launch_refine_load(s, rt, b->B, sh);
    if (sh.bk) {
      borderb_launch_solve(s, rt, b->B, sh, /*guard=*/false);
      bandb_launch_refine_axpy(s, rt, b->B, sh);
      borderb_launch_residual(s, rt, b->B, sh);
    } else if (sh.B > 8) {
      if (sh.split)
        bandb_launch_wide_kept_solve(s, rt, b->B, sh);
      else
        bandb_launch_wide_solve(s, rt, b->B, sh, /*lean=*/false, /*guard=*/false);
      bandb_launch_refine_axpy(s, rt, b->B, sh);
      bandb_launch_wide_residual(s, rt, b->B, sh);
    } else {
      bandb_launch_solve(s, rt, b->B, sh, /*residual=*/false, /*save_rhs=*/false);
      bandb_launch_refine_axpy(s, rt, b->B, sh);
      bandb_launch_residual(s, rt, b->B, sh);
    }
    bandb_launch_step_update(s, rt, b->B, sh);
  }
}

// the guard's setting of every handle, as it stands now (pgf_set_refinement), for kbb_step_final
// and the refinement rounds
int band_batch_ctl_init(pgf_batch b) {
  std::vector<double> g((size_t)BG_STRIDE * b->B);
  for (int i = 0; i < b->B; ++i) {
    g[BG_STRIDE * (size_t)i] = b->hs[i]->guard.refine_mode ? 1.0 : 0.0;
    g[BG_STRIDE * (size_t)i + 1] = b->hs[i]->guard.refine_tol;
    g[BG_STRIDE * (size_t)i + 2] = b->hs[i]->guard.refine_fail;
  }
  BHIPCHK(b, hipMemcpyAsync(b->band_guard, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice,
                            b->stream));
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  return PGF_OK;
}

// Behind the loop, stream idle: the host's view follows the device's.  The instances the controller
// froze in the last iteration stay frozen until the next pgf_batch_advance_outer*, so a host-driven
// pgf_batch_step_async right behind reports them as band_batch_sync reports frozen instances, with
// the inertia of the last step they took.  (No chain helpers here: the sticky word stays unused.)
int band_batch_ctl_read(pgf_batch b) {
  std::vector<int> ctl((size_t)4 * b->B), fl((size_t)3 * b->B);
  BHIPCHK(b, hipMemcpy(ctl.data(), b->ctl, ctl.size() * sizeof(int), hipMemcpyDeviceToHost));
  BHIPCHK(b, hipMemcpy(fl.data(), b->flags_out, fl.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int i = 0; i < b->B; ++i) {
    b->frozen[i] = ctl[4 * (size_t)i + 3] ? 1 : 0;
    if (b->dctl_logged > 0) b->last_neg[i] = fl[3 * (size_t)i + 1];
  }
  b->all_factored = false;
  return PGF_OK;
}

extern "C" int pgf_batch_debug_ctl_stats(pgf_batch b, int *pivot_rejects, int *guard_rejects) {
  if (!b) return PGF_INVALID;
  if (!pivot_rejects && !guard_rejects) return PGF_OK;
  std::vector<int> cnt((size_t)2 * b->B, 0);
  if (b->band_rejects) {
    (void)hipSetDevice(b->device);
    BHIPCHK(b, hipStreamSynchronize(b->stream));
    BHIPCHK(b, hipMemcpy(cnt.data(), b->band_rejects, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < b->B; ++i) {
    if (pivot_rejects) pivot_rejects[i] = cnt[2 * (size_t)i];
    if (guard_rejects) guard_rejects[i] = cnt[2 * (size_t)i + 1];
  }
  return PGF_OK;
}

extern "C" int pgf_batch_debug_ctl_refine_stats(pgf_batch b, int *refined_steps, int *rounds) {
  if (!b) return PGF_INVALID;
  if (!refined_steps && !rounds) return PGF_OK;
  std::vector<int> cnt((size_t)2 * b->B, 0);
  if (b->rcnt) {
    (void)hipSetDevice(b->device);
    BHIPCHK(b, hipStreamSynchronize(b->stream));
    BHIPCHK(b, hipMemcpy(cnt.data(), b->rcnt, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < b->B; ++i) {
    if (refined_steps) refined_steps[i] = cnt[2 * (size_t)i];
    if (rounds) rounds[i] = cnt[2 * (size_t)i + 1];
  }
  return PGF_OK;
}

extern "C" int pgf_batch_debug_band_stats(pgf_batch b, int *reductions, int *assemblies) {
  if (!b) return PGF_INVALID;
  if (reductions) *reductions = b->stat_band_reductions;
  if (assemblies) *assemblies = b->stat_band_assemblies;
  return PGF_OK;
}

extern "C" int pgf_batch_debug_band_wide_stats(pgf_batch b, int *reductions, int *solve_phases,
                                               int *lean_steps) {
  if (!b) return PGF_INVALID;
  if (lean_steps) *lean_steps = b->stat_band_lean;
  if (!reductions && !solve_phases) return PGF_OK;
  std::vector<int> cnt((size_t)2 * b->B, 0);
  if (b->band && b->wcnt) {
    (void)hipSetDevice(b->device);
    BHIPCHK(b, hipStreamSynchronize(b->stream));
    BHIPCHK(b, hipMemcpy(cnt.data(), b->wcnt, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < b->B; ++i) {
    if (reductions) reductions[i] = cnt[2 * i];
    if (solve_phases) solve_phases[i] = cnt[2 * i + 1];
  }
  return PGF_OK;
}

extern "C" int pgf_batch_debug_border_stats(pgf_batch b, int *factor_phases, int *solve_phases) {
  if (!b) return PGF_INVALID;
  if (!factor_phases && !solve_phases) return PGF_OK;
  std::vector<int> cnt((size_t)2 * b->B, 0);
  if (b->band && b->bsh.bk && b->bcnt) {
    (void)hipSetDevice(b->device);
    BHIPCHK(b, hipStreamSynchronize(b->stream));
    BHIPCHK(b, hipMemcpy(cnt.data(), b->bcnt, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < b->B; ++i) {
    if (factor_phases) factor_phases[i] = cnt[2 * (size_t)i];
    if (solve_phases) solve_phases[i] = cnt[2 * (size_t)i + 1];
  }
  return PGF_OK;
}
