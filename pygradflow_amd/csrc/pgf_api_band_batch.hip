// The banded half of the batch driver: pgf_batch_* for banded handles of one sparsity pattern, all
// on the narrow route -- with (PGF_BATCH_BORDER) one size of border or none -- or
// (PGF_BATCH_WIDE_BAND) all on the wide one, there with one size of border only under
// PGF_BATCH_WIDE_BORDER (pgf_api_batch.hip hands over in one line each;
// pgf_api_internal.h lists what is shared).  One launch sequence per Newton step for
// every instance -- the batched twins of the banded kernels (pgf_sparse.hip, pgf_band_wide.hip for
// the wide reduction, pgf_border.hip for a border) around the vector kernels the dense batch
// already has -- one host synchronisation per step (pgf_batch_sync) and one status copy for the whole
// batch.  The banded steps of the device-resident controller's loop: pgf_api_batch_ctl.hip.
#include <cmath>
#include <cstring>
#include <new>

#include "pgf_api_internal.h"
#include "pgf_kernels.h"

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
    const char *msg = nullptr;
    int rc;
    if (!h->sparse || !h0->sparse)
      return fail(h, PGF_INVALID, "batch: dense and banded handles cannot share a batch");
    if ((rc = batch_check_shape(h, h0, &msg))) return fail(h, rc, msg);
    const SparseDev &sp = h->sp;
    if (!sp.active || !sp.pat.values_set)
      return fail(h, PGF_NOT_READY, "batch: pgf_sparse_set_pattern and pgf_sparse_set_values first");
    if (sp_border_large(sp))
      return fail(h, PGF_INVALID, "batch: a large border (more than 64 nodes) cannot join a device batch");
    if (sp.bor.bk && !border_ok) return fail(h, PGF_INVALID, "batch: a bordered band cannot join a device batch");
    if (sp.bor.bk != h0->sp.bor.bk) return fail(h, PGF_INVALID, "batch: banded instances must share the border size");
    if (sp.bor.bk && sp.blk.B != 8 && !wide_border_ok)
      return fail(h, PGF_INVALID,
                  "batch: a bordered band joins a device batch on the narrow route only (block size 8)");
    // (pgf_batch_create_ex has seen to it that PGF_BATCH_BORDER_CTL comes with the other two)
    if (sp.bor.bk && (flags & PGF_BATCH_BAND_CTL) && !(flags & PGF_BATCH_BORDER_CTL))
      return fail(h, PGF_INVALID, "batch: the device-resident controller does not drive a bordered band batch");
    // (the wide border's phases are those of the handle under wide_kept, pgf_border.hip: B factorised
    // once, every solve against the kept factors)
    if (sp.bor.bk && sp.blk.B != 8 && !(sp.blk.split && sp.blk.bMr))
      return fail(h, PGF_INVALID, "batch: a bordered wide band needs the factor / solve split");
    if (sp.blk.B != 8 && !wide_ok)
      return fail(h, PGF_INVALID, "batch: a wide band (block size above 8) cannot join a device batch");
    const SparseDev &s0 = h0->sp;
    if (sp.pat.hash != s0.pat.hash || sp.pat.bw != s0.pat.bw || sp.pat.ldb != s0.pat.ldb || sp.pat.nnzH != s0.pat.nnzH ||
        sp.pat.nnzJ != s0.pat.nnzJ)
      return fail(h, PGF_INVALID, "batch: banded instances must share one sparsity pattern");
    // (the split matters on the wide route only, and is in force only where the multipliers are
    // allocated: sp_cyclic_solve)
    if (sp.blk.B != s0.blk.B || (sp.blk.B > 8 && (sp.blk.split != s0.blk.split || (sp.blk.bMr != nullptr) != (s0.blk.bMr != nullptr))))
      return fail(h, PGF_INVALID, "batch: banded instances must share the block size and the factor / solve split");
    if ((rc = batch_check_state(h, /*band=*/true, &msg))) return fail(h, rc, msg);
  }
  pgf_batch b = new (std::nothrow) pgf_batch_s();
  if (!b) return PGF_INVALID;
  auto &bd = b->band;
  bd.on = true;
  bd.ctl = (flags & PGF_BATCH_BAND_CTL) != 0;
  bd.refine = bd.ctl && (flags & PGF_BATCH_CTL_REFINE) != 0;
  hipError_t e = batch_begin(b, handles, count);
  bd.frozen.assign(count, 0);
  bd.last_neg.assign(count, 0);
  const int N = b->n + b->m;
  BandShape &sh = bd.sh;
  // the sizes every instance shares, a border's included (bk was compared; bkp, Nb, bnchunk, nred
  // follow from it and N), the status block with the handle's own stride
  sh = band_shape_of(h0->sp, N);
  sh.n = b->n;
  sh.m = b->m;
  const size_t cnt = (size_t)count, S = band_stat_stride(sh);
  batch_alloc(b, &e, &b->tab, cnt);
  batch_alloc(b, &e, &bd.tab, cnt);
  batch_alloc(b, &e, &b->ctl, cnt * BCTL_STRIDE, BA_ZERO);
  batch_alloc(b, &e, &bd.wcnt, cnt * 2, BA_ZERO);
  batch_alloc(b, &e, &bd.bcnt, cnt * 2, BA_ZERO);
  batch_alloc(b, &e, &b->out.norm, cnt);
  batch_alloc(b, &e, &b->out.red4, cnt * 4 * ((size_t)(N + 255) / 256 + 1));
  batch_alloc(b, &e, &b->out.meas, cnt * 4);
  batch_alloc(b, &e, &b->ps, cnt * BPS_STRIDE, BA_ZERO);
  batch_alloc(b, &e, &b->h_ps, cnt * BPS_STRIDE, BA_PINNED | BA_ZERO);
  batch_alloc(b, &e, &b->bytes, cnt);
  batch_alloc(b, &e, &b->h_bytes, cnt, BA_PINNED);
  batch_alloc(b, &e, &b->out.h_meas, cnt * 4, BA_PINNED);
  batch_alloc(b, &e, &b->out.h_flags, cnt * BFL_STRIDE, BA_PINNED | BA_ZERO);
  batch_alloc(b, &e, &b->out.h_norm, cnt, BA_PINNED);
  batch_alloc(b, &e, &bd.stat, cnt * S, BA_ZERO);
  batch_alloc(b, &e, &bd.h_stat, cnt * S, BA_PINNED);
  // what kbb_step_final writes for kb_dctl_mid / kb_dctl_end (zeroed: the guard is off and nothing
  // is counted until pgf_batch_ctl_init)
  if (bd.ctl) {
    batch_alloc(b, &e, &b->out.flags, cnt * BFL_STRIDE + 1, BA_ZERO);
    batch_alloc(b, &e, &b->out.diff, cnt, BA_ZERO);
    batch_alloc(b, &e, &bd.guard, cnt * BG_STRIDE, BA_ZERO);
    batch_alloc(b, &e, &bd.rejects, cnt * 2, BA_ZERO);
  }
  // the refinement rounds' control words (written by each round's decision kernel before anything
  // reads them), measure and counters
  if (bd.refine) {
    batch_alloc(b, &e, &bd.rctl, cnt * BCTL_STRIDE, BA_ZERO);
    batch_alloc(b, &e, &bd.rcnt, cnt * 2, BA_ZERO);
    batch_alloc(b, &e, &bd.rrel, cnt, BA_ZERO);
  }
  b->htab.resize(cnt);  // (zeros: no dense matrix, no factor)
  bd.htab.resize(cnt);
  for (int i = 0; i < count && e == hipSuccess; ++i) {
    const pgf_handle h = handles[i];
    (void)hipStreamSynchronize(h->stream);
    // what the vector kernels shared with the dense batch read
    batch_fill_vectors(b, i, b->htab[i]);
    BandInst &u = bd.htab[i];
    u = band_inst_of(h->sp, h->fac.flags, bd.stat + S * i);
    u.wcnt = bd.wcnt + 2 * i;
    u.bcnt = bd.bcnt + 2 * i;
    batch_fill_vectors(b, i, u);
    batch_own_handle(h);
  }
  if (e == hipSuccess) e = hipMemcpy(b->tab, b->htab.data(), cnt * sizeof(BInst), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(bd.tab, bd.htab.data(), cnt * sizeof(BandInst), hipMemcpyHostToDevice);
  // the refinement rounds' table
  if (bd.refine)
    batch_renamed_table(b, &e, &bd.rtab, bd.htab, [&](BandInst &u, size_t i) { u.ctl = bd.rctl + BCTL_STRIDE * i; });
  if (e != hipSuccess) {
    pgf_batch_destroy(b);
    return PGF_HIP_ERROR + (int)e;
  }
  *out = b;
  return PGF_OK;
}

// c = A x - b ; w = rho c + y ; g = Q x + (q + A' w) at every instance's point
void band_batch_eval(pgf_batch b) { bandb_launch_eval(b->stream, b->band.tab, b->B, b->band.sh); }

// c = A x - b and F = Q x + q + A' y for the termination measures (no rho term)
void band_batch_measures_eval(pgf_batch b) {
  bandb_launch_measures_eval(b->stream, b->band.tab, b->B, b->band.sh);
}

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
  auto &bd = b->band;
  batch_eval(b);
  if (search) batch_ls_eval_outer(b);
  batch_launch_mask(s, b->tab, b->B, b->sc, recompute ? (force ? 2 : 1) : 0, tau);
  b->have_mask = true;
  b->stepped = true;
  batch_launch_residual(s, search ? b->ls.otab : b->tab, b->B, b->sc);
  bandb_launch_rhs(s, bd.tab, b->B, bd.sh);
  // instances whose band is still valid return at once (ctl[0] == 0); when the host knows that
  // none assembles (a Simplified step behind a good one), the launches are skipped
  if (bd.sh.bk) {
    // The factor phase's workgroups return at once where the band, Y and the factor of S are still
    // valid; when the host knows that no instance factors, all its launches are left out.
    if (recompute || !lean_allowed) {
      borderb_launch_factor(s, bd.tab, b->B, bd.sh);
      ++b->dbg.band_assemblies;
    } else {
      ++b->dbg.band_lean;
    }
    borderb_launch_solve(s, bd.tab, b->B, bd.sh);
    ++b->dbg.band_reductions;
    bandb_launch_step_update(s, bd.tab, b->B, bd.sh);
    b->eval_fresh = false;
    return;
  }
  if (recompute || !lean_allowed) {
    bandb_launch_assemble(s, bd.tab, b->B, bd.sh);
    ++b->dbg.band_assemblies;
  }
  if (bd.sh.B > 8) {
    // With the split on, an instance whose band is still valid solves against its kept factors.  When
    // the host knows that none reduces (a Simplified step behind a good one) the inversion launches
    // are left out: their workgroups would all return.
    const bool lean = bd.sh.split && !recompute && lean_allowed;
    bandb_launch_wide_solve(s, bd.tab, b->B, bd.sh, lean);
    if (lean && bd.sh.N) ++b->dbg.band_lean;
  } else {
    // (the 8 x 8 reduction keeps no factors: every step runs it, on the band as it stands)
    bandb_launch_solve(s, bd.tab, b->B, bd.sh);
  }
  ++b->dbg.band_reductions;
  bandb_launch_step_update(s, search ? b->ls.obtab : bd.tab, b->B, bd.sh, /*move=*/!search);
  b->eval_fresh = false;
}

int band_batch_step_async(pgf_batch b, unsigned policy, double tau) {
  hipStream_t s = b->stream;
  band_batch_enqueue_step(b, policy, tau, b->all_factored);
  // (the Globalized policy: every instance's line search directly behind the step update)
  if (policy & PGF_STEP_LINE_SEARCH)
    if (int rc = batch_ls_enqueue_stage(b)) return rc;
  // g and c at the new points, ahead of the host synchronisation (as pgf_batch_step_async)
  if (eval_ahead()) batch_eval(b);
  BHIPCHK(b, hipMemcpyAsync(b->band.h_stat, b->band.stat,
                            (size_t)b->B * band_stat_stride(b->band.sh) * sizeof(double),
                            hipMemcpyDeviceToHost, s));
  BHIPCHK(b, hipGetLastError());
  b->step_pending = true;
  return PGF_OK;
}

// An instance whose normwise backward error misses refine_tol, on its own handle: the handle's
// buffers ARE the instance's, the band is intact, the solution is in sp.vec.brhs and its residual in
// sp.vec.bres.  The step update left the point the step started from in (xn, yn): it goes back, and
// band_refine corrects the solution and takes the step again from there.  The batch's stream is
// idle (band_batch_sync).  On the wide route with the split on, the handle holds the factors the
// batch's reduction left (the instance's flags were clean, or it would not be here): sp.blk.kept says so
// for the length of the repair, and the corrections are solve phases against the instance's own
// multipliers, as the single handle's would be.  With a border, band_refine -> sp_cyclic_solve ->
// sp_border_solve and sp_cyclic_residual -> sp_border_residual run the solve phase against the
// handle's bY, bS and bsflags, which ARE the instance's and hold what the batch's factor phase left
// (valid: the instance's flags were clean); nothing on that path tests fac.factored or assembles
// again (read: band_refine, sp_cyclic_solve, sp_border_solve).  With a border on a wide remainder
// sp_cyclic_solve takes its sp.bor.bk branch before it looks at sp.blk.kept, and sp_border_solve takes
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
  const size_t S = band_stat_stride(b->band.sh);  // (the handle's own stride: create compared the shapes)
  if (!search) {
    launch_copy(s, h->x, h->xn, h->n);
    launch_copy(s, h->y, h->yn, h->m);
  }
  std::memcpy(sp.vec.h_bred, st, S * sizeof(double));
  sp.vec.guarded = true;
  h->mask_set = true;
  sp.blk.kept = b->band.sh.split ? 2 : 0;
  if (search) batch_ls_handle_enter(b, i);
  const int refined = h->guard.stat_refined;
  int rc = band_refine(h, /*swapped=*/false, /*with_step=*/true);
  if (search) {
    ls_leave(h);
    b->ls.host_waits += h->guard.stat_refined - refined;  // (one wait per round)
  }
  sp.blk.kept = 0;  // (outside a repair the handle's own view stays: no factors of its making)
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
  const bool search = batch_ls_begin_sync(b);
  auto &bd = b->band;
  const int nred = bd.sh.nred;
  const size_t S = band_stat_stride(bd.sh);
  bool all_ok = true;
  for (int i = 0; i < b->B; ++i) {
    pgf_handle h = b->hs[i];
    if (bd.frozen[i]) {  // no step was taken
      all_ok = false;    // (whether its band is valid is the device's knowledge: ctl[1])
      if (status) status[i] = PGF_OK;
      if (n_neg) n_neg[i] = bd.last_neg[i];
      if (diff) diff[i] = 0.0;
      continue;
    }
    const double *st = bd.h_stat + S * i;
    int rc = PGF_OK;
    double d = 0.0;
    if (bd.sh.N > 0) {
      const int bad = (int)st[3 * nred];
      bd.last_neg[i] = (int)st[3 * nred + 1];
      if (bad) {
        rc = fail(h, PGF_SINGULAR, k_band_zero_pivot);  // (the step update left the point alone)
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
          if (rc == PGF_OK) ++b->dbg.repaired;
          else if (rc != PGF_SINGULAR) return bfail(b, rc, pgf_last_error(h));
        }
      }
    }
    if (rc) all_ok = false;
    if (status) status[i] = rc ? PGF_SINGULAR : PGF_OK;
    if (n_neg) n_neg[i] = bd.last_neg[i];
    if (diff) diff[i] = rc ? 0.0 : d;
    // (the Globalized policy: the instance's search decides its status and the length of its step)
    if (search && !rc) batch_ls_report(b, i, status, diff);
  }
  b->all_factored = all_ok;
  return PGF_OK;
}
