// The device-resident step controller of a batch behind the C ABI: pgf_batch_ctl_init / _iterate /
// _read (the DistanceRatioController on the device) for dense batches and, created
// with PGF_BATCH_BAND_CTL, for band batches -- there with the step finished on the device
// (kbb_step_final) and, with PGF_BATCH_CTL_REFINE, refined on it.  A Newton step of the loop is the
// host-driven one's launch sequence (batch_enqueue_step, band_batch_enqueue_step).  Host code only.
#include <algorithm>
#include <cmath>

#include "pgf_api_internal.h"
#include "pgf_kernels.h"

// ---- the banded halves, called only from the loop below ------------------------------------------
// The loop itself is pgf_batch_ctl_iterate's; a banded step in it is band_batch_enqueue_step and,
// where band_batch_sync would finish the step on the host, kbb_step_final on the device.
static void band_batch_enqueue_final(pgf_batch b) {
  auto &bd = b->band;
  bandb_launch_step_final(b->stream, bd.tab, b->B, bd.sh, bd.guard, b->out.diff, b->out.flags, bd.rejects,
                          bd.refine ? bd.rctl : nullptr);
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
static void band_batch_enqueue_refine(pgf_batch b) {
  hipStream_t s = b->stream;
  auto &bd = b->band;
  const BandShape &sh = bd.sh;
  const BandInst *rt = bd.rtab;
  for (int round = 0; round < 2; ++round) {
    bandb_launch_refine_decide(s, bd.tab, b->B, sh, bd.guard, bd.rctl, bd.rrel, bd.rcnt, round);
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
static int band_batch_ctl_init(pgf_batch b) {
  std::vector<double> g((size_t)BG_STRIDE * b->B);
  for (int i = 0; i < b->B; ++i) {
    g[BG_STRIDE * (size_t)i] = b->hs[i]->guard.refine_mode ? 1.0 : 0.0;
    g[BG_STRIDE * (size_t)i + 1] = b->hs[i]->guard.refine_tol;
    g[BG_STRIDE * (size_t)i + 2] = b->hs[i]->guard.refine_fail;
  }
  BHIPCHK(b, hipMemcpyAsync(b->band.guard, g.data(), g.size() * sizeof(double), hipMemcpyHostToDevice,
                            b->stream));
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  return PGF_OK;
}

// Behind the loop, stream idle: the host's view follows the device's.  The instances the controller
// froze in the last iteration stay frozen until the next pgf_batch_advance_outer*, so a host-driven
// pgf_batch_step_async right behind reports them as band_batch_sync reports frozen instances, with
// the inertia of the last step they took.  (No chain helpers here: the sticky word stays unused.)
static int band_batch_ctl_read(pgf_batch b) {
  std::vector<int> ctl((size_t)BCTL_STRIDE * b->B), fl((size_t)BFL_STRIDE * b->B);
  BHIPCHK(b, hipMemcpy(ctl.data(), b->ctl, ctl.size() * sizeof(int), hipMemcpyDeviceToHost));
  BHIPCHK(b, hipMemcpy(fl.data(), b->out.flags, fl.size() * sizeof(int), hipMemcpyDeviceToHost));
  for (int i = 0; i < b->B; ++i) {
    b->band.frozen[i] = ctl[BCTL_STRIDE * (size_t)i + 3] ? 1 : 0;
    if (b->dctl.logged > 0) b->band.last_neg[i] = fl[BFL_STRIDE * (size_t)i + BFL_NEG];
  }
  b->all_factored = false;
  return PGF_OK;
}

// ---- device-resident DistanceRatioController ------------------------------
static const char *const k_band_ctl =
    "band batch: the device-resident controller is for dense batches (drive dt per instance with "
    "pgf_batch_advance_outer_each)";
int pgf_batch_ctl_init(pgf_batch b, double lamb_init, double rho, const double *params,
                       int max_iterations) {
  if (!b || !params || !(lamb_init > 0.0) || !(rho > 0.0) || max_iterations < 1) return PGF_INVALID;
  if (b->band.on && !b->band.ctl) return bfail(b, PGF_INVALID, k_band_ctl);
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  (void)hipSetDevice(b->device);
  auto &dc = b->dctl;
  const size_t ncs = (size_t)b->B * DCS_STRIDE;
  if (!dc.cs) BHIPCHK(b, dalloc(&dc.cs, ncs));
  if (!dc.cp) BHIPCHK(b, dalloc(&dc.cp, (size_t)DCP_COUNT));
  if (dc.log_cap < max_iterations) {
    if (dc.log) (void)hipFree(dc.log);
    dc.log = nullptr;
    BHIPCHK(b, dalloc(&dc.log, (size_t)max_iterations * b->B * 3));
    dc.log_cap = max_iterations;
  }
  std::vector<double> cs(ncs, 0.0), cp(DCP_COUNT, 0.0);
  for (int i = 0; i < b->B; ++i) {
    cs[(size_t)DCS_STRIDE * i + DCS_LAMB] = lamb_init;
    cs[(size_t)DCS_STRIDE * i + DCS_ACCEPTED] = 1.0;
  }
  cp[DCP_RHO] = rho;
  // params: newton_tol, lamb_red, lamb_min, lamb_inc, theta_max, K_P, K_I, theta_ref
  cp[DCP_NEWTON_TOL] = params[0];
  cp[DCP_LAMB_RED] = params[1];
  cp[DCP_LAMB_MIN] = params[2];
  cp[DCP_LAMB_INC] = params[3];
  cp[DCP_THETA_MAX] = params[4];
  cp[DCP_K_P] = params[5];
  cp[DCP_K_I] = params[6];
  if (!(params[7] > 0.0)) return bfail(b, PGF_INVALID, "theta_ref must be positive");
  cp[DCP_LOG_THETA_REF] = std::log(params[7]);
  BHIPCHK(b, hipMemcpyAsync(dc.cs, cs.data(), ncs * sizeof(double), hipMemcpyHostToDevice, b->stream));
  BHIPCHK(b, hipMemcpyAsync(dc.cp, cp.data(), DCP_COUNT * sizeof(double), hipMemcpyHostToDevice,
                            b->stream));
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  dc.logged = 0;
  if (b->band.on) return band_batch_ctl_init(b);
  return PGF_OK;
}

// One Newton step of the loop below, finished on the device: out.diff and out.flags are what
// kb_dctl_mid / kb_dctl_end read.  The host cannot know all_factored inside the loop; lean (band
// batches): what it can still know, see there.
static void ctl_enqueue_step(pgf_batch b, unsigned policy, double tau, bool lean) {
  if (b->band.on) {
    band_batch_enqueue_step(b, policy, tau, lean);
    // (PGF_BATCH_CTL_REFINE: the host cannot know which instances refine, so both rounds go in)
    if (b->band.refine) band_batch_enqueue_refine(b);
    band_batch_enqueue_final(b);
  } else {
    batch_enqueue_step(b, policy, tau, false);
  }
}

int pgf_batch_ctl_iterate(pgf_batch b, unsigned policy, double tau, int iterations) {
  if (!b || iterations < 0) return PGF_INVALID;
  if (policy & PGF_STEP_LINE_SEARCH)
    return bfail(b, PGF_INVALID, "batch: PGF_STEP_LINE_SEARCH is for host-driven steps (pgf_batch_step_async)");
  if (b->band.on && !b->band.ctl) return bfail(b, PGF_INVALID, k_band_ctl);
  auto &dc = b->dctl;
  if (!dc.cs) return bfail(b, PGF_NOT_READY, "pgf_batch_ctl_init first");
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  if (dc.logged + iterations > dc.log_cap)
    return bfail(b, PGF_INVALID, "more iterations than pgf_batch_ctl_init reserved a log for");
  const bool recompute = (policy & PGF_STEP_RECOMPUTE_MASK) != 0;
  if (!recompute && (policy & PGF_STEP_REFACTOR))
    return bfail(b, PGF_INVALID, "batch: PGF_STEP_REFACTOR needs PGF_STEP_RECOMPUTE_MASK");
  (void)hipSetDevice(b->device);
  hipStream_t s = b->stream;
  b->ls.hat_fresh = false;  // (the loop moves the outer points)
  for (int it = 0; it < iterations; ++it) {
    // outer step of every instance at its own lambda; rejected instances go back first
    batch_launch_dctl_begin(s, b->B, dc.cs, dc.cp, b->ps, b->bytes);
    batch_launch_advance(s, b->tab, b->B, b->sc, b->bytes);
    // (lambda lives on the device here: the host cannot bound the growth of the condensed order)
    b->cond.wanted = false;
    b->cond.free = true;
    b->eval_fresh = false;
    b->outer_set = true;
    if (!recompute) {  // Simplified: mask and derivatives frozen at the outer point
      batch_eval(b);
      batch_launch_mask(s, b->tab, b->B, b->sc, 2, tau);
    }
    // lambda has changed: every instance assembles and factorises (ctl[0], decided on the device)
    ctl_enqueue_step(b, policy, tau, false);
    batch_eval(b);
    batch_launch_res_norm(s, b->tab, b->B, b->sc, b->out.norm);
    batch_launch_dctl_mid(s, b->tab, b->B, dc.cs, dc.cp, b->out.diff, b->out.flags, b->out.norm);
    // Band batches, a policy that keeps the mask: the second step is enqueued without the assembly
    // and, on the wide route with the split on, without the inversion launches.  Every instance
    // still live has a clean factor of the band step one assembled: a bad pivot or a miss of the
    // guard in step one set its flag word, and kb_dctl_mid has frozen it for this step; the mask
    // is kept, so the band stays valid (ctl[1] = 1 from step one's update, ctl[0] = 0 here), and
    // the workgroups of the launches left out would all return.
    ctl_enqueue_step(b, policy, tau, !recompute);
    batch_launch_dctl_end(s, b->B, dc.cs, dc.cp, b->out.diff, b->out.flags,
                          dc.log + (size_t)dc.logged * b->B * 3);
    ++dc.logged;
  }
  b->all_factored = false;
  BHIPCHK(b, hipGetLastError());
  return PGF_OK;
}

int pgf_batch_ctl_read(pgf_batch b, double *lamb, uint8_t *accepted, double *log3, int log_rows) {
  if (!b) return PGF_INVALID;
  if (b->band.on && !b->band.ctl) return bfail(b, PGF_INVALID, k_band_ctl);
  auto &dc = b->dctl;
  if (!dc.cs) return bfail(b, PGF_NOT_READY, "pgf_batch_ctl_init first");
  (void)hipSetDevice(b->device);
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  // A failed hand-over of a chain helper or of a chained solve looked like a singular matrix to
  // the device-resident controller (kb_dctl_mid / _end: reject, 2 lambda) -- correct for that
  // iteration, but with the helpers still on it could repeat every iteration and lambda would
  // grow without bound.  The sticky word behind the flag triples says whether any
  // step of the loop saw one: helpers and chained solves go off, as pgf_batch_sync does.
  if (b->band.on) {
    if (int rc = band_batch_ctl_read(b)) return rc;  // (no helpers: the frozen flags instead)
  } else {
    int sticky = 0;
    BHIPCHK(b, hipMemcpy(&sticky, b->out.flags + BFL_STRIDE * (size_t)b->B, sizeof(int), hipMemcpyDeviceToHost));
    if (sticky) {
      BHIPCHK(b, batch_chain_off(b, /*every instance*/ -1));
      BHIPCHK(b, hipStreamSynchronize(b->stream));
    }
  }
  std::vector<double> cs((size_t)b->B * DCS_STRIDE);
  BHIPCHK(b, hipMemcpy(cs.data(), dc.cs, cs.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int i = 0; i < b->B; ++i) {
    if (lamb) lamb[i] = cs[(size_t)DCS_STRIDE * i + DCS_LAMB];
    if (accepted) accepted[i] = cs[(size_t)DCS_STRIDE * i + DCS_ACCEPTED] != 0.0;
    // the handles' host-side scalars follow the device's (the next host-driven call may use them)
    pgf_handle h = b->hs[i];
    const double l = cs[(size_t)DCS_STRIDE * i + DCS_USED];
    if (l > 0.0) set_outer_scalars(h, 1.0 / l, h->rho);
  }
  if (log3 && log_rows > 0) {
    const int rows = std::min(log_rows, dc.logged);
    BHIPCHK(b, hipMemcpy(log3, dc.log, (size_t)rows * b->B * 3 * sizeof(double),
                         hipMemcpyDeviceToHost));
  }
  return PGF_OK;
}

// ---- per-instance counters of the loop on a band batch (two ints each, counted on the device) ----
extern "C" int pgf_batch_debug_ctl_stats(pgf_batch b, int *pivot_rejects, int *guard_rejects) {
  if (!b) return PGF_INVALID;
  return batch_read_pairs(b, b->band.rejects, pivot_rejects, guard_rejects);
}

extern "C" int pgf_batch_debug_ctl_refine_stats(pgf_batch b, int *refined_steps, int *rounds) {
  if (!b) return PGF_INVALID;
  return batch_read_pairs(b, b->band.rcnt, refined_steps, rounds);
}
