// The batch's read-outs and hooks behind the C ABI: residual norms, termination measures, points and
// masks of every instance, the profile of the trailing-update launches, and the counters the
// pgf_batch_debug_* hooks report (pgf_batch_s::dbg).  Host code only.
#include <cstring>

#include "pgf_api_internal.h"
#include "pgf_kernels.h"

int pgf_batch_residual_norms(pgf_batch b, double *norms_out, double *norms_out_dev) {
  if (!b) return PGF_INVALID;
  if (!b->outer_set) return bfail(b, PGF_NOT_READY, "pgf_batch_advance_outer first");
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  (void)hipSetDevice(b->device);
  batch_eval(b);
  batch_launch_res_norm(b->stream, b->tab, b->B, b->sc, b->out.norm);
  if (norms_out_dev)
    BHIPCHK(b, hipMemcpyAsync(norms_out_dev, b->out.norm, b->B * sizeof(double),
                              hipMemcpyDeviceToDevice, b->stream));
  BHIPCHK(b, hipMemcpyAsync(b->out.h_norm, b->out.norm, b->B * sizeof(double), hipMemcpyDeviceToHost,
                            b->stream));
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  if (norms_out) std::memcpy(norms_out, b->out.h_norm, b->B * sizeof(double));
  return PGF_OK;
}

int pgf_batch_measures(pgf_batch b, double active_tol, double *out) {
  if (!b || !out) return PGF_INVALID;
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  (void)hipSetDevice(b->device);
  if (!b->outer_set) return bfail(b, PGF_NOT_READY, "pgf_batch_advance_outer first");
  batch_eval(b);
  if (b->band.on) {
    band_batch_measures_eval(b);
    batch_launch_measures_final(b->stream, b->tab, b->B, b->sc, active_tol, b->out.red4, b->out.meas);
  } else {
    batch_launch_measures(b->stream, b->tab, b->B, b->sc, PGF_GEMVT_PARTS, active_tol, b->out.red4,
                          b->out.meas);
  }
  b->eval_fresh = false;  // tmpn / w were reused
  BHIPCHK(b, hipMemcpyAsync(b->out.h_meas, b->out.meas, (size_t)b->B * 4 * sizeof(double),
                            hipMemcpyDeviceToHost, b->stream));
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  std::memcpy(out, b->out.h_meas, (size_t)b->B * 4 * sizeof(double));
  return PGF_OK;
}

int pgf_batch_get_points(pgf_batch b, double *x, double *y) {
  if (!b) return PGF_INVALID;
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  (void)hipSetDevice(b->device);
  for (int i = 0; i < b->B; ++i) {
    if (x && b->n)
      BHIPCHK(b, hipMemcpyAsync(x + (size_t)i * b->n, b->hs[i]->x, b->n * sizeof(double),
                                hipMemcpyDeviceToHost, b->stream));
    if (y && b->m)
      BHIPCHK(b, hipMemcpyAsync(y + (size_t)i * b->m, b->hs[i]->y, b->m * sizeof(double),
                                hipMemcpyDeviceToHost, b->stream));
  }
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  return PGF_OK;
}

int pgf_batch_get_masks(pgf_batch b, uint8_t *mask) {
  if (!b || !mask) return PGF_INVALID;
  if (!b->have_mask) return bfail(b, PGF_NOT_READY, "no active set");
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  (void)hipSetDevice(b->device);
  for (int i = 0; i < b->B; ++i)
    if (b->n)
      BHIPCHK(b, hipMemcpyAsync(mask + (size_t)i * b->n, b->hs[i]->mask, b->n,
                                hipMemcpyDeviceToHost, b->stream));
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  return PGF_OK;
}

int pgf_batch_refinement_stats(pgf_batch b, int *repaired) {
  if (!b) return PGF_INVALID;
  if (repaired) *repaired = b->dbg.repaired;
  return PGF_OK;
}

int pgf_batch_profile_enable(pgf_batch b, int on) {
  if (!b) return PGF_INVALID;
  b->prof.enabled = on != 0;
  return PGF_OK;
}

// Accumulated device time of the K = LDLT_OB trailing-update launches since the last call and
// their algorithmic flops, from the reduced sizes of the last synchronised step.
int pgf_batch_profile_read(pgf_batch b, double *update_ms, int64_t *update_launches,
                           double *update_flops) {
  if (!b) return PGF_INVALID;
  if (b->step_pending) return bfail(b, PGF_NOT_READY, "pgf_batch_sync the previous step first");
  (void)hipSetDevice(b->device);
  BHIPCHK(b, hipStreamSynchronize(b->stream));
  PgfProfile &p = b->prof;
  double ms_sum = 0.0, fl_sum = 0.0;
  for (size_t i = 0; i < p.update_spans.size(); ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.update_spans[i].first, p.update_spans[i].second) == hipSuccess)
      ms_sum += ms;
    // update_flops[i] >= 0: first row of the launch's trailing region, K-depth LDLT_OB; < 0: the rank-m
    // launch of the condensed order over the whole lower triangle, K-depth = -value
    const double start = p.update_flops[i];
    for (int k = 0; k < b->B; ++k) {
      const double Nk = (double)(b->out.h_flags[BFL_STRIDE * k + BFL_NI] + (b->cond.last ? 0 : b->m));
      const double T = start < 0 ? Nk : Nk - start;
      const double depth = start < 0 ? -start : (double)LDLT_OB;
      if (T > 0) fl_sum += 2.0 * depth * (0.5 * T * (T + 1.0) + T);
    }
    p.pool.push_back(p.update_spans[i].first);
    p.pool.push_back(p.update_spans[i].second);
  }
  if (update_ms) *update_ms = ms_sum;
  if (update_launches) *update_launches = (int64_t)p.update_spans.size();
  if (update_flops) *update_flops = fl_sum;
  p.update_spans.clear();
  p.update_flops.clear();
  return PGF_OK;
}

// ---- the pgf_batch_debug_* hooks ------------------------------------------------------------------
int pgf_batch_debug_fail_next_helper(pgf_batch b) {
  if (!b) return PGF_INVALID;
  if (b->band.on) return bfail(b, PGF_INVALID, "band batch: no chain helpers");
  b->dbg.inject_helper_failure = 1;
  return PGF_OK;
}

int pgf_batch_debug_factor_kind(pgf_batch b) {
  if (!b || !b->stepped || b->band.on) return 0;
  return b->cond.last ? 2 : 1;
}

int batch_read_pairs(pgf_batch b, const int *pairs, int *first, int *second) {
  if (!first && !second) return PGF_OK;
  std::vector<int> cnt((size_t)2 * b->B, 0);
  if (pairs) {
    (void)hipSetDevice(b->device);
    BHIPCHK(b, hipStreamSynchronize(b->stream));
    BHIPCHK(b, hipMemcpy(cnt.data(), pairs, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < b->B; ++i) {
    if (first) first[i] = cnt[2 * (size_t)i];
    if (second) second[i] = cnt[2 * (size_t)i + 1];
  }
  return PGF_OK;
}

extern "C" int pgf_batch_debug_band_stats(pgf_batch b, int *reductions, int *assemblies) {
  if (!b) return PGF_INVALID;
  if (reductions) *reductions = b->dbg.band_reductions;
  if (assemblies) *assemblies = b->dbg.band_assemblies;
  return PGF_OK;
}

extern "C" int pgf_batch_debug_band_wide_stats(pgf_batch b, int *reductions, int *solve_phases,
                                               int *lean_steps) {
  if (!b) return PGF_INVALID;
  if (lean_steps) *lean_steps = b->dbg.band_lean;
  return batch_read_pairs(b, b->band.wcnt, reductions, solve_phases);
}

extern "C" int pgf_batch_debug_border_stats(pgf_batch b, int *factor_phases, int *solve_phases) {
  if (!b) return PGF_INVALID;
  return batch_read_pairs(b, b->band.sh.bk ? b->band.bcnt : nullptr, factor_phases, solve_phases);
}
