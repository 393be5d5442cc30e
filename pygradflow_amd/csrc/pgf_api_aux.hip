// Entry points of the C ABI that need nothing of the dense step: the handle's stream, the
// profiling read-out, the stand-alone linear solver pgf_ls_* and pgf_bench_update; and the
// pgf_debug_* hooks of the dense handle: test injections, counters (pgf_solver::dbg) and the host
// walks of the head and update plans.
#include <algorithm>
#include <cstring>
#include <new>

#include "pgf_api_internal.h"
#include "pgf_kernels.h"
#include "pgf_update_plan.h"

int pgf_stream(pgf_handle h, void **stream_out) {
  if (!h || !stream_out) return PGF_INVALID;
  *stream_out = (void *)h->stream;
  return PGF_OK;
}

int pgf_profile_enable(pgf_handle h, int on) {
  if (!h) return PGF_INVALID;
  h->prof.enabled = on != 0;
  h->prof.mode = on == 2 ? 2 : 1;
  return PGF_OK;
}

static void profile_collect(PgfProfile &p) {
  for (size_t i = 0; i < p.update_spans.size(); ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.update_spans[i].first, p.update_spans[i].second) == hipSuccess)
      p.acc_update_ms += ms;
    p.acc_update_flops += p.update_flops[i];
    if (i < p.update_bytes.size()) p.acc_update_bytes += p.update_bytes[i];
    p.acc_update_launches += 1;
    p.pool.push_back(p.update_spans[i].first);
    p.pool.push_back(p.update_spans[i].second);
  }
  p.update_spans.clear();
  p.update_flops.clear();
  p.update_bytes.clear();
  auto drain = [&](std::vector<std::pair<hipEvent_t, hipEvent_t>> &v, double &acc, int64_t *cnt) {
    for (auto &sp : v) {
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, sp.first, sp.second) == hipSuccess) acc += ms;
      if (cnt) *cnt += 1;
      p.pool.push_back(sp.first);
      p.pool.push_back(sp.second);
    }
    v.clear();
  };
  for (size_t i = 0; i < p.fused_spans.size(); ++i) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.fused_spans[i].first, p.fused_spans[i].second) == hipSuccess)
      p.acc_fused_ms += ms;
    p.acc_fused_flops += p.fused_flops[i];
    p.acc_fused_bytes += p.fused_bytes[i];
    p.acc_fused_launches += 1;
    p.pool.push_back(p.fused_spans[i].first);
    p.pool.push_back(p.fused_spans[i].second);
  }
  p.fused_spans.clear();
  p.fused_flops.clear();
  p.fused_bytes.clear();
  drain(p.trsmud_spans, p.acc_trsmud_ms, nullptr);
  drain(p.factor_spans, p.acc_factor_ms, nullptr);
  drain(p.chain_spans, p.acc_chain_ms, &p.acc_chain_launches);
  drain(p.trsm_spans, p.acc_trsm_ms, nullptr);
  drain(p.udiag_spans, p.acc_udiag_ms, nullptr);
}

static void profile_reset(PgfProfile &p) {
  p.acc_update_ms = p.acc_update_flops = p.acc_update_bytes = p.acc_factor_ms = 0;
  p.acc_chain_ms = p.acc_trsm_ms = p.acc_udiag_ms = 0;
  p.acc_update_launches = p.acc_chain_launches = 0;
  p.acc_fused_ms = p.acc_fused_flops = p.acc_fused_bytes = p.acc_trsmud_ms = 0;
  p.acc_fused_launches = 0;
}

int pgf_profile_read(pgf_handle h, double *update_ms, int64_t *update_launches,
                     double *update_flops, double *factor_ms) {
  if (!h) return PGF_INVALID;
  (void)hipSetDevice(h->device);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  PgfProfile &p = h->prof;
  profile_collect(p);
  if (update_ms) *update_ms = p.acc_update_ms;
  if (update_launches) *update_launches = p.acc_update_launches;
  if (update_flops) *update_flops = p.acc_update_flops;
  if (factor_ms) *factor_ms = p.acc_factor_ms;
  profile_reset(p);
  return PGF_OK;
}

int pgf_profile_read_ex(pgf_handle h, double *out, int count) {
  if (!h || !out || count < PGF_PROF_COUNT) return PGF_INVALID;
  (void)hipSetDevice(h->device);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  PgfProfile &p = h->prof;
  profile_collect(p);
  out[PGF_PROF_UPDATE_MS] = p.acc_update_ms;
  out[PGF_PROF_UPDATE_LAUNCHES] = (double)p.acc_update_launches;
  out[PGF_PROF_UPDATE_FLOPS] = p.acc_update_flops;
  out[PGF_PROF_UPDATE_BYTES] = p.acc_update_bytes;
  out[PGF_PROF_FACTOR_MS] = p.acc_factor_ms;
  out[PGF_PROF_CHAIN_MS] = p.acc_chain_ms;
  out[PGF_PROF_CHAIN_LAUNCHES] = (double)p.acc_chain_launches;
  out[PGF_PROF_TRSM_MS] = p.acc_trsm_ms;
  out[PGF_PROF_UDIAG_MS] = p.acc_udiag_ms;
  if (count >= PGF_PROF_COUNT2) {
    out[PGF_PROF_FUSED_MS] = p.acc_fused_ms;
    out[PGF_PROF_FUSED_LAUNCHES] = (double)p.acc_fused_launches;
    out[PGF_PROF_FUSED_FLOPS] = p.acc_fused_flops;
    out[PGF_PROF_FUSED_BYTES] = p.acc_fused_bytes;
    out[PGF_PROF_TRSMUD_MS] = p.acc_trsmud_ms;
  }
  if (count >= PGF_PROF_COUNT3) {
    out[PGF_PROF_UNSYM_ASM_MS] = h->unsym.acc_unsym_asm_ms;
    out[PGF_PROF_UNSYM_ASM_LAUNCHES] = (double)h->unsym.acc_unsym_asm_launches;
    h->unsym.acc_unsym_asm_ms = 0;
    h->unsym.acc_unsym_asm_launches = 0;
  }
  profile_reset(p);
  return PGF_OK;
}

// ---------------------------------------------------------------- stand-alone linear solver
int pgf_ls_create_dense(int N, const double *A, int64_t lda, int symmetric, int device,
                        pgf_ls_handle *out) {
  if (!out || N < 0 || N > 60000 || (N && (!A || lda < N))) return PGF_INVALID;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return PGF_HIP_ERROR + (int)e;
  pgf_ls_handle ls = new (std::nothrow) pgf_linsolver();
  if (!ls) return PGF_INVALID;
  ls->N = N;
  ls->device = device;
  ls->symmetric = symmetric != 0;
  int rc = PGF_OK;
  do {
    if ((e = hipStreamCreateWithFlags(&ls->stream, hipStreamNonBlocking)) != hipSuccess) break;
    if ((e = dalloc(&ls->rhs, (size_t)N + 1)) != hipSuccess) break;
    if ((e = dalloc(&ls->sol, (size_t)N + 1)) != hipSuccess) break;
    if (!ls->symmetric) {  // LU with partial pivoting of the full matrix
      if ((e = lu_alloc(ls->lu, N, ls->stream)) != hipSuccess) break;
      if (N) {
        e = hipMemcpy2DAsync(ls->lu.A, (size_t)ls->lu.ld * sizeof(double), A,
                             (size_t)lda * sizeof(double), (size_t)N * sizeof(double), N,
                             hipMemcpyHostToDevice, ls->stream);
        if (e != hipSuccess) break;
      }
      const int st = lu_factor(ls->lu, &e);
      if (st < 0) break;
      if (st == 1) rc = PGF_SINGULAR;
      break;
    }
    if ((e = ldlt_alloc(ls->fac, N, ls->stream)) != hipSuccess) break;
    if (N) {
      e = hipMemcpy2DAsync(ls->fac.K, (size_t)ls->fac.ldk * sizeof(double), A,
                           (size_t)lda * sizeof(double), (size_t)N * sizeof(double), N,
                           hipMemcpyHostToDevice, ls->stream);
      if (e != hipSuccess) break;
    }
    if ((e = ldlt_factor_async(ls->fac, N, N)) != hipSuccess) break;
    int st = ldlt_finish(ls->fac, &e);
    if (st == 2) {  // chain helpers failed their checks (off now): upload and factorise again
      if (N) {
        e = hipMemcpy2DAsync(ls->fac.K, (size_t)ls->fac.ldk * sizeof(double), A,
                             (size_t)lda * sizeof(double), (size_t)N * sizeof(double), N,
                             hipMemcpyHostToDevice, ls->stream);
        if (e != hipSuccess) break;
      }
      if ((e = ldlt_factor_async(ls->fac, N, N)) != hipSuccess) break;
      st = ldlt_finish(ls->fac, &e);
      if (st == 2) rc = PGF_HIP_ERROR;
    }
    if (st < 0) break;
    if (st == 1) rc = PGF_SINGULAR;
  } while (0);
  if (e != hipSuccess) rc = PGF_HIP_ERROR + (int)e;
  if (rc != PGF_OK) {
    pgf_ls_destroy(ls);
    return rc;
  }
  *out = ls;
  return PGF_OK;
}

int pgf_ls_solve(pgf_ls_handle ls, const double *rhs, int trans, double *sol) {
  if (!ls || (ls->N && (!rhs || !sol))) return PGF_INVALID;
  if (ls->N == 0) return PGF_OK;
  (void)hipSetDevice(ls->device);
  hipError_t e = hipMemcpyAsync(ls->rhs, rhs, ls->N * sizeof(double), hipMemcpyHostToDevice,
                                ls->stream);
  if (!ls->symmetric) {
    if (e == hipSuccess) e = lu_solve_async(ls->lu, ls->rhs, ls->sol, trans);
    if (e == hipSuccess)
      e = hipMemcpyAsync(sol, ls->sol, ls->N * sizeof(double), hipMemcpyDeviceToHost, ls->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ls->stream);
    return e == hipSuccess ? PGF_OK : PGF_HIP_ERROR + (int)e;
  }
  if (e == hipSuccess) e = ldlt_solve_async(ls->fac, ls->rhs, ls->sol);
  if (e == hipSuccess)
    e = hipMemcpyAsync(sol, ls->sol, ls->N * sizeof(double), hipMemcpyDeviceToHost, ls->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ls->stream);
  if (e == hipSuccess && ldlt_chain_check(ls->fac)) {  // chain off now: per-block kernels
    e = ldlt_solve_async(ls->fac, ls->rhs, ls->sol);
    if (e == hipSuccess)
      e = hipMemcpyAsync(sol, ls->sol, ls->N * sizeof(double), hipMemcpyDeviceToHost, ls->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ls->stream);
    if (e == hipSuccess && ldlt_chain_check(ls->fac)) return PGF_HIP_ERROR;
  }
  return e == hipSuccess ? PGF_OK : PGF_HIP_ERROR + (int)e;
}

int pgf_ls_get_factor(pgf_ls_handle ls, double *LD_out, int64_t ld) {
  if (!ls || (ls->N && (!LD_out || ld < ls->N))) return PGF_INVALID;
  if (ls->N == 0) return PGF_OK;
  (void)hipSetDevice(ls->device);
  const double *src = ls->symmetric ? ls->fac.K : ls->lu.A;
  const int64_t lds = ls->symmetric ? ls->fac.ldk : ls->lu.ld;
  hipError_t e = hipMemcpy2DAsync(LD_out, (size_t)ld * sizeof(double), src,
                                  (size_t)lds * sizeof(double),
                                  (size_t)ls->N * sizeof(double), ls->N, hipMemcpyDeviceToHost,
                                  ls->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ls->stream);
  return e == hipSuccess ? PGF_OK : PGF_HIP_ERROR + (int)e;
}

int pgf_ls_num_neg(pgf_ls_handle ls, int *out) {
  if (!ls || !out) return PGF_INVALID;
  if (!ls->symmetric) return PGF_NOT_READY;  // an LU has no inertia (LUSolver returns None)
  *out = ls->fac.n_neg;
  return PGF_OK;
}

int pgf_ls_debug_lu(pgf_ls_handle ls, int *perm_out, int *reg_panels, int *streamed_panels) {
  if (!ls) return PGF_INVALID;
  if (ls->symmetric) return PGF_NOT_READY;  // an LDL^T does not pivot
  if (reg_panels) *reg_panels = ls->lu.reg_panels;
  if (streamed_panels) *streamed_panels = ls->lu.streamed_panels;
  if (!perm_out || ls->N == 0) return PGF_OK;
  (void)hipSetDevice(ls->device);
  hipError_t e = hipMemcpyAsync(perm_out, ls->lu.perm, (size_t)ls->N * sizeof(int),
                                hipMemcpyDeviceToHost, ls->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ls->stream);
  return e == hipSuccess ? PGF_OK : PGF_HIP_ERROR + (int)e;
}

int pgf_ls_destroy(pgf_ls_handle ls) {
  if (!ls) return PGF_OK;
  (void)hipSetDevice(ls->device);
  if (ls->stream) (void)hipStreamSynchronize(ls->stream);
  ldlt_free(ls->fac);
  lu_free(ls->lu);
  if (ls->rhs) (void)hipFree(ls->rhs);
  if (ls->sol) (void)hipFree(ls->sol);
  if (ls->stream) (void)hipStreamDestroy(ls->stream);
  delete ls;
  return PGF_OK;
}

int pgf_bench_update(int N, int KB, int variant, int reps, int device, double *ms_out,
                     double *flops_out) {
  if (N <= 0 || KB <= 0 || KB % 16 || reps <= 0 || !ms_out || !flops_out) return PGF_INVALID;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = ldlt_bench_update(N, KB, variant, reps, ms_out, flops_out);
  return e == hipSuccess ? PGF_OK : PGF_HIP_ERROR + (int)e;
}

int pgf_debug_fail_next_chain(pgf_handle h) {
  if (!h) return PGF_INVALID;
  h->fac.inject_chain_failure = 1;
  return PGF_OK;
}

int pgf_debug_chain_enable(int on) {
  ldlt_chain_set_enabled(on != 0);
  return PGF_OK;
}

int pgf_debug_fail_next_helper(pgf_handle h) {
  if (!h) return PGF_INVALID;
  h->fac.inject_helper_failure = 1;
  return PGF_OK;
}

int pgf_debug_step_stats(pgf_handle h, int *host_syncs, int *redone_steps) {
  if (!h) return PGF_INVALID;
  if (host_syncs) *host_syncs = h->dbg.stat_host_syncs;
  if (redone_steps) *redone_steps = h->dbg.stat_redone;
  return PGF_OK;
}

int pgf_debug_handback_stats(pgf_handle h, int *by_word, int *fell_back) {
  if (!h) return PGF_INVALID;
  if (by_word) *by_word = h->dbg.stat_hb_word;
  if (fell_back) *fell_back = h->dbg.stat_hb_fallback;
  return PGF_OK;
}

int pgf_debug_handback_spin_bound(pgf_handle h, double seconds) {
  if (!h) return PGF_INVALID;
  h->hb.bound_override = seconds;
  return PGF_OK;
}

int pgf_debug_front_stats(pgf_handle h, int *general, int *unbounded) {
  if (!h) return PGF_INVALID;
  if (general) *general = h->dbg.stat_compactions;
  if (unbounded) *unbounded = h->dbg.stat_unb_fronts;
  return PGF_OK;
}

int pgf_debug_gram_stats(pgf_handle h, int *builds, int *factorisations_with_gram) {
  if (!h) return PGF_INVALID;
  if (builds) *builds = h->dbg.stat_gram_builds;
  if (factorisations_with_gram) *factorisations_with_gram = h->dbg.stat_gram_factors;
  return PGF_OK;
}

int pgf_debug_tail_stats(pgf_handle h, int *fused_steps, int *plain_steps) {
  if (!h) return PGF_INVALID;
  if (fused_steps) *fused_steps = h->dbg.stat_tail_fused;
  if (plain_steps) *plain_steps = h->dbg.stat_tail_plain;
  return PGF_OK;
}

int pgf_debug_head_stats(pgf_handle h, int *fused, int *plain) {
  if (!h) return PGF_INVALID;
  if (fused) *fused = h->dbg.stat_head_fused;
  if (plain) *plain = h->dbg.stat_head_plain;
  return PGF_OK;
}

// The head workers' unit list, walked on the host (no GPU): k_units[i * N + j] counts the units
// that write entry (i, j) of K, k_head the same for the head launch's row groups, v_units the
// units per entry of V ((nI + 1) x mp: the tail row last) -- N = nI in the condensed layout
// (V: m columns padded to mp = a multiple of 32), nI + m in the natural one (no V).  The entry
// tests are those of b_assemble_kkt and the panel's tile body.
int pgf_debug_head_plan(int nI, int m, int condensed, int *k_units, int *k_head, int *v_units, int *n_units) {
  if (nI < 0 || m < 0) return PGF_INVALID;
  const int N = condensed ? nI : nI + m, mp = condensed ? round_up32(m) : 0;
  // (the list as head_unit defines it; ldlt_head_wanted fuses nothing for N <= 256, whose list is
  // the panel's tiles alone)
  const int total = head_asm_units(N) + head_panel_units(nI, mp);
  if (n_units) *n_units = total;
  auto rows = [&](int *cnt, int cb, int rg) {
    if (cb * 256 >= N || cb * 256 > rg * HEAD_ASM_ROWS + HEAD_ASM_ROWS - 1) return;
    for (int i = rg * HEAD_ASM_ROWS; i < (rg + 1) * HEAD_ASM_ROWS; ++i)
      for (int j = cb * 256; j < cb * 256 + 256; ++j)
        if (i < N && j <= i && j < N) ++cnt[(size_t)i * N + j];
  };
  if (k_head)
    for (int rg = 0; rg < (std::min(N, LDLT_OB) + HEAD_ASM_ROWS - 1) / HEAD_ASM_ROWS; ++rg) rows(k_head, 0, rg);
  for (int u = 0; u < total; ++u) {
    const HeadUnit hu = head_unit(u, N, nI, mp);
    if (hu.kind == 0 && k_units) rows(k_units, hu.a, hu.b);
    if (hu.kind == 1 && v_units) {
      for (int i = hu.a * 32; i < hu.a * 32 + 32; ++i)
        for (int r = hu.b * 32; r < hu.b * 32 + 32; ++r)
          if (i < nI && r < mp) ++v_units[(size_t)i * mp + r];
      if (hu.a == 0)
        for (int r = hu.b * 32; r < hu.b * 32 + 32; ++r)
          if (r < mp) ++v_units[(size_t)nI * mp + r];
    }
    if (hu.kind < 0) return PGF_INVALID;
  }
  return PGF_OK;
}

// The lazy update plan of a dense factorisation, walked on the host (no GPU, no handle): the
// jobs of every stage, and on request every tile of them as upd_tile -- the mapping the device
// workers run -- numbers it.
int pgf_debug_update_plan(int N, int nrows, int vdepth, int budget, int cap, int *jobs, int jobs_cap,
                          int *n_jobs, int *tiles, int tiles_cap, int *n_tiles, int *stage_jobs,
                          int *budget_out) {
  if (N < 1 || nrows < N || nrows > N + 1 || vdepth < 0 || vdepth % 32 || (budget >= 0 && cap < 1))
    return PGF_INVALID;
  UpdPlan made;
  if (budget >= 0) plan_updates(made, N, nrows, LDLT_OB, budget ? budget : UPD_NO_LIMIT, cap, vdepth);
  const UpdPlan &pl = budget >= 0 ? made : update_plan_for(N, nrows, vdepth, false);
  if (budget_out) *budget_out = pl.budget == UPD_NO_LIMIT ? 0 : pl.budget;
  const int nblk = (N + LDLT_OB - 1) / LDLT_OB;
  int nj = 0, nt = 0;
  for (int st = -1; st < nblk - 1; ++st) {
    UpdJobs none;
    none.njobs = 0;
    none.tile_begin[0] = 0;
    const UpdJobs &js = st >= 0 ? pl.launch[st] : (vdepth > 0 ? pl.first : none);
    if (stage_jobs) stage_jobs[st + 1] = js.njobs;
    for (int q = 0; q < js.njobs; ++q, ++nj) {
      if (!jobs || nj >= jobs_cap) continue;
      const int rec[PGF_UPDATE_PLAN_JOB_INTS] = {st,         js.col0[q], js.ntc[q], js.rowstart[q],     js.kc0v[q],
                                                 js.KBv[q],  js.kc0[q],  js.KB[q],  js.tile_begin[q],
                                                 js.tile_begin[q + 1]};
      std::memcpy(jobs + (size_t)PGF_UPDATE_PLAN_JOB_INTS * nj, rec, sizeof rec);
    }
    if (!tiles || tiles_cap <= 0) continue;
    for (int t = 0;; ++t, ++nt) {  // until the mapping itself says "past the end"
      int q, i0, j0;
      if (!upd_tile(js, t, N, nrows, q, i0, j0)) break;
      if (nt >= tiles_cap) continue;
      const int rec[4] = {st, q, i0, j0};
      std::memcpy(tiles + (size_t)4 * nt, rec, sizeof rec);
    }
  }
  if (n_jobs) *n_jobs = nj;
  if (n_tiles) *n_tiles = nt;
  return PGF_OK;
}

int pgf_debug_factor_kind(pgf_handle h) {
  if (!h || h->sparse) return 0;
  if (h->guard.lu_active) return 3;
  if (!h->fac.factored) return 0;
  return h->cond.condensed ? 2 : 1;
}

int pgf_debug_chain_helpers(int on) {
  const int was = ldlt_chain_helpers_enabled() ? 1 : 0;
  if (on == 0 || on == 1) ldlt_chain_helpers_set(on == 1);
  return was;
}
