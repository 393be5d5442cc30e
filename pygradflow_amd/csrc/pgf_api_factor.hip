// The factorisation of the dense Symmetric handle: the condensed system and its resident Gram
// matrix, the solves with the factor, enqueueing a factorisation (factor_async) and finishing it
// after the host synchronisation (finish_factor_state, factor_finish, factor_sync), pgf_factor,
// and adopt_batch_factor for the batch driver.  Host code only: the kernels are in
// pgf_kernels.hip / pgf_ldlt.hip / pgf_factor2.hip.
#include <cmath>
#include <vector>

#include "pgf_api_internal.h"
#include "pgf_env.h"
#include "pgf_kernels.h"

// ---- the condensed system ------------------------------------------------------------------
// K = [[A, J_I^T], [J_I, -delta I]], A = H[I,I] + lamb I.  Pivoting on the constraint block first
// (it is diagonal: nothing to factorise) leaves the nI x nI Schur complement S = A + J_I^T J_I /
// delta: m fewer pivots on the serial diagonal chain -- 16 column blocks instead of 20 at
// n = 4096, m = 1024 -- and N^3/3 -> nI^3/3 + nI^2 m flops, the second term as one more pending
// rank-m update of the look-ahead schedule (DenseLdlt::V, pgf_factor2.hip).  Same LDL^T of the
// same matrix in another (symmetric) pivot order; inertia = m + that of S.
//   S s_x = b_x + J_I^T b_y / delta,   s_y = (J_I s_x - b_y) / delta.
// The order is only stable while the eliminated block does not dwarf A: the growth
// ||J_I^T J_I / delta|| / ||A|| is bounded by g = ||J||_1 ||J||_inf / (delta (||H||_inf + lamb));
// beyond PGF_CONDENSED_GROWTH (default 1e3) the natural order is kept.  The residual guard
// (refine_if_needed) sees the full K either way.
// PGF_CONDENSED: 0 never, 1 (default) when it saves a column block, 2 whenever the growth allows
// (tests: the small golden cases).
int condensed_mode() { static const int v = env_int("PGF_CONDENSED", 1); return v; }
// The two a-priori bounds of the condensed order, from the norms of H and J in HBM (h_rs[4..6],
// residual_norms): (i) growth g = ||J||_1 ||J||_inf / (delta (||H||_inf + lamb)) <= 1e3
// (PGF_CONDENSED_GROWTH): the backward error of the block elimination is ~ eps g ||K||; (ii) the
// forward error that backward error can cost, eps g cond(K) with cond(K) <= ||K||_inf / min(lamb,
// delta) (K quasi-definite, H positive semi-definite), must stay below 1e-11 (PGF_CONDENSED_ERR):
// measured on the cond = 1.9e7 fixture (dt = 1e6, g = 100) the condensed order was 20 x less
// accurate than the natural one, 1e-8 against the reference's 6e-11.
bool condensed_growth_ok(pgf_handle h) {
  static const double gmax = env_double("PGF_CONDENSED_GROWTH", 1e3);
  static const double emax = env_double("PGF_CONDENSED_ERR", 1e-11);
  const double nH = h->guard.h_rs[4] + h->lamb;
  const double g = h->guard.h_rs[6] * h->guard.h_rs[5] / (h->delta * nH);
  const double nK = std::max(nH + h->guard.h_rs[6], h->guard.h_rs[5] + h->delta);
  return g <= gmax && 1.1e-16 * g * nK <= emax * std::min(h->lamb, h->delta);
}
static bool condensed_wanted(pgf_handle h) {
  const int mode = condensed_mode();
  if (!mode || h->cond.condensed_veto || h->m == 0 || h->nI == 0 || h->m > h->n) return false;
  if (mode == 1 && (h->m < 64 || (h->N + 255) / 256 <= (h->nI + 255) / 256)) return false;
  if (residual_norms(h)) return false;
  return condensed_growth_ok(h);
}
// row stride of the panel V: its depth rounded up to 32, plus 16 doubles -- at m = 1024 an 8 KB
// stride would put the 64 / 128 rows a tile stages on the same HBM channels (as pick_ldk for K)
int64_t condensed_ldv(int m) {
  const int mp = round_up32(m);
  static const bool pad = env_on("PGF_VPAD");
  return pad ? mp + 16 : mp;
}
hipError_t condensed_reserve(pgf_handle h) {
  DenseLdlt &f = h->fac;
  const int mp = round_up32(h->m);
  const size_t need = (size_t)(h->n + 1) * condensed_ldv(h->m);
  hipError_t e = hipSuccess;
  if (f.vcap < need) {
    if (f.V) (void)hipFree(f.V);
    f.V = nullptr;
    f.vcap = 0;
    if ((e = hipMalloc((void **)&f.V, need * sizeof(double))) != hipSuccess) return e;
    f.vcap = need;
  }
  if (f.vdcap < (size_t)mp) {
    if (f.vd) (void)hipFree(f.vd);
    f.vd = nullptr;
    f.vdcap = 0;
    if ((e = hipMalloc((void **)&f.vd, (size_t)mp * sizeof(double))) != hipSuccess) return e;
    f.vdcap = mp;
  }
  return e;
}

// The resident Gram matrix.  (J^T J)[I,I] = J_I^T J_I for every index set I: the rank-m term of S
// depends on J alone -- not on the mask, lamb, delta, rho or the point -- and J only changes with
// pgf_set_derivs_*.  With G = J^T J in HBM the assembly gathers S = H[I,I] + lamb I + G[I,I] / delta
// in its one pass (k_assemble_kkt_gram) and the factorisation runs without virtual blocks
// (vdepth = 0, no k_virtual_diag): n^2 m flops once per upload instead of nI^2 m in every
// factorisation.  The build reuses the trailing update's tiles (ldlt_gram_async) on the panel
// J^T of ALL n columns, which k_cond_panel writes for the identity index list.
// PGF_CONDENSED_GRAM: 0 never (the virtual blocks, as before), 1 (default) G is built at the SECOND
// condensed factorisation since the last upload -- a caller with fresh derivatives every step
// never pays for it --, 2 at the first (tests).
static int gram_mode() { static const int v = env_int("PGF_CONDENSED_GRAM", 1); return v; }
// true: h->cond.G holds J^T J for the matrices in HBM (built now if the rule says so); false: this
// factorisation takes the virtual-block path.  Never an error: a failed allocation switches the
// Gram path off for the handle.  (condensed_reserve has been called: f.V, f.vd hold n + 1 rows.)
static bool gram_prepare(pgf_handle h) {
  const int mode = gram_mode();
  if (!mode || h->cond.gram_off) return false;
  if (h->cond.gram_valid) return true;
  if (mode == 1 && h->cond.cond_since_upload < 1) return false;
  return gram_build(h);
}
// the build itself (also asked for by the device-resident Standard formulation, unsym_gram)
bool gram_build(pgf_handle h) {
  DenseLdlt &f = h->fac;
  const int n = h->n, mp = round_up32(h->m);
  if (!h->cond.G) {
    int64_t ld = ((int64_t)n + 15) / 16 * 16;  // (as pick_ldk: row starts off one HBM channel)
    if (ld % 512 == 0) ld += 16;
    std::vector<int> ident((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) ident[i] = i;
    if (hipMalloc((void **)&h->cond.G, (size_t)n * ld * sizeof(double)) != hipSuccess ||
        hipMalloc((void **)&h->cond.gram_aux, ((size_t)n + 1) * sizeof(int)) != hipSuccess ||
        hipMemcpy(h->cond.gram_aux, ident.data(), ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      if (h->cond.G) (void)hipFree(h->cond.G);
      if (h->cond.gram_aux) (void)hipFree(h->cond.gram_aux);
      h->cond.G = nullptr;
      h->cond.gram_aux = nullptr;
      h->cond.gram_off = true;
      return false;
    }
    h->cond.ldg = ld;
  }
  // V <- J^T (all columns), vd <- -1 (delta = 1); both are rewritten for this step right after
  launch_cond_panel(h->stream, f.V, condensed_ldv(h->m), mp, f.vd, h->J, h->ldj, h->cond.gram_aux, n, h->m, 1.0,
                    nullptr);
  if (ldlt_gram_async(h->stream, h->cond.G, h->cond.ldg, n, f.V, condensed_ldv(h->m), f.vd, mp, h->cond.gram_aux + n) !=
      hipSuccess) {
    (void)hipGetLastError();
    h->cond.gram_off = true;
    return false;
  }
  h->cond.gram_valid = true;
  ++h->dbg.stat_gram_builds;
  return true;
}
// the factorisation that was counted last is discarded and will be enqueued again
void gram_uncount(pgf_handle h) {
  if (h->flight.fac_counted) --h->cond.cond_since_upload;
  if (h->flight.fac_used_gram) --h->dbg.stat_gram_factors;
  if (h->flight.fac_head == 1) --h->dbg.stat_head_fused;
  if (h->flight.fac_head == 2) --h->dbg.stat_head_plain;
  h->flight.forget_factor();
}

// sol <- K^{-1} rhs with the current LDL^T factor (rhs, sol: N-vectors in the order
// [inactive variables; constraints]; rhs != sol)
hipError_t kkt_solve_async(pgf_handle h, const double *rhs, double *sol) {
  if (!h->cond.condensed) return ldlt_solve_async(h->fac, rhs, sol);
  DenseLdlt &f = h->fac;
  launch_cond_rhs(h->stream, h->nI, h->m, f.V, f.ldv, rhs, h->delta, h->cond.cd_t);
  hipError_t e = ldlt_solve_async(f, h->cond.cd_t, sol);
  if (e != hipSuccess) return e;
  launch_cond_y(h->stream, h->nI, h->m, f.V, f.ldv, sol, rhs + h->nI, h->delta, h->partial,
                (size_t)PGF_GEMVT_PARTS * (h->n ? h->n : 1), sol + h->nI);
  return hipGetLastError();
}
// the backward half for the right-hand side h->rhs that rode through the factorisation
// (cy: a condensed step leaves s_y to the step update that follows directly -- only the partial
// products are enqueued here, *cy describes them)
hipError_t kkt_backsolve_async(pgf_handle h, double *sol, StepCondY *cy) {
  DenseLdlt &f = h->fac;
  if (cy) cy->partial = nullptr;
  if (!h->cond.condensed) return ldlt_backsolve_async(f, f.K + (int64_t)h->N * f.ldk, sol);
  hipError_t e = ldlt_backsolve_async(f, f.K + (int64_t)h->nI * f.ldk, sol);
  if (e != hipSuccess) return e;
  const size_t cap = (size_t)PGF_GEMVT_PARTS * (h->n ? h->n : 1);
  if (cy && h->m) {
    cy->nparts = launch_cond_y_partial(h->stream, h->nI, h->m, f.V, f.ldv, sol, h->partial, cap);
    cy->partial = h->partial;
    cy->rhs_y = h->rhs + h->nI;
    cy->sol_y = sol + h->nI;
    cy->delta = h->delta;
    return hipGetLastError();
  }
  launch_cond_y(h->stream, h->nI, h->m, f.V, f.ldv, sol, h->rhs + h->nI, h->delta, h->partial, cap, sol + h->nI);
  return hipGetLastError();
}

// the assembly operands of a head descriptor (m: the constraint rows that go into K)
static LdltHead head_assembly(pgf_handle h, int nI, int m) {
  LdltHead hw;
  hw.H = h->H;
  hw.ldh = h->ldh;
  hw.J = h->J;
  hw.ldj = h->ldj;
  hw.idxI = h->idxI;
  hw.nI = nI;
  hw.m = m;
  hw.lamb = h->lamb;
  hw.delta = h->delta;
  return hw;
}
// pgf_debug_head_stats: the factorisation being enqueued, by kind (undone by gram_uncount)
static void count_head(pgf_handle h, bool fused) {
  ++(fused ? h->dbg.stat_head_fused : h->dbg.stat_head_plain);
  h->flight.fac_head = fused ? 1 : 2;
}

// enqueue assemble + factor; with_rhs: carry h->rhs through the elimination in the row behind the
// matrix.  Where ldlt_head_wanted, the assembly is not launched here but described in hw.
int factor_async(pgf_handle h, bool with_rhs) {
  if (h->sparse) return band_factor_async(h);
  DenseLdlt &f = h->fac;
  h->guard.lu_active = false;
  h->cond.condensed = condensed_wanted(h);
  f.vdepth = 0;
  f.vneg = 0;
  h->flight.forget_factor();
  const int nI = h->nI, Nf = h->cond.condensed ? nI : h->N;  // pivots of this factorisation
  double *row = f.K + (int64_t)Nf * f.ldk;               // the row behind them: the right-hand side's
  const double *row_src = with_rhs ? h->rhs : nullptr;
  LdltHead hw;
  bool head;
  if (h->cond.condensed) {
    HIPCHK(h, condensed_reserve(h));
    const int mp = round_up32(h->m);
    f.ldv = condensed_ldv(h->m);
    f.vneg = h->m;  // the eliminated block is -delta I
    const bool gram = gram_prepare(h);
    ++h->cond.cond_since_upload;
    h->flight.fac_counted = true;
    h->flight.fac_used_gram = gram;
    if (gram)
      ++h->dbg.stat_gram_factors;
    else
      f.vdepth = mp;  // the rank-m term as virtual blocks
    const double *rhs_y = with_rhs ? h->rhs + nI : nullptr;
    head = gram && ldlt_head_wanted(f, nI);
    if (head) {
      // Gram, all of it beside the first diagonal chain, which reads the first 256 rows only
      hw = head_assembly(h, nI, 0);
      hw.G = h->cond.G;
      hw.ldg = h->cond.ldg;
      hw.V = f.V;
      hw.ldv = f.ldv;
      hw.mp = mp;
      hw.pm = h->m;
      hw.vd = f.vd;
      hw.rhs_y = rhs_y;
      if (with_rhs) {
        hw.crhs = h->rhs;
        hw.crhs_out = row;
      }
    } else {
      if (gram)  // S = H[I,I] + lamb I + G[I,I] / delta in the assembly's one pass
        launch_assemble_kkt(h->stream, f.K, f.ldk, h->H, h->ldh, h->J, h->ldj, h->idxI, nI, 0, h->lamb, h->delta,
                            f.flags, 4 + LDLT_UPD_COUNTERS, nullptr, nullptr, 0, h->cond.G, h->cond.ldg);
      else  // virtual blocks: A = H[I,I] + lamb I (no constraint rows), b_x into row nI
        launch_assemble_kkt(h->stream, f.K, f.ldk, h->H, h->ldh, h->J, h->ldj, h->idxI, nI, 0, h->lamb, h->delta,
                            f.flags, 4 + LDLT_UPD_COUNTERS, row_src, row, nI);
      // V = J_I^T (it also serves the solves: launch_cond_rhs, launch_cond_y), b_y in its row nI
      launch_cond_panel(h->stream, f.V, f.ldv, mp, f.vd, h->J, h->ldj, h->idxI, nI, h->m, h->delta, rhs_y);
      // Gram: row nI of K <- b_x + J_I^T b_y / delta, which the virtual blocks produce on the way (in
      // place of k_virtual_diag: as many launches)
      if (gram && with_rhs) launch_cond_rhs(h->stream, nI, h->m, f.V, f.ldv, h->rhs, h->delta, row);
    }
  } else {
    head = ldlt_head_wanted(f, Nf);
    if (head) {
      hw = head_assembly(h, nI, h->m);
      if (with_rhs) {
        hw.row_src = h->rhs;
        hw.row_dst = row;
        hw.row_n = Nf;
      }
    } else {  // (the assembly launch also copies the rhs into row N)
      launch_assemble_kkt(h->stream, f.K, f.ldk, h->H, h->ldh, h->J, h->ldj, h->idxI, nI, h->m, h->lamb, h->delta,
                          f.flags, 4 + LDLT_UPD_COUNTERS, row_src, row, Nf);
    }
  }
  f.flags_zeroed = Nf > 0;  // (every assembly, launched or in hw, also clears the factorisation's flags)
  count_head(h, head);
  HIPCHK(h, ldlt_factor_async(f, Nf, Nf + (with_rhs ? 1 : 0), head ? &hw : nullptr));  // (sets f.N = Nf)
  return PGF_OK;
}

int finish_factor_state(pgf_handle h, hipError_t *e, bool awaited) {
  const int st = ldlt_finish(h->fac, e, awaited && !h->sparse);
  if (h->sparse && st >= 0) band_kept_resolve(h);
  if (st == 1 && h->cond.condensed && !h->cond.condensed_veto) {
    h->cond.condensed_veto = true;
    h->fac.factored = false;
    gram_uncount(h);
    return 2;
  }
  if (st == 2) gram_uncount(h);
  return st;
}

int factor_finish(pgf_handle h) {
  int rcs;
  if ((rcs = band_status_sync(h))) return rcs;
  hipError_t e;
  const int st = finish_factor_state(h, &e);
  if (st < 0) return hip_fail(h, e, "factor");
  if (st == 2) return PGF_RETRY_FACTOR;
  if (st == 1) return fail(h, PGF_SINGULAR, "zero or non-finite pivot in LDL^T of the KKT matrix");
  return PGF_OK;
}

// assemble + factorise (no right-hand side row) and wait
int factor_sync(pgf_handle h) {
  int rc;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if ((rc = factor_async(h, false))) return rc;
    if ((rc = factor_finish(h)) != PGF_RETRY_FACTOR) return rc;
  }
  return fail(h, PGF_HIP_ERROR, k_helper_msg);
}

// The batch driver's repair of one instance (batch_repair_instance): the handle is dressed as the
// holder of the factor the batch made for it -- nI inactive variables, in the condensed order or
// not, cond_mp the depth of its virtual blocks, n_neg_reported the negative pivots the batch's
// factorisation counted -- so that refine_if_needed and the solves take that factor for one of the
// handle's own (a full solve of a factored matrix, no LU).
void adopt_batch_factor(pgf_handle h, int nI, int n_neg_reported, bool condensed, int cond_mp) {
  h->nI = nI;
  h->nA = h->n - nI;
  h->N = nI + h->m;
  h->mask_set = true;
  h->cond.condensed = condensed;
  h->guard.lu_active = false;
  h->flight.last_solve = 2;
  DenseLdlt &f = h->fac;
  f.N = h->cond.condensed ? nI : h->N;
  f.vdepth = h->cond.condensed ? cond_mp : 0;
  f.ldv = condensed_ldv(h->m);
  f.vneg = h->cond.condensed ? h->m : 0;
  f.factored = true;
  f.n_neg = n_neg_reported + (h->cond.condensed ? h->m : 0);
}

int pgf_factor(pgf_handle h, int *n_neg) {
  if (!h) return PGF_INVALID;
  int rc;
  if ((rc = check_ready(h))) return rc;
  (void)hipSetDevice(h->device);
  if (h->unsym.form) {
    if (!h->unsym.ulu_ok && (rc = unsym_factor(h))) return rc;  // (the factor of the current matrix stays)
    if (n_neg) *n_neg = -1;
    return PGF_OK;
  }
  if ((rc = factor_sync(h))) return rc;
  if (n_neg) *n_neg = h->fac.n_neg;
  return PGF_OK;
}
