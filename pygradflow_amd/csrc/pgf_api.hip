// C ABI of libpgf_hip.so (include/pgf_hip.h): the dense Symmetric handle and the per-step
// orchestration of the kernels in pgf_kernels.hip / pgf_ldlt.hip, the device-resident LQ step
// included.  (pgf_hip.h declares every entry point extern "C": the definitions follow it.)
#include <cmath>
#include <cstdio>
#include <cstring>
#include <new>
#include <utility>

#include "pgf_api_internal.h"
#include "pgf_kernels.h"
#include "pgf_unsym.h"
#include "pgf_update_plan.h"

// PGF_EVAL_AHEAD=0: g and c at the new point are evaluated at the start of the next step, not
// ahead of the host synchronisation of this one (newton_core_async, enqueue_qp_step, pgf_batch_step_async)
bool eval_ahead() { static const bool ahead = env_on("PGF_EVAL_AHEAD"); return ahead; }

// PGF_STEP_FUSED=0: the launches in front of and behind the factorisation of a qp step as before --
// k_mask_compact + k_residual_rhs; k_cond_y, k_step_update, the J and H row passes, k_sum_partials2,
// k_kkt_residual; three launches in pgf_qp_advance_outer -- instead of the fused ones (same values)
static bool step_fused() { static const bool on = env_on("PGF_STEP_FUSED"); return on; }

int pgf_version(void) { return 1; }

int pgf_device_count(int *count) {
  if (!count) return PGF_INVALID;
  hipError_t e = hipGetDeviceCount(count);
  if (e != hipSuccess) {
    *count = 0;
    return PGF_HIP_ERROR + (int)e;
  }
  return PGF_OK;
}

const char *pgf_last_error(pgf_handle h) { return h ? h->err.c_str() : k_no_handle; }

int pgf_create(int n, int m, int device, unsigned flags, pgf_handle *out) {
  const bool sparse = (flags & PGF_CREATE_SPARSE) != 0;
  if (!out || n < 0 || m < 0 || (!sparse && (int64_t)n + m > 60000)) return PGF_INVALID;
  pgf_handle h = new (std::nothrow) pgf_solver();
  if (!h) return PGF_INVALID;
  h->n = n;
  h->m = m;
  h->device = device;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) {
    delete h;
    return PGF_HIP_ERROR + (int)e;
  }
#define A_(ptr, cnt)                                        \
  if ((e = dalloc(&h->ptr, (size_t)(cnt))) != hipSuccess) { \
    pgf_destroy(h);                                         \
    return PGF_HIP_ERROR + (int)e;                          \
  }
  if ((e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking)) != hipSuccess) {
    delete h;
    return PGF_HIP_ERROR + (int)e;
  }
  const int N = n + m;
  A_(lb, n) A_(ub, n) A_(slb, n) A_(sub, n) A_(xhat, n) A_(yhat, m);
  A_(x, n) A_(y, m) A_(xn, n) A_(yn, m) A_(g, n) A_(c, m) A_(F, N) A_(b0full, n);
  A_(rhs, N + 1) A_(sol, N + 1) A_(dx, n) A_(dy, m);
  // (partial: two sets of PGF_GEMVT_PARTS row chunks of n: launch_residual_and_eval carries two vectors)
  A_(q, n) A_(b, m) A_(w, m) A_(tmpn, n) A_(partial, (size_t)2 * PGF_GEMVT_PARTS * (n ? n : 1));
  A_(red, (N + 255) / 256 + 1) A_(meas, 4 * ((N + 255) / 256) + 4) A_(stat, STAT_ALLOC);
  if (!sparse) {
    A_(rs_v, n) A_(rs_lv, n) A_(rs_u, n) A_(rs_wy, m) A_(rs_r, N + 1) A_(rs_d, N + 1);
    A_(cd_t, n + 1);
  }
  A_(mask, n) A_(mask_new, n) A_(idxI, n) A_(idxA, n) A_(pos, n);
#undef A_
  // index lists hold valid indices from the start: a step enqueued with stale counts reads them
  if ((e = hipMemset(h->stat, 0, STAT_ALLOC * sizeof(double))) != hipSuccess ||
      (n && (e = hipMemset(h->idxI, 0, (size_t)n * sizeof(int))) != hipSuccess) ||
      (n && (e = hipMemset(h->idxA, 0, (size_t)n * sizeof(int))) != hipSuccess) ||
      (n && (e = hipMemset(h->pos, 0, (size_t)n * sizeof(int))) != hipSuccess) ||
      (e = hipHostMalloc((void **)&h->h_stat, STAT_COPY * sizeof(double))) != hipSuccess ||
      (e = hipHostMalloc((void **)&h->h_meas, 4 * sizeof(double))) != hipSuccess) {
    pgf_destroy(h);
    return PGF_HIP_ERROR + (int)e;
  }
  h->rs_red = h->stat;
  h->scal = h->stat + 8;
  h->counts = reinterpret_cast<int *>(h->stat + 12);
  h->ticket = reinterpret_cast<unsigned *>(h->stat + 16);
  for (int i = 0; i < STAT_COPY; ++i) h->h_stat[i] = 0.0;
  h->h_rs = h->h_stat;
  h->h_scal = h->h_stat + 8;
  h->h_counts = reinterpret_cast<int *>(h->h_stat + 12);
  h->sparse = sparse;
  h->sp.split = band_split_default();
  if (sparse) {
    // banded mode: no dense N x N storage; only the factor's flag words are shared
    h->fac.stream = h->stream;
    if ((e = hipMalloc((void **)&h->fac.flags, 4 * sizeof(int))) != hipSuccess ||
        (e = hipHostMalloc((void **)&h->fac.h_flags, 4 * sizeof(int))) != hipSuccess) {
      pgf_destroy(h);
      return PGF_HIP_ERROR + (int)e;
    }
    for (int i = 0; i < 4; ++i) h->fac.h_flags[i] = 0;
  } else if ((e = ldlt_alloc(h->fac, N, h->stream)) != hipSuccess) {
    pgf_destroy(h);
    return PGF_HIP_ERROR + (int)e;
  }
  h->fac.prof = &h->prof;
  *out = h;
  return PGF_OK;
}

int pgf_destroy(pgf_handle h) {
  if (!h) return PGF_OK;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  ldlt_chain_timing_dump();
  void *ptrs[] = {h->csr_ptr, h->csr_idx, h->csr_val, h->Hown, h->Jown, h->lb,  h->ub,   h->slb,  h->sub,      h->xhat, h->yhat,
                  h->x,    h->y,    h->xn,  h->yn,   h->g,    h->c,        h->F,    h->b0full,
                  h->rhs,  h->sol,  h->dx,  h->dy,   h->q,    h->b,        h->w,    h->tmpn,
                  h->partial, h->red, h->stat, h->mask, h->mask_new, h->idxI, h->idxA, h->pos,
                  h->meas, h->rs_v, h->rs_lv, h->rs_u, h->rs_wy, h->rs_r, h->rs_d, h->cd_t,
                  h->G,    h->gram_aux};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  if (h->h_stat) (void)hipHostFree(h->h_stat);
  if (h->h_mask_stage) (void)hipHostFree(h->h_mask_stage);
  if (h->mask_ev) (void)hipEventDestroy(h->mask_ev);
  lu_free(h->lu);
  lu_free(h->ulu);
  if (h->h_meas) (void)hipHostFree(h->h_meas);
  band_free(h);
  ldlt_free(h->fac);
  for (hipEvent_t e : h->prof.pool) (void)hipEventDestroy(e);
  for (auto &sp : h->prof.update_spans) {
    (void)hipEventDestroy(sp.first);
    (void)hipEventDestroy(sp.second);
  }
  for (auto &sp : h->prof.factor_spans) {
    (void)hipEventDestroy(sp.first);
    (void)hipEventDestroy(sp.second);
  }
  if (h->stream) (void)hipStreamDestroy(h->stream);
  delete h;
  return PGF_OK;
}

// new derivatives: what was computed from the matrices in HBM goes (their norms, the Gram matrix)
static void invalidate_derivs(pgf_handle h) {
  h->norms_valid = false;
  h->gram_valid = false;
  h->cond_since_upload = 0;
}

int pgf_set_bounds(pgf_handle h, const double *lb, const double *ub) {
  if (!h) return PGF_INVALID;
  if (h->n && (!lb || !ub)) return fail(h, PGF_INVALID, "null bounds");
  (void)hipSetDevice(h->device);
  int rc;
  if ((rc = up(h, h->lb, lb, h->n * sizeof(double)))) return rc;
  if ((rc = up(h, h->ub, ub, h->n * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->bounds_set = true;
  if (h->outer_set) launch_scale_bounds(h->stream, h->n, h->lamb, h->lb, h->ub, h->slb, h->sub);
  return PGF_OK;
}

int pgf_set_outer(pgf_handle h, const double *xhat, const double *yhat, double dt, double rho) {
  if (!h) return PGF_INVALID;
  if (!(dt > 0.0) || !(rho > 0.0)) return fail(h, PGF_INVALID, "dt and rho must be positive");
  if (!h->bounds_set) return fail(h, PGF_NOT_READY, "pgf_set_bounds first");
  if ((h->n && !xhat) || (h->m && !yhat)) return fail(h, PGF_INVALID, "null outer iterate");
  (void)hipSetDevice(h->device);
  int rc;
  if ((rc = up(h, h->xhat, xhat, h->n * sizeof(double)))) return rc;
  if ((rc = up(h, h->yhat, yhat, h->m * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->dt = dt;
  h->lamb = 1.0 / dt;
  h->rho = rho;
  h->fact = 1.0 / (1.0 + h->lamb * rho);
  h->delta = h->lamb / (1.0 + h->lamb * rho);
  launch_scale_bounds(h->stream, h->n, h->lamb, h->lb, h->ub, h->slb, h->sub);
  h->outer_set = true;
  h->mask_set = false;
  invalidate_factor(h);
  return PGF_OK;
}

static int set_matrix(pgf_handle h, const double *src, int64_t ld, int rows, int cols, int loc,
                      double **own, double **cur, int64_t *curld, bool *owned) {
  if (rows == 0 || cols == 0) {
    *cur = nullptr;
    *curld = cols;
    return PGF_OK;
  }
  if (!src || ld < cols) return fail(h, PGF_INVALID, "bad matrix pointer / leading dimension");
  if (loc == PGF_DEVICE) {
    *cur = const_cast<double *>(src);
    *curld = ld;
    *owned = false;
    return PGF_OK;
  }
  if (!*own) HIPCHK(h, dalloc(own, (size_t)rows * cols));
  HIPCHK(h, hipMemcpy2DAsync(*own, (size_t)cols * sizeof(double), src, (size_t)ld * sizeof(double),
                             (size_t)cols * sizeof(double), rows, hipMemcpyHostToDevice,
                             h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *cur = *own;
  *curld = cols;
  *owned = true;
  return PGF_OK;
}

int pgf_set_derivs_dense(pgf_handle h, const double *H, int64_t ldh, const double *J, int64_t ldj,
                         int loc) {
  if (!h) return PGF_INVALID;
  (void)hipSetDevice(h->device);
  int rc;
  if ((rc = set_matrix(h, H, ldh, h->n, h->n, loc, &h->Hown, &h->H, &h->ldh, &h->ownH))) return rc;
  if ((rc = set_matrix(h, J, ldj, h->m, h->n, loc, &h->Jown, &h->J, &h->ldj, &h->ownJ))) return rc;
  h->derivs_set = true;
  h->h_has_lag_only = false;
  invalidate_derivs(h);
  invalidate_factor(h);
  return PGF_OK;
}

// one CSR matrix (host arrays) -> the library-owned dense buffer *own (rows x cols)
static int csr_matrix_to_dense(pgf_handle h, int rows, int cols, const int *ptr, const int *idx,
                               const double *val, double **own, double **cur, int64_t *curld,
                               bool *owned) {
  if (rows == 0 || cols == 0) {
    *cur = nullptr;
    *curld = cols;
    return PGF_OK;
  }
  if (!ptr) return fail(h, PGF_INVALID, "null CSR row pointer");
  const int nnz = ptr[rows];
  if (ptr[0] != 0 || nnz < 0 || (nnz && (!idx || !val)))
    return fail(h, PGF_INVALID, "bad CSR arrays");
  for (int r = 0; r < rows; ++r)
    if (ptr[r + 1] < ptr[r]) return fail(h, PGF_INVALID, "CSR row pointers must be non-decreasing");
  for (int p = 0; p < nnz; ++p)
    if (idx[p] < 0 || idx[p] >= cols) return fail(h, PGF_INVALID, "CSR column index out of range");
  if ((size_t)rows + 1 > h->csr_ptr_cap) {
    if (h->csr_ptr) (void)hipFree(h->csr_ptr);
    h->csr_ptr = nullptr;
    HIPCHK(h, dalloc(&h->csr_ptr, (size_t)rows + 1));
    h->csr_ptr_cap = (size_t)rows + 1;
  }
  if ((size_t)nnz > h->csr_nnz_cap) {
    if (h->csr_idx) (void)hipFree(h->csr_idx);
    if (h->csr_val) (void)hipFree(h->csr_val);
    h->csr_idx = nullptr;
    h->csr_val = nullptr;
    const size_t cap = (size_t)nnz + (size_t)nnz / 4 + 16;
    HIPCHK(h, dalloc(&h->csr_idx, cap));
    HIPCHK(h, dalloc(&h->csr_val, cap));
    h->csr_nnz_cap = cap;
  }
  if (!*own) HIPCHK(h, dalloc(own, (size_t)rows * cols));
  int rc;
  if ((rc = up(h, h->csr_ptr, ptr, ((size_t)rows + 1) * sizeof(int)))) return rc;
  if (nnz) {
    if ((rc = up(h, h->csr_idx, idx, (size_t)nnz * sizeof(int)))) return rc;
    if ((rc = up(h, h->csr_val, val, (size_t)nnz * sizeof(double)))) return rc;
  }
  HIPCHK(h, hipMemsetAsync(*own, 0, (size_t)rows * cols * sizeof(double), h->stream));
  launch_csr_to_dense(h->stream, rows, h->csr_ptr, h->csr_idx, h->csr_val, *own, cols);
  // the staging arrays are reused by the next matrix: finish before returning
  HIPCHK(h, hipStreamSynchronize(h->stream));
  *cur = *own;
  *curld = cols;
  *owned = true;
  return PGF_OK;
}

int pgf_set_derivs_csr(pgf_handle h, const int *Hptr, const int *Hidx, const double *Hval,
                       const int *Jptr, const int *Jidx, const double *Jval) {
  if (!h) return PGF_INVALID;
  if (h->sparse) return fail(h, PGF_INVALID, "banded handles take pgf_sparse_set_pattern / _values");
  (void)hipSetDevice(h->device);
  int rc;
  if ((rc = csr_matrix_to_dense(h, h->n, h->n, Hptr, Hidx, Hval, &h->Hown, &h->H, &h->ldh,
                                &h->ownH)))
    return rc;
  if ((rc = csr_matrix_to_dense(h, h->m, h->n, Jptr, Jidx, Jval, &h->Jown, &h->J, &h->ldj,
                                &h->ownJ)))
    return rc;
  h->derivs_set = true;
  h->h_has_lag_only = false;
  invalidate_derivs(h);
  invalidate_factor(h);
  return PGF_OK;
}

void tau_factors(pgf_handle h, double tau, int *use_tau, double *f_x, double *f_x0,
                        double *f_d) {
  // implicit_func.py:237-244
  *use_tau = std::isnan(tau) ? 0 : 1;
  const double lamb = 1.0 / h->dt;
  *f_x = *use_tau ? lamb * (1 - tau * lamb) : 0.0;
  *f_x0 = *use_tau ? tau * lamb * lamb : 0.0;
  *f_d = *use_tau ? tau * lamb : 0.0;
}

int pgf_active_set(pgf_handle h, const double *x, const double *g, double tau, uint8_t *mask_out) {
  if (!h) return PGF_INVALID;
  if (!h->outer_set) return fail(h, PGF_NOT_READY, "pgf_set_outer first");
  if (h->n && (!x || !g || !mask_out)) return fail(h, PGF_INVALID, "null argument");
  (void)hipSetDevice(h->device);
  int rc;
  if ((rc = up(h, h->tmpn, x, h->n * sizeof(double)))) return rc;
  if ((rc = up(h, h->g, g, h->n * sizeof(double)))) return rc;
  int use_tau;
  double f_x, f_x0, f_d;
  tau_factors(h, tau, &use_tau, &f_x, &f_x0, &f_d);
  if (h->form == PGF_FORM_STANDARD)  // the unscaled projection and thresholds
    launch_unscaled_active_set(h->stream, h->n, use_tau, h->dt, use_tau ? 1.0 - tau * h->lamb : 0.0,
                               use_tau ? tau * h->lamb : 0.0, use_tau ? tau : 0.0, h->xhat, h->tmpn, h->g,
                               h->lb, h->ub, h->mask_new);
  else
    launch_active_set(h->stream, h->n, use_tau, h->lamb, f_x, f_x0, f_d, h->xhat, h->tmpn, h->g,
                      h->slb, h->sub, h->mask_new);
  if ((rc = down(h, mask_out, h->mask_new, h->n))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->eval_fresh = false;
  return PGF_OK;
}

// PGF_STEP_SPEC=0: a step waits for the sizes of its index sets (one more host synchronisation
// per step) instead of running with the last known ones
static bool step_spec() { static const bool on = env_on("PGF_STEP_SPEC"); return on; }

// After the compaction of h->mask into index lists + counts (enqueued by the caller with
// expect = h->nI when `spec', else -1).  spec: a step is being enqueued and will run with the last
// known |I|, |A| -- no host synchronisation here; pgf_qp_sync reads the true counts and the
// mismatch word with the step's status block and redoes the step if they differ.  Otherwise the
// counts are awaited (one host sync).
static int adopt_index_sets(pgf_handle h, bool spec) {
  h->mask_set = true;
  invalidate_factor(h);
  if (spec) {
    h->spec_pending = true;
    return PGF_OK;
  }
  int rc;
  if ((rc = down(h, h->h_counts, h->counts, 2 * sizeof(int)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  ++h->stat_host_syncs;
  adopt_counts(h);
  return PGF_OK;
}
static int refresh_index_sets(pgf_handle h, bool in_step) {
  const bool spec = in_step && h->counts_known && step_spec();
  launch_compact(h->stream, h->n, h->mask, h->idxI, h->idxA, h->pos, h->counts, spec ? h->nI : -1);
  return adopt_index_sets(h, spec);
}

int pgf_set_active_set(pgf_handle h, const uint8_t *mask) {
  if (!h) return PGF_INVALID;
  if (h->n && !mask) return fail(h, PGF_INVALID, "null mask");
  (void)hipSetDevice(h->device);
  int rc;
  if (h->sparse) {
    if ((rc = up(h, h->mask, mask, h->n))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
  } else if (h->n) {
    // through a pinned stage (the caller's buffer may go as soon as this returns); the stage is
    // reused once the previous upload from it has run
    if (!h->h_mask_stage) {
      HIPCHK(h, hipHostMalloc((void **)&h->h_mask_stage, (size_t)h->n));
      HIPCHK(h, hipEventCreateWithFlags(&h->mask_ev, hipEventDisableTiming));
    } else {
      HIPCHK(h, hipEventSynchronize(h->mask_ev));
    }
    memcpy(h->h_mask_stage, mask, (size_t)h->n);
    if ((rc = up(h, h->mask, h->h_mask_stage, h->n))) return rc;
    HIPCHK(h, hipEventRecord(h->mask_ev, h->stream));
  }
  // the sizes are counted here: no wait for the device's counts
  int na = 0;
  for (int i = 0; i < h->n; ++i) na += mask[i] ? 1 : 0;
  h->nA = na;
  h->nI = h->n - na;
  h->N = h->nI + h->m;
  h->counts_known = true;
  h->mask_set = true;
  invalidate_factor(h);
  if (!h->sparse)
    launch_compact(h->stream, h->n, h->mask, h->idxI, h->idxA, h->pos, h->counts, h->nI);
  return PGF_OK;
}

int pgf_reduced_dims(pgf_handle h, int *n_inactive, int *n_reduced) {
  if (!h) return PGF_INVALID;
  if (!h->mask_set) return fail(h, PGF_NOT_READY, "no active set");
  if (n_inactive) *n_inactive = h->nI;
  if (n_reduced) *n_reduced = h->form ? h->n + h->m : h->N;
  return PGF_OK;
}

int check_ready(pgf_handle h) {
  if (!h->outer_set) return fail(h, PGF_NOT_READY, "pgf_set_outer first");
  if (h->sparse ? !h->sp.values_set : !h->derivs_set)
    return fail(h, PGF_NOT_READY, "pgf_set_derivs_* / pgf_sparse_set_values first");
  if (!h->mask_set) return fail(h, PGF_NOT_READY, "pgf_set_active_set first");
  return PGF_OK;
}

static void assemble(pgf_handle h, double *K, int64_t ldk) {
  launch_assemble_kkt(h->stream, K, ldk, h->H, h->ldh, h->J, h->ldj, h->idxI, h->nI, h->m, h->lamb,
                      h->delta);
}

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
  const double nH = h->h_rs[4] + h->lamb;
  const double g = h->h_rs[6] * h->h_rs[5] / (h->delta * nH);
  const double nK = std::max(nH + h->h_rs[6], h->h_rs[5] + h->delta);
  return g <= gmax && 1.1e-16 * g * nK <= emax * std::min(h->lamb, h->delta);
}
static bool condensed_wanted(pgf_handle h) {
  const int mode = condensed_mode();
  if (!mode || h->condensed_veto || h->m == 0 || h->nI == 0 || h->m > h->n) return false;
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
// true: h->G holds J^T J for the matrices in HBM (built now if the rule says so); false: this
// factorisation takes the virtual-block path.  Never an error: a failed allocation switches the
// Gram path off for the handle.  (condensed_reserve has been called: f.V, f.vd hold n + 1 rows.)
static bool gram_prepare(pgf_handle h) {
  const int mode = gram_mode();
  if (!mode || h->gram_off) return false;
  if (h->gram_valid) return true;
  if (mode == 1 && h->cond_since_upload < 1) return false;
  return gram_build(h);
}
// the build itself (also asked for by the device-resident Standard formulation, unsym_gram)
bool gram_build(pgf_handle h) {
  DenseLdlt &f = h->fac;
  const int n = h->n, mp = round_up32(h->m);
  if (!h->G) {
    int64_t ld = ((int64_t)n + 15) / 16 * 16;  // (as pick_ldk: row starts off one HBM channel)
    if (ld % 512 == 0) ld += 16;
    std::vector<int> ident((size_t)n + 1, 0);
    for (int i = 0; i < n; ++i) ident[i] = i;
    if (hipMalloc((void **)&h->G, (size_t)n * ld * sizeof(double)) != hipSuccess ||
        hipMalloc((void **)&h->gram_aux, ((size_t)n + 1) * sizeof(int)) != hipSuccess ||
        hipMemcpy(h->gram_aux, ident.data(), ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
      (void)hipGetLastError();
      if (h->G) (void)hipFree(h->G);
      if (h->gram_aux) (void)hipFree(h->gram_aux);
      h->G = nullptr;
      h->gram_aux = nullptr;
      h->gram_off = true;
      return false;
    }
    h->ldg = ld;
  }
  // V <- J^T (all columns), vd <- -1 (delta = 1); both are rewritten for this step right after
  launch_cond_panel(h->stream, f.V, condensed_ldv(h->m), mp, f.vd, h->J, h->ldj, h->gram_aux, n, h->m, 1.0,
                    nullptr);
  if (ldlt_gram_async(h->stream, h->G, h->ldg, n, f.V, condensed_ldv(h->m), f.vd, mp, h->gram_aux + n) !=
      hipSuccess) {
    (void)hipGetLastError();
    h->gram_off = true;
    return false;
  }
  h->gram_valid = true;
  ++h->stat_gram_builds;
  return true;
}
// the factorisation that was counted last is discarded and will be enqueued again
static void gram_uncount(pgf_handle h) {
  if (h->fac_counted) --h->cond_since_upload;
  if (h->fac_used_gram) --h->stat_gram_factors;
  if (h->fac_head == 1) --h->stat_head_fused;
  if (h->fac_head == 2) --h->stat_head_plain;
  h->fac_counted = h->fac_used_gram = false;
  h->fac_head = 0;
}

// sol <- K^{-1} rhs with the current LDL^T factor (rhs, sol: N-vectors in the order
// [inactive variables; constraints]; rhs != sol)
static hipError_t kkt_solve_async(pgf_handle h, const double *rhs, double *sol) {
  if (!h->condensed) return ldlt_solve_async(h->fac, rhs, sol);
  DenseLdlt &f = h->fac;
  launch_cond_rhs(h->stream, h->nI, h->m, f.V, f.ldv, rhs, h->delta, h->cd_t);
  hipError_t e = ldlt_solve_async(f, h->cd_t, sol);
  if (e != hipSuccess) return e;
  launch_cond_y(h->stream, h->nI, h->m, f.V, f.ldv, sol, rhs + h->nI, h->delta, h->partial,
                (size_t)PGF_GEMVT_PARTS * (h->n ? h->n : 1), sol + h->nI);
  return hipGetLastError();
}
// the backward half for the right-hand side h->rhs that rode through the factorisation
// (cy: a condensed step leaves s_y to the step update that follows directly -- only the partial
// products are enqueued here, *cy describes them)
static hipError_t kkt_backsolve_async(pgf_handle h, double *sol, StepCondY *cy = nullptr) {
  DenseLdlt &f = h->fac;
  if (cy) cy->partial = nullptr;
  if (!h->condensed) return ldlt_backsolve_async(f, f.K + (int64_t)h->N * f.ldk, sol);
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
  ++(fused ? h->stat_head_fused : h->stat_head_plain);
  h->fac_head = fused ? 1 : 2;
}

// enqueue assemble + factor; with_rhs: carry h->rhs through the elimination in the row behind the
// matrix.  Where ldlt_head_wanted, the assembly is not launched here but described in hw.
static int factor_async(pgf_handle h, bool with_rhs) {
  if (h->sparse) return band_factor_async(h);
  DenseLdlt &f = h->fac;
  h->lu_active = false;
  h->condensed = condensed_wanted(h);
  f.vdepth = 0;
  f.vneg = 0;
  h->fac_counted = h->fac_used_gram = false;
  h->fac_head = 0;
  const int nI = h->nI, Nf = h->condensed ? nI : h->N;  // pivots of this factorisation
  double *row = f.K + (int64_t)Nf * f.ldk;               // the row behind them: the right-hand side's
  const double *row_src = with_rhs ? h->rhs : nullptr;
  LdltHead hw;
  bool head;
  if (h->condensed) {
    HIPCHK(h, condensed_reserve(h));
    const int mp = round_up32(h->m);
    f.ldv = condensed_ldv(h->m);
    f.vneg = h->m;  // the eliminated block is -delta I
    const bool gram = gram_prepare(h);
    ++h->cond_since_upload;
    h->fac_counted = true;
    h->fac_used_gram = gram;
    if (gram)
      ++h->stat_gram_factors;
    else
      f.vdepth = mp;  // the rank-m term as virtual blocks
    const double *rhs_y = with_rhs ? h->rhs + nI : nullptr;
    head = gram && ldlt_head_wanted(f, nI);
    if (head) {
      // Gram, all of it beside the first diagonal chain, which reads the first 256 rows only
      hw = head_assembly(h, nI, 0);
      hw.G = h->G;
      hw.ldg = h->ldg;
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
                            f.flags, 4 + LDLT_UPD_COUNTERS, nullptr, nullptr, 0, h->G, h->ldg);
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

// internal: the factorisation just awaited must be repeated (its chain helpers failed their
// hand-over checks and are switched off now, ldlt_finish -- or the condensed pivot order met a
// zero pivot the natural order may not have: S = A + J^T J / delta can cancel exactly where no
// pivot of K does); never leaves the library
#define PGF_RETRY_FACTOR (-2)
static int finish_factor_state(pgf_handle h, hipError_t *e) {
  const int st = ldlt_finish(h->fac, e);
  if (h->sparse && st >= 0) band_kept_resolve(h);
  if (st == 1 && h->condensed && !h->condensed_veto) {
    h->condensed_veto = true;
    h->fac.factored = false;
    gram_uncount(h);
    return 2;
  }
  if (st == 2) gram_uncount(h);
  return st;
}
static const char *k_helper_msg =
    "the dense factorisation failed its hand-over checks with and without helper workgroups";

static int factor_finish(pgf_handle h) {
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
static int factor_sync(pgf_handle h) {
  int rc;
  for (int attempt = 0; attempt < 2; ++attempt) {
    if ((rc = factor_async(h, false))) return rc;
    if ((rc = factor_finish(h)) != PGF_RETRY_FACTOR) return rc;
  }
  return fail(h, PGF_HIP_ERROR, k_helper_msg);
}

// (expand: also the residual check's expansion of the solution into rs_v, rs_lv and the zeroing of
// its maxima, launch_residual_and_eval(..., prepared = true))
void enqueue_step_update(pgf_handle h, bool expand, const StepCondY *cy) {
  DenseLdlt &f = h->fac;
  const int bits = f.status_words;  // deferred status words go to the status block
  f.status_words = 0;
  h->stat_bits |= bits;
  launch_step_update(h->stream, h->n, h->m, h->nI, h->fact, h->rho, h->x, h->y, h->lb, h->ub,
                     h->mask, h->pos, h->b0full, h->F, h->sol, h->dx, h->dy, h->xn, h->yn, h->red,
                     h->scal, h->ticket, h->lamb, expand ? h->rs_v : nullptr, expand ? h->rs_lv : nullptr,
                     expand ? h->rs_red : nullptr, (bits & 1) ? f.flags : nullptr,
                     (bits & 2) ? f.chain + 2 * f.chain_stride + 1 : nullptr,
                     reinterpret_cast<int *>(h->stat + 14), cy && cy->partial ? cy : nullptr);
}
// after the host synchronisation of a step with deferred status words: to DenseLdlt::h_flags,
// in the order the two separate copies would have left them
static void absorb_status(pgf_handle h) {
  const int *w = reinterpret_cast<const int *>(h->h_stat + 14);
  if (h->stat_bits & 1)
    for (int k = 0; k < 4; ++k) h->fac.h_flags[k] = w[k];
  else if (h->stat_bits & 2)
    h->fac.h_flags[3] = w[3];
  h->stat_bits = 0;
}

// r = rhs - K s of the solve just enqueued, with K applied from H, J and the mask (the factor
// overwrote the assembled matrix); the three maxima reach the host with the next sync
void enqueue_residual(pgf_handle h, bool may_skip) {
  if (!h->refine_mode) return;
  h->rs_skipped = may_skip && h->factor_clean;
  if (h->rs_skipped) return;
  launch_kkt_residual(h->stream, h->n, h->m, h->nI, h->lamb, h->delta, h->H, h->ldh, h->J, h->ldj,
                      h->idxI, h->pos, h->mask, h->rhs, h->sol, h->rs_v, h->rs_lv, h->rs_u, h->rs_wy,
                      h->partial, PGF_GEMVT_PARTS, h->rs_r, h->rs_red);
  (void)hipMemcpyAsync(h->h_rs, h->rs_red, 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream);
}

// The measure of a solve: max |rhs - K s| against max |rhs| -- and, once the matrices' norms are
// known (residual_norms), against ||K|| max |s| + max |rhs|: the normwise backward error.  A
// backward-stable solve only guarantees |r| <~ eps ||K|| ||s||, which is eps cond(K) ||rhs||: at
// cond(K) ~ 1e5 and beyond the first form alone would send good solves into refinement, and at
// ~1e9 not even the pivoted LU could meet it -- the reference's splu accepts those solves
// (lu_solver.py:14-21).  ||K||_inf <= max(||H||_inf + lambda + ||J||_1, ||J||_inf + delta): the
// reduced matrix is a principal submatrix of that one.
static double residual_rel(pgf_handle h) {
  const double r = h->h_rs[0], b = h->h_rs[1], sn = h->h_rs[2];
  if (!(r == r) || !(r <= 1.79e308)) return HUGE_VAL;
  double den = b;
  if (h->norms_valid) {
    const double nK = std::max(h->h_rs[4] + h->lamb + h->h_rs[6], h->h_rs[5] + h->delta);
    if (sn == sn && sn <= 1.79e308) den += nK * sn;
  }
  return r / (den > 0.0 ? den : 1.0);
}
// the norms of H and J in HBM (one pass over both, one synchronisation; cached until the next
// pgf_set_derivs_*)
int residual_norms(pgf_handle h) {
  if (h->norms_valid) return PGF_OK;
  launch_matrix_norms(h->stream, h->n, h->m, h->H, h->ldh, h->J, h->ldj, h->rs_red + 4);
  HIPCHK(h, hipMemcpyAsync(h->h_rs + 4, h->rs_red + 4, 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->norms_valid = true;
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
  if (!h->refine_mode || h->N == 0 || h->rs_skipped) return PGF_OK;
  double rel = residual_rel(h);
  int rc;
  if (rel > h->refine_tol && !h->norms_valid) {
    // missed against max |rhs| alone: take the size of K and of the solution into account
    if ((rc = residual_norms(h))) return rc;
    rel = residual_rel(h);
  }
  h->stat_last_rel = rel;
  if (h->last_solve == 1) h->factor_clean = rel <= 1e-3 * h->refine_tol;
  if (rel <= h->refine_tol) return PGF_OK;
  hipStream_t s = h->stream;
  auto unswap = [&]() { if (swapped) swap_point(h); };
  auto finish_round = [&]() -> int {
    enqueue_residual(h);
    h->eval_fresh = false;  // the point moves: what pgf_qp_step_async evaluated ahead is stale
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
  for (int it = 0; it < 2 && rel > h->refine_tol && rel < 1.0 && !h->lu_active; ++it) {
    HIPCHK(h, kkt_solve_async(h, h->rs_r, h->rs_d));
    launch_axpy1(s, h->N, h->rs_d, h->sol);
    if ((rc = finish_round())) return rc;
    ++h->stat_refined;
    const double now = residual_rel(h);
    if (!(now < rel)) {  // not contracting: leave it to the pivoted factorisation
      rel = now;
      break;
    }
    rel = now;
  }
  h->stat_last_rel = rel;
  if (rel <= h->refine_fail) return PGF_OK;
  // pivoted LU of the reduced matrix
  if (!h->lu_active) {
    if (!h->lu.A || h->lu.N != h->N) {
      lu_free(h->lu);
      HIPCHK(h, lu_alloc(h->lu, h->N, s));
    }
    HIPCHK(h, hipMemsetAsync(h->lu.A, 0, (size_t)h->lu.N * h->lu.ld * sizeof(double), s));
    assemble(h, h->lu.A, h->lu.ld);
    launch_symmetrize(s, h->lu.A, h->lu.ld, h->N);
    hipError_t e;
    const int st = lu_factor(h->lu, &e);
    if (st < 0) return hip_fail(h, e, "LU fallback");
    if (st == 1) return fail(h, PGF_SINGULAR, "reduced KKT matrix is singular (LDL^T unstable, LU failed)");
    h->lu_active = true;
    ++h->stat_lu;
  }
  HIPCHK(h, lu_solve_async(h->lu, h->rhs, h->sol, 0));
  if ((rc = finish_round())) return rc;
  rel = residual_rel(h);
  h->stat_last_rel = rel;
  if (!(rel <= h->refine_fail))
    return fail(h, PGF_SINGULAR, "reduced KKT system could not be solved to a small residual");
  return PGF_OK;
}

// After a host synchronisation: a chained triangular solve that failed its own checks
// (placement, timeout) has left garbage in h->sol and whatever was derived from it.  The
// chain is off from now on (ldlt_chain_check); the solve and the step update are enqueued
// again with the per-super-block kernels and awaited, so that the caller never sees the
// failure.  swapped: the caller has already exchanged (x, y) with (xn, yn) (pgf_qp_step_async).
static int chain_recover(pgf_handle h, bool swapped) {
  if (!ldlt_chain_check(h->fac)) return PGF_OK;  // (0 on a banded handle: it has no chain)
  h->eval_fresh = false;  // the point is computed again
  if (swapped) swap_point(h);
  if (h->last_solve == 1)
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

int pgf_factor(pgf_handle h, int *n_neg) {
  if (!h) return PGF_INVALID;
  int rc;
  if ((rc = check_ready(h))) return rc;
  (void)hipSetDevice(h->device);
  if (h->form) {
    if (!h->ulu_ok && (rc = unsym_factor(h))) return rc;  // (the factor of the current matrix stays)
    if (n_neg) *n_neg = -1;
    return PGF_OK;
  }
  if ((rc = factor_sync(h))) return rc;
  if (n_neg) *n_neg = h->fac.n_neg;
  return PGF_OK;
}

// residual + reduced rhs for the point in (h->x, h->y, h->g, h->c), then solve and update.
// Everything is enqueued; returns without syncing.  factored_out tells whether a factor
// was enqueued (its flags then need checking at the sync).
static int newton_core_async(pgf_handle h, bool *did_factor) {
  hipStream_t s = h->stream;
  h->fused_eval_done = false;
  h->fac_counted = h->fac_used_gram = false;  // (set by factor_async, if this step factorises)
  h->fac_head = 0;
  if (h->sparse) return band_step_async(h, did_factor);
  const bool front_done = h->front_done;
  h->front_done = false;
  if (front_done) {
    // (qp_refresh_mask: F, b0full and rhs came with the compaction's launch)
  } else if (h->nA == 0) {  // the residual and the reduced right-hand side in one launch
    launch_residual_rhs(s, h->n, h->m, h->nI, h->lamb, h->dt, h->fact, h->xhat, h->yhat, h->x, h->y, h->g,
                        h->c, h->slb, h->sub, h->mask, h->idxI, h->F, h->b0full, h->rhs);
  } else {
    launch_residual(s, h->n, h->m, h->lamb, h->dt, h->xhat, h->yhat, h->x, h->y, h->g, h->c, h->slb,
                    h->sub, h->mask, h->F, h->b0full);
    launch_reduced_rhs(s, h->n, h->m, h->nI, h->nA, h->fact, h->F, h->idxI, h->idxA, h->H, h->ldh, h->J,
                       h->ldj, h->b0full, h->partial, PGF_GEMVT_PARTS, h->rhs);
  }
  *did_factor = false;
  h->rs_skipped = h->fac.factored && h->factor_clean;  // (a step that factorises is always checked)
  // the tail of a qp step in fewer launches (same values): s_y in the step update, the row passes
  // over J and H in one launch, the sums, the H pass's epilogue and the residual in another
  const bool ahead = eval_ahead() && h->qp_mode && h->refine_mode && !h->rs_skipped;
  const bool fused_tail = ahead && step_fused();
  StepCondY cy{nullptr, nullptr, nullptr, 0.0, 0};
  if (!h->fac.factored) {
    int rc;
    if ((rc = factor_async(h, true))) return rc;
    *did_factor = true;
    h->last_solve = 1;
    h->lu_active = false;
    HIPCHK(h, kkt_backsolve_async(h, h->sol, fused_tail ? &cy : nullptr));
  } else {
    h->last_solve = 2;
    if (h->lu_active)
      HIPCHK(h, lu_solve_async(h->lu, h->rhs, h->sol, 0));
    else
      HIPCHK(h, kkt_solve_async(h, h->rhs, h->sol));
  }
  // Device-resident mode: the residual check of this solve and g, c at the point the step update
  // produces read the same matrices -- one pass over H and two over J for both
  // (launch_residual_and_eval) instead of two and four.  (PGF_EVAL_AHEAD=0: separately, the
  // evaluation at the start of the next step.)
  h->fused_eval_done = false;
  if (ahead) {
    enqueue_step_update(h, /*expand=*/true, &cy);
    ++(fused_tail ? h->stat_tail_fused : h->stat_tail_plain);
    if (fused_tail)
      launch_residual_and_eval_fused(s, h->n, h->m, h->nI, h->delta, h->H, h->ldh, h->J, h->ldj, h->pos, h->mask,
                                     h->rhs, h->sol, h->rs_v, h->rs_lv, h->rs_u, h->rs_wy, h->partial,
                                     PGF_GEMVT_PARTS, h->rs_r, h->rs_red, h->xn, h->yn, h->b, h->q, h->rho, h->c,
                                     h->w, h->tmpn, h->g);
    else
      launch_residual_and_eval(s, h->n, h->m, h->nI, h->lamb, h->delta, h->H, h->ldh, h->J, h->ldj, h->idxI,
                               h->pos, h->mask, h->rhs, h->sol, h->rs_v, h->rs_lv, h->rs_u, h->rs_wy, h->partial,
                               PGF_GEMVT_PARTS, h->rs_r, h->rs_red, h->xn, h->yn, h->b, h->q, h->rho, h->c, h->w,
                               h->tmpn, h->g, /*prepared=*/true);
    // (a qp step reads the maxima with its whole status block)
    if (!h->fac.defer_status)
      (void)hipMemcpyAsync(h->h_rs, h->rs_red, 3 * sizeof(double), hipMemcpyDeviceToHost, s);
    h->fused_eval_done = true;
    return PGF_OK;
  }
  enqueue_residual(h, !*did_factor);
  enqueue_step_update(h);
  return PGF_OK;
}

int pgf_newton_solve(pgf_handle h, const double *x, const double *y, const double *g,
                     const double *c, int inertia_check, double *dx, double *dy, double *xn,
                     double *yn, double *diff) {
  if (!h) return PGF_INVALID;
  int rc;
  if ((rc = check_ready(h))) return rc;
  if ((h->n && (!x || !g)) || (h->m && (!y || !c))) return fail(h, PGF_INVALID, "null argument");
  (void)hipSetDevice(h->device);
  if ((rc = up(h, h->x, x, h->n * sizeof(double)))) return rc;
  if ((rc = up(h, h->y, y, h->m * sizeof(double)))) return rc;
  if ((rc = up(h, h->g, g, h->n * sizeof(double)))) return rc;
  if ((rc = up(h, h->c, c, h->m * sizeof(double)))) return rc;
  h->eval_fresh = false;
  if (h->form) {
    if (inertia_check) return fail(h, PGF_INVALID, "no inertia with an unsymmetric formulation (LU)");
    if ((rc = unsym_step_core(h))) return rc;
    if ((rc = down(h, h->h_scal, h->scal, sizeof(double)))) return rc;
    if (dx && (rc = down(h, dx, h->dx, h->n * sizeof(double)))) return rc;
    if (dy && (rc = down(h, dy, h->dy, h->m * sizeof(double)))) return rc;
    if (xn && (rc = down(h, xn, h->xn, h->n * sizeof(double)))) return rc;
    if (yn && (rc = down(h, yn, h->yn, h->m * sizeof(double)))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (diff) *diff = h->h_scal[0];
    return PGF_OK;
  }
  bool did_factor;
  for (int attempt = 0;; ++attempt) {
    if ((rc = newton_core_async(h, &did_factor))) return rc;
    // (a banded step has enqueued the copy of its own status: band_step_async)
    if (!h->sparse && (rc = down(h, h->h_scal, h->scal, sizeof(double)))) return rc;
    if (did_factor) {
      rc = factor_finish(h);
      if (rc == PGF_RETRY_FACTOR) {  // once more, without the chain's helper workgroups
        if (attempt == 0) continue;
        return fail(h, PGF_HIP_ERROR, k_helper_msg);
      }
      if (rc) return rc;
    } else {
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    break;
  }
  if ((rc = chain_recover(h, false))) return rc;
  if ((rc = refine_if_needed(h, false))) return rc;
  if (inertia_check && h->fac.n_neg != h->m) return fail(h, PGF_INERTIA, "Invalid matrix inertia");
  if (dx && (rc = down(h, dx, h->dx, h->n * sizeof(double)))) return rc;
  if (dy && (rc = down(h, dy, h->dy, h->m * sizeof(double)))) return rc;
  if (xn && (rc = down(h, xn, h->xn, h->n * sizeof(double)))) return rc;
  if (yn && (rc = down(h, yn, h->yn, h->m * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (diff) *diff = h->h_scal[0];
  return PGF_OK;
}

int pgf_residual(pgf_handle h, const double *x, const double *y, const double *g, const double *c,
                 const uint8_t *mask, double *F_out) {
  if (!h) return PGF_INVALID;
  if (!h->outer_set) return fail(h, PGF_NOT_READY, "pgf_set_outer first");
  if ((h->n && (!x || !g)) || (h->m && (!y || !c)) || !F_out)
    return fail(h, PGF_INVALID, "null argument");
  (void)hipSetDevice(h->device);
  int rc;
  // scratch: xn / yn / tmpn / w hold the point so the solver state is untouched
  if ((rc = up(h, h->xn, x, h->n * sizeof(double)))) return rc;
  if ((rc = up(h, h->yn, y, h->m * sizeof(double)))) return rc;
  if ((rc = up(h, h->tmpn, g, h->n * sizeof(double)))) return rc;
  if ((rc = up(h, h->w, c, h->m * sizeof(double)))) return rc;
  if (mask) {
    if ((rc = up(h, h->mask_new, mask, h->n))) return rc;
  } else if (h->form == PGF_FORM_STANDARD) {
    unsym_mask(h, NAN, h->xn, h->tmpn, h->mask_new);
  } else {
    launch_active_set(h->stream, h->n, 0, h->lamb, 0, 0, 0, h->xhat, h->xn, h->tmpn, h->slb,
                      h->sub, h->mask_new);
  }
  if (h->form == PGF_FORM_STANDARD) {  // the unscaled residual (ImplicitFunc.value_at)
    launch_unsym_residual_rhs(h->stream, h->form, h->n, h->m, h->lamb, h->dt, h->fact, h->xhat, h->yhat,
                              h->xn, h->yn, h->tmpn, h->w, h->lb, h->ub, h->mask_new, nullptr, nullptr,
                              h->sol, nullptr);
  } else {
    launch_residual(h->stream, h->n, h->m, h->lamb, h->dt, h->xhat, h->yhat, h->xn, h->yn, h->tmpn,
                    h->w, h->slb, h->sub, h->mask_new, h->sol, nullptr);
  }
  if ((rc = down(h, F_out, h->sol, (size_t)(h->n + h->m) * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PGF_OK;
}

int pgf_linear_solve(pgf_handle h, const double *rhs, int trans, double *sol) {
  // (the Symmetric path ignores trans: K is symmetric; a formulation honours it)
  if (!h) return PGF_INVALID;
  int rc;
  if ((rc = check_ready(h))) return rc;
  if (h->sparse) return band_linear_solve(h, rhs, sol);
  if (h->form) {  // the full system, A or A^T (cond_estimate.py:82)
    const int Nf = h->n + h->m;
    if (Nf && (!rhs || !sol)) return fail(h, PGF_INVALID, "null argument");
    if (Nf == 0) return PGF_OK;
    (void)hipSetDevice(h->device);
    if (!h->ulu_ok && (rc = unsym_factor(h))) return rc;
    if ((rc = up(h, h->rhs, rhs, (size_t)Nf * sizeof(double)))) return rc;
    HIPCHK(h, lu_solve_async(h->ulu, h->rhs, h->sol, trans));
    if ((rc = down(h, sol, h->sol, (size_t)Nf * sizeof(double)))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PGF_OK;
  }
  if (h->N && (!rhs || !sol)) return fail(h, PGF_INVALID, "null argument");
  (void)hipSetDevice(h->device);
  if (!h->fac.factored) {
    if ((rc = factor_sync(h))) return rc;
  }
  if ((rc = up(h, h->rhs, rhs, h->N * sizeof(double)))) return rc;
  if (h->lu_active) {  // the pivoted factor took over for this matrix (refine_if_needed)
    HIPCHK(h, lu_solve_async(h->lu, h->rhs, h->sol, 0));
    if ((rc = down(h, sol, h->sol, h->N * sizeof(double)))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return PGF_OK;
  }
  HIPCHK(h, kkt_solve_async(h, h->rhs, h->sol));
  enqueue_residual(h);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (ldlt_chain_check(h->fac)) {  // the chain is off now: once more with the per-block kernels
    HIPCHK(h, kkt_solve_async(h, h->rhs, h->sol));
    enqueue_residual(h);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (ldlt_chain_check(h->fac)) return fail(h, PGF_HIP_ERROR, k_chain_msg);
  }
  if ((rc = refine_if_needed(h, false, false))) return rc;
  if ((rc = down(h, sol, h->sol, h->N * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PGF_OK;
}

int pgf_linear_solve_multi(pgf_handle h, const double *rhs, int nrhs, int64_t ld, int trans, double *sol) {
  if (!h) return PGF_INVALID;
  int rc;
  if ((rc = check_ready(h))) return rc;
  if (nrhs < 0) return fail(h, PGF_INVALID, "negative number of right-hand sides");
  if (nrhs == 0) return PGF_OK;
  const int rows = h->sparse || h->form ? h->n + h->m : h->N;
  if (!rhs || !sol) return fail(h, PGF_INVALID, "null argument");
  if (nrhs > 1 && ld < rows) return fail(h, PGF_INVALID, "column stride is smaller than the system");
  // a wide band without a border: panels on the matrix pipes; everything else column by column
  if (band_multi_panel(h)) return band_linear_solve_multi(h, rhs, nrhs, ld, sol);
  for (int j = 0; j < nrhs; ++j)
    if ((rc = pgf_linear_solve(h, rhs + (int64_t)j * ld, trans, sol + (int64_t)j * ld))) return rc;
  return PGF_OK;
}

// out <- K v for the reduced KKT matrix of the current mask, applied from H, J and the mask on
// the device (no N x N copy crosses PCIe): the products of the condition estimate
int pgf_kkt_apply(pgf_handle h, const double *v, double *out) {
  if (!h) return PGF_INVALID;
  int rc;
  if ((rc = check_ready(h))) return rc;
  if (h->sparse) return fail(h, PGF_NOT_READY, "pgf_kkt_apply: dense mode only");
  if (h->N && (!v || !out)) return fail(h, PGF_INVALID, "null argument");
  if (h->N == 0) return PGF_OK;
  (void)hipSetDevice(h->device);
  // r = 0 - K v with the residual kernels: rs_d holds v, rs_r starts as the zero right-hand side
  if ((rc = up(h, h->rs_d, v, (size_t)h->N * sizeof(double)))) return rc;
  HIPCHK(h, hipMemsetAsync(h->rs_r, 0, (size_t)(h->N + 1) * sizeof(double), h->stream));
  launch_kkt_residual(h->stream, h->n, h->m, h->nI, h->lamb, h->delta, h->H, h->ldh, h->J, h->ldj,
                      h->idxI, h->pos, h->mask, h->rs_r, h->rs_d, h->rs_v, h->rs_lv, h->rs_u,
                      h->rs_wy, h->partial, PGF_GEMVT_PARTS, h->rs_r, h->rs_red);
  if ((rc = down(h, out, h->rs_r, (size_t)h->N * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int i = 0; i < h->N; ++i) out[i] = -out[i];
  return PGF_OK;
}

int pgf_get_kkt(pgf_handle h, double *K_out, int64_t ldk_out) {
  if (!h) return PGF_INVALID;
  int rc;
  if ((rc = check_ready(h))) return rc;
  const int N = h->N;
  if (h->sparse) return fail(h, PGF_NOT_READY, "pgf_get_kkt: dense mode only");
  if (N == 0) return PGF_OK;
  if (!K_out || ldk_out < N) return fail(h, PGF_INVALID, "bad output matrix");
  (void)hipSetDevice(h->device);
  double *tmp = nullptr;
  HIPCHK(h, dalloc(&tmp, (size_t)N * N));
  HIPCHK(h, hipMemsetAsync(tmp, 0, (size_t)N * N * sizeof(double), h->stream));
  assemble(h, tmp, N);
  hipError_t e = hipMemcpy2DAsync(K_out, (size_t)ldk_out * sizeof(double), tmp,
                                  (size_t)N * sizeof(double), (size_t)N * sizeof(double), N,
                                  hipMemcpyDeviceToHost, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  (void)hipFree(tmp);
  if (e != hipSuccess) return hip_fail(h, e, "pgf_get_kkt");
  return PGF_OK;
}

int pgf_qp_set_vectors(pgf_handle h, const double *q, const double *b) {
  if (!h) return PGF_INVALID;
  if ((h->n && !q) || (h->m && !b)) return fail(h, PGF_INVALID, "null argument");
  (void)hipSetDevice(h->device);
  int rc;
  if ((rc = up(h, h->q, q, h->n * sizeof(double)))) return rc;
  if ((rc = up(h, h->b, b, h->m * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->qp_mode = true;
  h->h_has_lag_only = true;
  return PGF_OK;
}

// ---------------------------------------------------------------- device-resident LQ mode
int pgf_qp_set_problem(pgf_handle h, const double *Q, int64_t ldq, const double *q,
                       const double *A, int64_t lda, const double *b, int loc) {
  if (!h) return PGF_INVALID;
  if ((h->n && !q) || (h->m && !b)) return fail(h, PGF_INVALID, "null argument");
  int rc;
  if ((rc = pgf_set_derivs_dense(h, Q, ldq, A, lda, loc))) return rc;
  if (loc == PGF_DEVICE) {
    HIPCHK(h, hipMemcpyAsync(h->q, q, h->n * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
    if (h->m)
      HIPCHK(h, hipMemcpyAsync(h->b, b, h->m * sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  } else {
    if ((rc = up(h, h->q, q, h->n * sizeof(double)))) return rc;
    if ((rc = up(h, h->b, b, h->m * sizeof(double)))) return rc;
  }
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->qp_mode = true;
  h->h_has_lag_only = true;
  return PGF_OK;
}

int pgf_qp_set_point(pgf_handle h, const double *x, const double *y) {
  if (!h) return PGF_INVALID;
  if ((h->n && !x) || (h->m && !y)) return fail(h, PGF_INVALID, "null argument");
  (void)hipSetDevice(h->device);
  int rc;
  if ((rc = up(h, h->x, x, h->n * sizeof(double)))) return rc;
  if ((rc = up(h, h->y, y, h->m * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->point_set = true;
  h->eval_fresh = false;
  return PGF_OK;
}

// a read of the point while a speculative step is in flight: the step is settled first (one wait,
// off the production path), so that the point read is never that of a discarded step
static int settle_spec(pgf_handle h, bool *redone);
static int settle_before_read(pgf_handle h) {
  if (!h->step_pending || !h->spec_pending) return PGF_OK;  // (never speculative on a banded handle)
  HIPCHK(h, hipStreamSynchronize(h->stream));
  bool redone;
  return settle_spec(h, &redone);
}

int pgf_qp_get_point(pgf_handle h, double *x, double *y) {
  if (!h) return PGF_INVALID;
  if (!h->point_set) return fail(h, PGF_NOT_READY, "pgf_qp_set_point first");
  (void)hipSetDevice(h->device);
  int rc;
  if ((rc = settle_before_read(h))) return rc;
  if (x && (rc = down(h, x, h->x, h->n * sizeof(double)))) return rc;
  if (y && (rc = down(h, y, h->y, h->m * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PGF_OK;
}

int pgf_qp_get_mask(pgf_handle h, uint8_t *mask) {
  if (!h || !mask) return PGF_INVALID;
  if (!h->mask_set) return fail(h, PGF_NOT_READY, "no active set");
  (void)hipSetDevice(h->device);
  int rc;
  if ((rc = down(h, mask, h->mask, h->n))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PGF_OK;
}

// c = A x - b ; w = rho c + y ; g = Q x + (q + A' w)   at the device point
void qp_eval(pgf_handle h) {
  if (h->eval_fresh) return;
  h->eval_fresh = true;
  if (h->sparse) return band_eval(h);
  hipStream_t s = h->stream;
  launch_gemv_rows(s, h->m, h->n, h->J, h->ldj, h->x, h->b, -1.0, h->c);
  launch_mult_vec(s, h->m, h->rho, h->c, h->y, h->w);
  launch_gemvT(s, h->m, h->n, h->J, h->ldj, h->w, h->q, h->partial, PGF_GEMVT_PARTS, h->tmpn);
  launch_gemv_rows(s, h->n, h->n, h->H, h->ldh, h->x, h->tmpn, 1.0, h->g);
}

static int qp_ready(pgf_handle h) {
  if (!h->qp_mode) return fail(h, PGF_NOT_READY, "pgf_qp_set_problem first");
  if (!h->outer_set) return fail(h, PGF_NOT_READY, "pgf_set_outer first");
  if (!h->point_set) return fail(h, PGF_NOT_READY, "pgf_qp_set_point first");
  return PGF_OK;
}

// mask at the device point -> mask_new; adopt it if it differs (or none yet).  in_step: a step is
// being enqueued (its index-set sizes may be speculative, refresh_index_sets).
static int qp_refresh_mask(pgf_handle h, double tau, bool force, int *changed_out, bool in_step) {
  int use_tau;
  double f_x, f_x0, f_d;
  tau_factors(h, tau, &use_tau, &f_x, &f_x0, &f_d);
  hipStream_t s = h->stream;
  if (force && !h->sparse) {
    // the mask, straight into h->mask, and its compaction in one launch
    const bool spec = in_step && h->counts_known && step_spec();
    if (changed_out) *changed_out = 1;
    // a step enqueued with |A| = 0: its residual and reduced rhs in the same launch (newton_core_async
    // then enqueues neither; a step that is discarded and redone takes the launches of its own)
    h->front_done = spec && h->nA == 0 && step_fused();
    if (h->front_done)
      launch_mask_compact_rhs(s, h->n, h->m, h->nI, use_tau, h->lamb, f_x, f_x0, f_d, h->dt, h->fact, h->xhat,
                              h->yhat, h->x, h->y, h->g, h->c, h->slb, h->sub, h->mask, h->idxI, h->idxA, h->pos,
                              h->counts, h->nI, h->F, h->b0full, h->rhs);
    else
      launch_mask_compact(s, h->n, use_tau, h->lamb, f_x, f_x0, f_d, h->xhat, h->x, h->g, h->slb, h->sub,
                          h->mask, h->idxI, h->idxA, h->pos, h->counts, spec ? h->nI : -1);
    return adopt_index_sets(h, spec);
  }
  launch_active_set(s, h->n, use_tau, h->lamb, f_x, f_x0, f_d, h->xhat, h->x, h->g, h->slb, h->sub,
                    h->mask_new);
  int changed = 1;
  if (h->mask_set && !force) {
    HIPCHK(h, hipMemsetAsync(h->counts + 2, 0, sizeof(int), s));
    launch_mask_diff(s, h->n, h->mask, h->mask_new, h->counts + 2);
    int rc;
    if ((rc = down(h, h->h_counts + 2, h->counts + 2, sizeof(int)))) return rc;
    HIPCHK(h, hipStreamSynchronize(s));
    if (in_step) ++h->stat_host_syncs;
    changed = h->h_counts[2] != 0;
  }
  if (changed_out) *changed_out = changed;
  if (changed) {
    launch_copy_u8(s, h->mask, h->mask_new, h->n);
    if (h->sparse) {  // full-size banded system: no index sets to rebuild
      h->mask_set = true;
      invalidate_factor(h);
      return PGF_OK;
    }
    return refresh_index_sets(h, in_step);
  }
  return PGF_OK;
}

int pgf_qp_update_active_set(pgf_handle h, double tau, int *changed) {
  if (!h) return PGF_INVALID;
  int rc;
  if ((rc = qp_ready(h))) return rc;
  (void)hipSetDevice(h->device);
  qp_eval(h);
  if (h->form) return unsym_refresh_mask(h, tau, false, changed, true);
  return qp_refresh_mask(h, tau, false, changed, false);
}

int pgf_qp_advance_outer(pgf_handle h, double dt, double rho) {
  if (!h) return PGF_INVALID;
  int rc;
  if ((rc = qp_ready(h))) return rc;
  if (!(dt > 0.0) || !(rho > 0.0)) return fail(h, PGF_INVALID, "dt and rho must be positive");
  (void)hipSetDevice(h->device);
  const bool one = step_fused() && !h->sparse;  // the copies and the scaling in one launch
  if (!one) {
    launch_copy(h->stream, h->xhat, h->x, h->n);
    launch_copy(h->stream, h->yhat, h->y, h->m);
  }
  if (rho != h->rho) h->eval_fresh = false;  // g depends on rho
  h->dt = dt;
  h->lamb = 1.0 / dt;
  h->rho = rho;
  h->fact = 1.0 / (1.0 + h->lamb * rho);
  h->delta = h->lamb / (1.0 + h->lamb * rho);
  if (one)
    launch_advance_outer(h->stream, h->n, h->m, h->lamb, h->x, h->y, h->lb, h->ub, h->xhat, h->yhat, h->slb,
                         h->sub);
  else
    launch_scale_bounds(h->stream, h->n, h->lamb, h->lb, h->ub, h->slb, h->sub);
  h->mask_set = false;
  invalidate_factor(h);
  return PGF_OK;
}

// newton_core_async at the device point, (x, y) <- (xn, yn), and the read-back of the step's status:
// dense, ONE copy of the status block (the factorisation's and the chained solve's status words
// are gathered into it by the step update, DenseLdlt::defer_status).
static int enqueue_qp_step(pgf_handle h) {
  qp_eval(h);
  bool did_factor;
  const bool armed = h->fac.inject_helper_failure != 0;
  h->fac.defer_status = true;  // (read by the dense factorisation and solves only)
  int rc = newton_core_async(h, &did_factor);
  h->fac.defer_status = false;
  h->step_took_inject = armed && !h->fac.inject_helper_failure;
  if (rc) return rc;
  swap_point(h);  // (x, y) <- (xn, yn)
  h->eval_fresh = false;
  // g and c at the new point, enqueued NOW: the next step needs them first thing, and behind the
  // step's host synchronisation the four small launches would wait for the host one by one
  // (~35 us of gaps at config 2).  Whatever moves the point afterwards (refinement, a repeated
  // step, pgf_qp_set_point, a new rho) clears eval_fresh again.
  if (h->sparse) return PGF_OK;  // (nothing ahead; band_step_async has enqueued the copy of its status)
  if (h->fused_eval_done) {  // (newton_core_async did it beside the residual check)
    h->eval_fresh = true;
    h->fused_eval_done = false;
  } else if (eval_ahead()) {
    qp_eval(h);
  }
  return down(h, h->h_stat, h->stat, STAT_COPY * sizeof(double));
}

// A step in flight that was enqueued with speculative index-set sizes, after a host
// synchronisation that brought its status block: if the compaction found other sizes, the step
// ran with the previous |I|, |A| and its factor, flags and point are garbage (every index it read
// was in range).  Nothing of it is reported or acted on -- no PGF_SINGULAR, no refinement, no
// change of condensed_veto, no switching off of the chain helpers or the chained solves (a
// chained solve's half-published state is only reset) -- and it is enqueued again from the
// point it started at, with the true sizes.  *redone: it was.
static int settle_spec(pgf_handle h, bool *redone) {
  *redone = false;
  if (!h->step_pending || !h->spec_pending) return PGF_OK;  // (never speculative on a banded handle)
  h->spec_pending = false;
  if (!h->h_counts[3]) return PGF_OK;
  ++h->stat_redone;
  const int *w = reinterpret_cast<const int *>(h->h_stat + 14);
  ldlt_chain_discard(h->fac, (h->stat_bits & 2) ? w[3] : 0);
  h->stat_bits = 0;  // (the discarded step's status words are not read)
  // a test hook's injected helper failure belongs to the step that is kept
  if (h->step_took_inject) h->fac.inject_helper_failure = 1;
  gram_uncount(h);
  h->fac.factored = false;
  h->lu_active = false;
  swap_point(h);
  h->eval_fresh = false;  // (g, c were evaluated ahead at the point that is discarded)
  adopt_counts(h);
  int rc;
  if ((rc = enqueue_qp_step(h))) return rc;
  *redone = true;
  return PGF_OK;
}

int pgf_qp_step_async(pgf_handle h, unsigned policy, double tau) {
  if (!h) return PGF_INVALID;
  int rc;
  if ((rc = qp_ready(h))) return rc;
  if (h->step_pending) return fail(h, PGF_NOT_READY, "pgf_qp_sync the previous step first");
  (void)hipSetDevice(h->device);
  if (h->form) return unsym_qp_step_async(h, policy, tau);
  h->front_done = false;
  qp_eval(h);
  if (policy & PGF_STEP_RECOMPUTE_MASK) {
    // Full (newton.py:83-89): the mask is always re-set, which drops the factor;
    // ActiveSet (:203-215): only when it differs elementwise.
    const bool force = (policy & PGF_STEP_REFACTOR) != 0;
    if ((rc = qp_refresh_mask(h, tau, force, nullptr, true))) return rc;
  }
  if (!h->mask_set) return fail(h, PGF_NOT_READY, "no active set: pgf_qp_update_active_set first");
  if (policy & PGF_STEP_REFACTOR) invalidate_factor(h);
  if ((rc = enqueue_qp_step(h))) return rc;
  h->step_pending = true;
  return PGF_OK;
}

int pgf_qp_sync(pgf_handle h, int *n_neg, double *diff) {
  if (!h) return PGF_INVALID;
  if (!h->step_pending) return fail(h, PGF_NOT_READY, "no step pending");
  h->step_pending = false;
  (void)hipSetDevice(h->device);
  if (h->form) return unsym_qp_sync(h, n_neg, diff);
  hipError_t e;
  int rc;
  if ((rc = band_status_sync(h))) return rc;
  if (!h->sparse) {
    // the step's one wait: its status block
    HIPCHK(h, hipStreamSynchronize(h->stream));
    ++h->stat_host_syncs;
    h->step_pending = true;  // (settle_spec acts on a step in flight)
    bool redone;
    rc = settle_spec(h, &redone);
    h->step_pending = false;
    if (rc) return rc;
    if (redone) {
      HIPCHK(h, hipStreamSynchronize(h->stream));
      ++h->stat_host_syncs;
    }
    absorb_status(h);
  }
  int st = finish_factor_state(h, &e);  // flags are only rewritten by a factor launch
  if (st == 2) {
    // the chain's helper workgroups failed their checks (off now): the step is computed again
    // from the point it started at
    swap_point(h);
    h->eval_fresh = false;  // (g, c were evaluated ahead at the point that is discarded)
    if ((rc = enqueue_qp_step(h))) return rc;
    if (!h->sparse) {
      HIPCHK(h, hipStreamSynchronize(h->stream));
      ++h->stat_host_syncs;
      absorb_status(h);
    }
    st = finish_factor_state(h, &e);
    if (st == 2) return fail(h, PGF_HIP_ERROR, k_helper_msg);
  }
  if (st < 0) return hip_fail(h, e, "step");
  if (st == 1) return fail(h, PGF_SINGULAR, "zero or non-finite pivot in LDL^T of the KKT matrix");
  if ((rc = chain_recover(h, true))) return rc;
  if ((rc = refine_if_needed(h, true))) return rc;
  if (n_neg) *n_neg = h->fac.n_neg;
  if (diff) *diff = h->h_scal[0];
  return PGF_OK;
}

int pgf_set_refinement(pgf_handle h, int mode, double tol, double fail_tol) {
  if (!h || mode < 0 || mode > 1) return PGF_INVALID;
  h->refine_mode = mode;
  if (tol > 0.0) h->refine_tol = tol;
  if (fail_tol > 0.0) h->refine_fail = fail_tol;
  return PGF_OK;
}

int pgf_refinement_stats(pgf_handle h, int *refined, int *lu_fallbacks, double *last_rel_residual) {
  if (!h) return PGF_INVALID;
  if (refined) *refined = h->stat_refined;
  if (lu_fallbacks) *lu_fallbacks = h->stat_lu;
  if (last_rel_residual) *last_rel_residual = h->stat_last_rel;
  return PGF_OK;
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
  if (host_syncs) *host_syncs = h->stat_host_syncs;
  if (redone_steps) *redone_steps = h->stat_redone;
  return PGF_OK;
}

int pgf_debug_gram_stats(pgf_handle h, int *builds, int *factorisations_with_gram) {
  if (!h) return PGF_INVALID;
  if (builds) *builds = h->stat_gram_builds;
  if (factorisations_with_gram) *factorisations_with_gram = h->stat_gram_factors;
  return PGF_OK;
}

int pgf_debug_tail_stats(pgf_handle h, int *fused_steps, int *plain_steps) {
  if (!h) return PGF_INVALID;
  if (fused_steps) *fused_steps = h->stat_tail_fused;
  if (plain_steps) *plain_steps = h->stat_tail_plain;
  return PGF_OK;
}

int pgf_debug_head_stats(pgf_handle h, int *fused, int *plain) {
  if (!h) return PGF_INVALID;
  if (fused) *fused = h->stat_head_fused;
  if (plain) *plain = h->stat_head_plain;
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
  if (h->lu_active) return 3;
  if (!h->fac.factored) return 0;
  return h->condensed ? 2 : 1;
}

int pgf_debug_chain_helpers(int on) {
  const int was = ldlt_chain_helpers_enabled() ? 1 : 0;
  if (on == 0 || on == 1) ldlt_chain_helpers_set(on == 1);
  return was;
}

int pgf_qp_step(pgf_handle h, unsigned policy, double tau, int inertia_check, int *n_neg,
                double *diff) {
  int rc;
  if (h && h->form && inertia_check)
    return fail(h, PGF_INVALID, "no inertia with an unsymmetric formulation (LU)");
  if ((rc = pgf_qp_step_async(h, policy, tau))) return rc;
  if ((rc = pgf_qp_sync(h, n_neg, diff))) return rc;
  if (!h->form && inertia_check && h->fac.n_neg != h->m)
    return fail(h, PGF_INERTIA, "Invalid matrix inertia");
  return PGF_OK;
}

int pgf_qp_residual_norm(pgf_handle h, double *norm_out, double *norm_out_dev) {
  if (!h) return PGF_INVALID;
  int rc;
  if ((rc = qp_ready(h))) return rc;
  (void)hipSetDevice(h->device);
  qp_eval(h);
  // (the norm also reaches norm_out_dev from the launch itself).  Between pgf_qp_step_async and
  // pgf_qp_sync the point is that of the step in flight; if that step turns out to have run with
  // stale index-set sizes (settle_spec), it is redone and the norm taken again at its new point.
  for (int pass = 0; pass < 2; ++pass) {
    launch_unscaled_res_norm(h->stream, h->n, h->m, h->dt, h->xhat, h->yhat, h->x, h->y, h->g, h->c,
                             h->lb, h->ub, h->red, h->scal + 1, norm_out_dev, h->ticket + 1);
    if ((rc = down(h, h->h_scal + 1, h->scal + 1, sizeof(double)))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    bool redone;
    if ((rc = settle_spec(h, &redone))) return rc;
    if (!redone) break;
    qp_eval(h);
  }
  if (norm_out) *norm_out = h->h_scal[1];
  return PGF_OK;
}

int pgf_qp_measures(pgf_handle h, double active_tol, double *out) {
  if (!h || !out) return PGF_INVALID;
  if (!h->qp_mode || !h->point_set || !h->bounds_set)
    return fail(h, PGF_NOT_READY, "pgf_set_bounds, pgf_qp_set_problem, pgf_qp_set_point first");
  (void)hipSetDevice(h->device);
  int rc0;
  if ((rc0 = settle_before_read(h))) return rc0;
  hipStream_t s = h->stream;
  const int n = h->n, m = h->m;
  // c = A x - b and r = Q x + q + A'y (no rho term: iterate.py:141, 176)
  launch_copy(s, h->w, h->y, m);
  if (h->sparse) {
    band_measures_eval(h);
  } else {
    launch_gemv_rows(s, m, n, h->J, h->ldj, h->x, h->b, -1.0, h->c);
    launch_gemvT(s, m, n, h->J, h->ldj, h->w, h->q, h->partial, PGF_GEMVT_PARTS, h->tmpn);
    launch_gemv_rows(s, n, n, h->H, h->ldh, h->x, h->tmpn, 1.0, h->F);
  }
  const int nb = (n + m + 255) / 256;
  double *res = h->meas + 4 * nb;
  launch_measures(s, n, m, active_tol, h->x, h->y, h->F, h->c, h->lb, h->ub, h->meas, res);
  int rc;
  if ((rc = down(h, h->h_meas, res, 4 * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(s));
  std::memcpy(out, h->h_meas, 4 * sizeof(double));
  return PGF_OK;
}

