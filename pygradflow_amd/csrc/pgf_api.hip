// C ABI of libpgf_hip.so (include/pgf_hip.h): the dense Symmetric handle -- its lifecycle, the
// uploads of bounds, outer iterate and derivatives (dense and CSR), the active set and its index
// sets, and the entry points that solve with or read the reduced KKT matrix (pgf_linear_solve,
// pgf_kkt_apply, pgf_get_kkt).  The factorisation is in pgf_api_factor.hip, the accuracy guard in
// pgf_api_guard.hip, the Newton step and the device-resident LQ mode in pgf_api_step.hip.
// (pgf_hip.h declares every entry point extern "C": the definitions follow it.)
#include <cmath>
#include <cstring>
#include <new>

#include "pgf_api_internal.h"
#include "pgf_kernels.h"
#include "pgf_unsym.h"

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
    A_(guard.rs_v, n) A_(guard.rs_lv, n) A_(guard.rs_u, n) A_(guard.rs_wy, m) A_(guard.rs_r, N + 1) A_(guard.rs_d, N + 1);
    A_(cond.cd_t, n + 1);
  }
  A_(mask, n) A_(mask_new, n) A_(idxI, n) A_(idxA, n) A_(pos, n);
#undef A_
  // index lists hold valid indices from the start: a step enqueued with stale counts reads them
  if ((e = hipMemset(h->stat, 0, STAT_ALLOC * sizeof(double))) != hipSuccess ||
      (n && (e = hipMemset(h->idxI, 0, (size_t)n * sizeof(int))) != hipSuccess) ||
      (n && (e = hipMemset(h->idxA, 0, (size_t)n * sizeof(int))) != hipSuccess) ||
      (n && (e = hipMemset(h->pos, 0, (size_t)n * sizeof(int))) != hipSuccess) ||
      // (coherent: the hand-back's last launch stores into it while the host spins on the word behind it)
      (e = hipHostMalloc((void **)&h->h_stat, (STAT_COPY + 1) * sizeof(double),
                         hipHostMallocMapped | hipHostMallocCoherent)) != hipSuccess ||
      (e = hipHostMalloc((void **)&h->h_meas, 4 * sizeof(double))) != hipSuccess) {
    pgf_destroy(h);
    return PGF_HIP_ERROR + (int)e;
  }
  if ((e = hipHostGetDevicePointer((void **)&h->hb.dev, h->h_stat, 0)) != hipSuccess) {
    pgf_destroy(h);
    return PGF_HIP_ERROR + (int)e;
  }
  h->guard.rs_red = h->stat;
  h->scal = h->stat + 8;
  h->counts = reinterpret_cast<int *>(h->stat + 12);
  h->ticket = reinterpret_cast<unsigned *>(h->stat + 16);
  for (int i = 0; i <= STAT_COPY; ++i) h->h_stat[i] = 0.0;  // (the sequence word: 0, as hb.issued)
  h->guard.h_rs = h->h_stat;
  h->h_scal = h->h_stat + 8;
  h->h_counts = reinterpret_cast<int *>(h->h_stat + 12);
  h->sparse = sparse;
  h->sp.blk.split = band_split_default();
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
                  h->meas, h->guard.rs_v, h->guard.rs_lv, h->guard.rs_u, h->guard.rs_wy, h->guard.rs_r, h->guard.rs_d, h->cond.cd_t,
                  h->cond.G,    h->cond.gram_aux};
  for (void *p : ptrs)
    if (p) (void)hipFree(p);
  if (h->h_stat) (void)hipHostFree(h->h_stat);
  if (h->h_mask_stage) (void)hipHostFree(h->h_mask_stage);
  if (h->mask_ev) (void)hipEventDestroy(h->mask_ev);
  lu_free(h->guard.lu);
  lu_free(h->unsym.ulu);
  if (h->h_meas) (void)hipHostFree(h->h_meas);
  band_free(h);
  ls_free(h);
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
  h->guard.norms_valid = false;
  h->ls.hat_fresh = false;
  h->cond.gram_valid = false;
  h->cond.cond_since_upload = 0;
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
  // no finite bound anywhere: the active set is empty at every point (pgf_solver::unb)
  bool none = true;
  for (int i = 0; i < h->n && none; ++i) none = lb[i] == -HUGE_VAL && ub[i] == HUGE_VAL;
  h->unb.no_finite_bound = none;
  h->unb.lists_ready = false;
  drop_norm(h);
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
  if (rho != h->rho) h->eval_fresh = false;  // g depends on rho (as pgf_qp_advance_outer; the point may stay)
  set_outer_scalars(h, dt, rho);
  launch_scale_bounds(h->stream, h->n, h->lamb, h->lb, h->ub, h->slb, h->sub);
  h->outer_set = true;
  h->mask_set = false;
  h->ls.hat_fresh = false;
  drop_norm(h);
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
  h->unsym.h_has_lag_only = false;
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
  h->unsym.h_has_lag_only = false;
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
  if (h->unsym.form == PGF_FORM_STANDARD)  // the unscaled projection and thresholds
    launch_unscaled_active_set(h->stream, h->n, use_tau, h->dt, use_tau ? 1.0 - tau * h->lamb : 0.0,
                               use_tau ? tau * h->lamb : 0.0, use_tau ? tau : 0.0, h->xhat, h->tmpn, h->g,
                               h->lb, h->ub, h->mask_new);
  else
    launch_active_set(h->stream, h->n, use_tau, h->lamb, f_x, f_x0, f_d, h->xhat, h->tmpn, h->g,
                      h->slb, h->sub, h->mask_new);
  if ((rc = down(h, mask_out, h->mask_new, h->n))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->eval_fresh = false;
  drop_norm(h);
  return PGF_OK;
}

// After the compaction of h->mask into index lists + counts (enqueued by the caller with
// expect = h->nI when `spec', else -1).  spec: a step is being enqueued and will run with the last
// known |I|, |A| -- no host synchronisation here; pgf_qp_sync reads the true counts and the
// mismatch word with the step's status block and redoes the step if they differ.  Otherwise the
// counts are awaited (one host sync).
int adopt_index_sets(pgf_handle h, bool spec) {
  h->mask_set = true;
  invalidate_factor(h);
  if (spec) {
    h->flight.spec_pending = true;
    return PGF_OK;
  }
  int rc;
  if ((rc = down(h, h->h_counts, h->counts, 2 * sizeof(int)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  ++h->dbg.stat_host_syncs;
  adopt_counts(h);
  return PGF_OK;
}
int refresh_index_sets(pgf_handle h, bool in_step) {
  const bool spec = in_step && h->counts_known && step_spec();
  h->unb.lists_ready = false;
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
  // (an empty mask compacts to what a handle without finite bounds keeps: zero, the identity, (n, 0, ., 0))
  h->unb.lists_ready = !h->sparse && na == 0;
  if (!h->sparse)
    launch_compact(h->stream, h->n, h->mask, h->idxI, h->idxA, h->pos, h->counts, h->nI);
  return PGF_OK;
}

int pgf_reduced_dims(pgf_handle h, int *n_inactive, int *n_reduced) {
  if (!h) return PGF_INVALID;
  if (!h->mask_set) return fail(h, PGF_NOT_READY, "no active set");
  if (n_inactive) *n_inactive = h->nI;
  if (n_reduced) *n_reduced = h->unsym.form ? h->n + h->m : h->N;
  return PGF_OK;
}

int check_ready(pgf_handle h) {
  if (!h->outer_set) return fail(h, PGF_NOT_READY, "pgf_set_outer first");
  if (h->sparse ? !h->sp.pat.values_set : !h->derivs_set)
    return fail(h, PGF_NOT_READY, "pgf_set_derivs_* / pgf_sparse_set_values first");
  if (!h->mask_set) return fail(h, PGF_NOT_READY, "pgf_set_active_set first");
  return PGF_OK;
}

void assemble(pgf_handle h, double *K, int64_t ldk) {
  launch_assemble_kkt(h->stream, K, ldk, h->H, h->ldh, h->J, h->ldj, h->idxI, h->nI, h->m, h->lamb,
                      h->delta);
}

int pgf_linear_solve(pgf_handle h, const double *rhs, int trans, double *sol) {
  // (the Symmetric path ignores trans: K is symmetric; a formulation honours it)
  if (!h) return PGF_INVALID;
  int rc;
  if ((rc = check_ready(h))) return rc;
  if (h->sparse) return band_linear_solve(h, rhs, sol);
  if (h->unsym.form) {  // the full system, A or A^T (cond_estimate.py:82)
    const int Nf = h->n + h->m;
    if (Nf && (!rhs || !sol)) return fail(h, PGF_INVALID, "null argument");
    if (Nf == 0) return PGF_OK;
    (void)hipSetDevice(h->device);
    if (!h->unsym.ulu_ok && (rc = unsym_factor(h))) return rc;
    if ((rc = up(h, h->rhs, rhs, (size_t)Nf * sizeof(double)))) return rc;
    HIPCHK(h, lu_solve_async(h->unsym.ulu, h->rhs, h->sol, trans));
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
  if (h->guard.lu_active) {  // the pivoted factor took over for this matrix (refine_if_needed)
    HIPCHK(h, lu_solve_async(h->guard.lu, h->rhs, h->sol, 0));
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
  const int rows = h->sparse || h->unsym.form ? h->n + h->m : h->N;
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
  if ((rc = up(h, h->guard.rs_d, v, (size_t)h->N * sizeof(double)))) return rc;
  HIPCHK(h, hipMemsetAsync(h->guard.rs_r, 0, (size_t)(h->N + 1) * sizeof(double), h->stream));
  launch_kkt_residual(h->stream, h->n, h->m, h->nI, h->lamb, h->delta, h->H, h->ldh, h->J, h->ldj,
                      h->idxI, h->pos, h->mask, h->guard.rs_r, h->guard.rs_d, h->guard.rs_v, h->guard.rs_lv, h->guard.rs_u,
                      h->guard.rs_wy, h->partial, PGF_GEMVT_PARTS, h->guard.rs_r, h->guard.rs_red);
  if ((rc = down(h, out, h->guard.rs_r, (size_t)h->N * sizeof(double)))) return rc;
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
