// What the translation units behind the C ABI share -- pgf_api.hip: the dense Symmetric handle's
// lifecycle, uploads, index sets and linear solves; pgf_api_factor.hip: its factorisation (condensed
// order, Gram matrix); pgf_api_guard.hip: its accuracy guard; pgf_api_step.hip: the Newton step and
// the device-resident LQ mode; pgf_api_line_search.hip: the Globalized policy's line search around that
// step; pgf_api_band.hip: the banded solve driver with pgf_api_band_setup.hip its configuration and
// lifetimes (pattern, values, block size, split, borders); pgf_api_unsym.hip: the
// unsymmetric formulations; pgf_api_batch.hip: the batch driver (lifecycle, outer step, host-driven
// step) with pgf_api_band_batch.hip its banded half, pgf_api_batch_ctl.hip its device-resident
// controller, pgf_api_batch_line_search.hip its Globalized policy and pgf_api_batch_read.hip its
// read-outs; pgf_api_comm.hip: the RCCL communicator; pgf_api_aux.hip: profiling read-out,
// the stand-alone linear solver and the pgf_debug_* hooks -- the handles, the error helpers and
// the small interfaces between the files.
#pragma once

#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../include/pgf_hip.h"
#include "pgf_band_batch.h"
#include "pgf_batch.h"
#include "pgf_batch_line_search.h"
#include "pgf_ldlt.h"
#include "pgf_lu.h"
#include "pgf_sparse.h"

// The status block of a dense step (doubles): every word the host reads after the step, read
// with ONE device-to-host copy of STAT_COPY doubles into the pinned mirror h_stat.
//   [0, 8)   rs_red: max |r|, max |rhs|, max |s| of the residual check; [4, 7) the matrix norms
//   [8, 12)  scal:   [0] step diff, [1] residual norm
//   [12, 14) counts (int): |I|, |A|, mask difference, size mismatch of a speculative step
//   [14, 16) status (int): factor flags [0, 3), chained-solve status [3] (DenseLdlt::h_flags)
//   [16, 17) two tickets of the last-workgroup reductions (never copied)
// With the hand-back (pgf_solver::hb) the step's last launch stores the STAT_COPY doubles into
// h_stat itself; h_stat[STAT_COPY] is the sequence word it writes behind them.
#define STAT_COPY 16
#define STAT_ALLOC 17
#define STAT_NORM 9  // scal[1] inside the block

#define PGF_GEMVT_PARTS 32  // row chunks of the J^T products' partial sums (pgf_solver::partial)

struct pgf_solver {
  int n = 0, m = 0, device = 0;
  hipStream_t stream = nullptr;
  std::string err = "";
  // host-known state
  double dt = 0, lamb = 0, rho = 0, fact = 0, delta = 0;
  bool bounds_set = false, outer_set = false, derivs_set = false, mask_set = false;
  bool qp_mode = false, point_set = false, eval_fresh = false;
  int nI = 0, nA = 0, N = 0;
  // device data
  double *H = nullptr, *J = nullptr;
  int64_t ldh = 0, ldj = 0;
  bool ownH = false, ownJ = false;
  double *Hown = nullptr, *Jown = nullptr;  // library-owned storage (reused across uploads)
  // staging of pgf_set_derivs_csr (grown on demand): row pointers, column indices, values
  int *csr_ptr = nullptr, *csr_idx = nullptr;
  double *csr_val = nullptr;
  size_t csr_ptr_cap = 0, csr_nnz_cap = 0;
  double *lb = nullptr, *ub = nullptr, *slb = nullptr, *sub = nullptr;
  double *xhat = nullptr, *yhat = nullptr;
  double *x = nullptr, *y = nullptr, *xn = nullptr, *yn = nullptr;
  double *g = nullptr, *c = nullptr, *F = nullptr, *b0full = nullptr;
  double *rhs = nullptr, *sol = nullptr, *dx = nullptr, *dy = nullptr;
  double *q = nullptr, *b = nullptr, *w = nullptr, *tmpn = nullptr, *partial = nullptr;
  double *red = nullptr, *scal = nullptr;  // scal[0] diff, scal[1] residual norm
  double *meas = nullptr;                  // termination measures: partial maxima + 4 results
  double *h_meas = nullptr;
  uint8_t *mask = nullptr, *mask_new = nullptr;
  int *idxI = nullptr, *idxA = nullptr, *pos = nullptr, *counts = nullptr;
  // pinned host mirrors
  int *h_counts = nullptr;
  double *h_scal = nullptr;
  DenseLdlt fac;
  SparseDev sp;
  bool sparse = false;
  PgfProfile prof;
  bool step_pending = false;
  // status block (STAT_COPY above) and its pinned mirror
  double *stat = nullptr, *h_stat = nullptr;
  unsigned *ticket = nullptr;
  // speculative index-set sizes (pgf_qp_step_async): the step is enqueued with the last known
  // |I|, |A|; the compaction flags a mismatch in counts[3], and pgf_qp_sync redoes the step
  // (flight.spec_pending)
  bool counts_known = false;
  uint8_t *h_mask_stage = nullptr;  // pinned staging of pgf_set_active_set's mask
  hipEvent_t mask_ev = nullptr;

  // ---- the accuracy guard (pgf_api_guard.hip) ----
  struct {
    // residual check of the reduced system (dense mode): scratch vectors, r = rhs - K s, the
    // correction, [max |r|, max |rhs|, max |s|] on device and pinned host; the pivoted LU that
    // takes over when refinement does not converge (allocated on first use)
    double *rs_v = nullptr, *rs_lv = nullptr, *rs_u = nullptr, *rs_wy = nullptr, *rs_r = nullptr,
           *rs_d = nullptr, *rs_red = nullptr, *h_rs = nullptr;
    DenseLu lu;
    bool lu_active = false;       // the current factor is the LU (until the next factorisation)
    int refine_mode = 1;          // 0 off, 1 check + refine on demand (default)
    double refine_tol = 1e-11, refine_fail = 1e-7;
    // ||H||_inf, ||J||_inf, ||J||_1 of the matrices in HBM (h_rs[4..6]); computed the first time a
    // residual misses refine_tol against max |rhs| alone
    bool norms_valid = false;
    int stat_refined = 0, stat_lu = 0;
    double stat_last_rel = 0.0;
    // the factorisation step's own residual was far below the tolerance: the back-solve steps
    // with the same factor (same backward error, other right-hand sides) skip the check
    bool factor_clean = false;
    bool rs_skipped = false;
  } guard;

  // ---- the condensed order and its resident Gram matrix (pgf_api_factor.hip) ----
  struct {
    // the current dense factor is that of the condensed system (constraint block eliminated
    // first, condensed_wanted); cd_t: its right-hand side
    bool condensed = false;
    bool condensed_veto = false;  // it met a zero pivot: natural order until the matrix changes
    double *cd_t = nullptr;
    // The condensed system's rank-m term from a resident Gram matrix (gram_prepare): G = J^T J,
    // n x n with row stride ldg, lower triangle; gram_aux: the identity index list of the build
    // (n ints) and, behind it, the build's tile counter.  Valid until the next pgf_set_derivs_*
    // (as norms_valid); gram_off: the allocation failed once, the handle keeps the virtual blocks.
    double *G = nullptr;
    int64_t ldg = 0;
    int *gram_aux = nullptr;
    bool gram_valid = false, gram_off = false;
    int cond_since_upload = 0;  // condensed factorisations enqueued since the last derivative upload
  } cond;

  // ---- the hand-back of a dense qp step to the host (pgf_api_step.hip; PGF_STEP_HANDBACK) ----
  // h_stat is coherent host memory: the last launch of a step with the fused tail stores the status
  // block into it and then the sequence word h_stat[STAT_COPY] (issued: the value of the last such
  // launch enqueued), and the step's one wait spins on that word (hb_wait) instead of calling the
  // runtime.  armed: the step in flight ends in such a launch (else: the copy and
  // hipStreamSynchronize).  seen: the last value a wait has observed -- a wait for a value already
  // seen returns at once.  norm_fresh: scal[1] of the block is the residual norm of the current
  // device point under the current outer point (written by the tail's last launch); cleared by
  // whatever moves either (drop_norm).
  struct {
    double *dev = nullptr;  // h_stat as the device addresses it
    unsigned long long issued = 0, seen = 0;
    bool armed = false, norm_fresh = false;
    double t_enqueued = 0.0, last_step_s = -1.0;  // seconds: when the step was enqueued, how long the last one took
    double bound_override = -1.0;                 // pgf_debug_handback_spin_bound (< 0: the derived bound)
  } hb;

  // ---- a handle without a finite bound (pgf_set_bounds; PGF_UNBOUNDED_FRONT) ----
  // every lb is -inf and every ub +inf: the active set is empty at every point, so the mask (zero),
  // the index lists (the identity) and the counts (n, 0, ., 0) are written once (lists_ready; cleared by
  // whatever else writes them) and a step takes neither the compaction nor the mask difference
  struct {
    bool no_finite_bound = false, lists_ready = false;
  } unb;

  // ---- what the step or factorisation in flight took: valid until it is settled (pgf_qp_sync,
  // factor_finish) ----
  struct {
    int last_solve = 0;  // what newton_core_async enqueued: 1 back-solve of row N, 2 full solve
    int stat_bits = 0;   // DenseLdlt::status_words gathered into the block by the step update
    bool spec_pending = false;      // it was enqueued with speculative index-set sizes (counts_known)
    bool step_took_inject = false;  // the step in flight consumed pgf_debug_fail_next_helper
    // PGF_STEP_FUSED: the forced mask refresh of the step being enqueued has also written F, b0full
    // and the reduced rhs (consumed by newton_core_async)
    bool front_done = false;
    bool fused_eval_done = false;  // newton_core_async evaluated g, c at (xn, yn) beside the residual check
    bool fused_norm_done = false;  // ... and the tail's last launch left that point's residual norm and the hand-back
    // what the factorisation in flight added to the counters (taken back when it is discarded)
    bool fac_counted = false, fac_used_gram = false;
    // the factorisation in flight took the step's head beside its first chain (1) or not (2);
    // pgf_debug_head_stats counts both kinds
    int fac_head = 0;
    // forget what the last factorisation counted
    void forget_factor() {
      fac_counted = fac_used_gram = false;
      fac_head = 0;
    }
  } flight;

  // ---- the Globalized policy's line search (pgf_api_line_search.hip; allocated by the first step
  // that carries PGF_STEP_LINE_SEARCH) ----
  struct {
    double newton_tol = 1e-8;  // Params().newton_tol (pgf_qp_set_line_search)
    // g, c at the outer point (hat_fresh: current for the outer step, the matrices and rho as they
    // are); the direction's images u = A dx, v = Q dx + A'(rho u + dy); zeros in place of q and b;
    // the ladder's partial sums; the block the host reads (pgf_line_search.h) and its pinned mirror
    double *ghat = nullptr, *chat = nullptr, *u = nullptr, *v = nullptr, *zero = nullptr, *red = nullptr,
           *blk = nullptr, *h_blk = nullptr;
    bool hat_fresh = false;
    bool want = false;    // the step being enqueued or in flight carries the bit
    // the handle's (x, y, g, c) name the outer point's vectors, (ox, oy, og, oc) the device
    // point's, until the step in flight is settled (ls_enter / ls_leave)
    bool active = false;
    double *ox = nullptr, *oy = nullptr, *og = nullptr, *oc = nullptr;
    bool have_stats = false;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;  // around the stage while profiling is enabled
    double stage_ms = 0.0;
  } ls;

  // ---- counters read only by the pgf_debug_* hooks (pgf_api_aux.hip, pgf_api_unsym.hip) ----
  struct {
    int stat_host_syncs = 0, stat_redone = 0;  // pgf_debug_step_stats
    int stat_hb_word = 0, stat_hb_fallback = 0;    // pgf_debug_handback_stats
    int stat_compactions = 0, stat_unb_fronts = 0;  // pgf_debug_front_stats
    // steps enqueued with the residual check and the evaluation ahead in the fused / the separate
    // launches (pgf_debug_tail_stats)
    int stat_tail_fused = 0, stat_tail_plain = 0;
    int stat_gram_builds = 0, stat_gram_factors = 0;  // pgf_debug_gram_stats
    int stat_head_fused = 0, stat_head_plain = 0;     // pgf_debug_head_stats
    int stat_unsym_asm = 0, stat_unsym_lu = 0;        // pgf_debug_unsym_stats
    int64_t stat_unsym_bytes = 0;
  } dbg;

  // ---- The unsymmetric formulations (pgf_set_formulation, pgf_api_unsym.hip): form --
  // PGF_FORM_*; ulu -- the pivoted LU of the (n + m) x (n + m) Newton matrix, assembled on the
  // device into ulu.A (its own factor: guard.lu belongs to the accuracy guard of the Symmetric
  // path and is never touched here); ulu_ok -- it holds the factor of the current matrix;
  // h_has_lag_only -- H in HBM is the plain Lagrangian Hessian (pgf_qp_set_problem), so Standard
  // adds rho J^T J from the resident Gram matrix; a caller of pgf_set_derivs_* uploads
  // aug_lag_deriv_xx(rho) itself.
  struct {
    int form = PGF_FORM_SYMMETRIC;
    DenseLu ulu;
    bool ulu_ok = false;
    bool h_has_lag_only = false;
    // while profiling is enabled: device time of the assembly launches of unsym_factor since the
    // last pgf_profile_read_ex, and their count
    double acc_unsym_asm_ms = 0;
    int64_t acc_unsym_asm_launches = 0;
  } unsym;
};

struct pgf_linsolver {
  int N = 0, device = 0;
  bool symmetric = true;  // LDL^T (fac) or LU with partial pivoting (lu)
  hipStream_t stream = nullptr;
  DenseLdlt fac;
  DenseLu lu;
  double *rhs = nullptr, *sol = nullptr;
};

static const char *const k_no_handle = "null handle";
static const char *const k_chain_msg = "chained triangular solve failed its placement / timeout check "
                                       "and so did the per-block solve that replaced it";
static const char *const k_band_zero_pivot = "zero or non-finite pivot in the banded KKT factorisation";
static const char *const k_helper_msg =
    "the dense factorisation failed its hand-over checks with and without helper workgroups";
// internal: the factorisation just awaited must be repeated (its chain helpers failed their
// hand-over checks and are switched off now, ldlt_finish -- or the condensed pivot order met a
// zero pivot the natural order may not have: S = A + J^T J / delta can cancel exactly where no
// pivot of K does); never leaves the library
#define PGF_RETRY_FACTOR (-2)

static inline int fail(pgf_handle h, int code, const char *msg) {
  if (h) h->err = msg;
  return code;
}

static inline int hip_fail(pgf_handle h, hipError_t e, const char *where) {
  if (h) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", where, hipGetErrorString(e));
    h->err = buf;
  }
  return PGF_HIP_ERROR + (int)e;
}

#define HIPCHK(h, call)                                  \
  do {                                                   \
    hipError_t e__ = (call);                             \
    if (e__ != hipSuccess) return hip_fail(h, e__, #call); \
  } while (0)

template <typename T>
static inline hipError_t dalloc(T **p, size_t count) {
  return hipMalloc((void **)p, (count ? count : 1) * sizeof(T));
}

// free what is set and null it: device memory (any number of pointers) / pinned host memory
template <typename... T>
static inline void dev_free(T *&...p) {
  ((p ? (void)hipFree(p) : (void)0, p = nullptr), ...);
}
template <typename T>
static inline void pinned_free(T *&p) {
  if (p) (void)hipHostFree(p);
  p = nullptr;
}

template <typename T>
static inline int up_new(pgf_handle h, T **dst, const T *src, size_t count) {
  dev_free(*dst);
  HIPCHK(h, dalloc(dst, count));
  if (count) HIPCHK(h, hipMemcpyAsync(*dst, src, count * sizeof(T), hipMemcpyHostToDevice, h->stream));
  return PGF_OK;
}

static inline int up(pgf_handle h, void *dst, const void *src, size_t bytes) {
  if (!bytes) return PGF_OK;
  HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, h->stream));
  return PGF_OK;
}

static inline int down(pgf_handle h, void *dst, const void *src, size_t bytes) {
  if (!bytes) return PGF_OK;
  HIPCHK(h, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
  return PGF_OK;
}

// (x, y) <-> (xn, yn): a step's new point becomes the point, or a discarded step's point goes back
static inline void swap_point(pgf_handle h) {
  std::swap(h->x, h->xn);
  std::swap(h->y, h->yn);
}
// the index-set sizes the compaction left in the pinned counts, after the wait that brought them
static inline void adopt_counts(pgf_handle h) {
  h->nI = h->h_counts[0];
  h->nA = h->h_counts[1];
  h->N = h->nI + h->m;
  h->counts_known = true;
}
// the depth of the panel V: the constraint count in whole 32-column tiles
static inline int round_up32(int m) { return (m + 31) / 32 * 32; }

// the device point, the outer point, dt, the bounds or the problem's vectors change: the block's
// residual norm is no longer that of the current point
static inline void drop_norm(pgf_handle h) { h->hb.norm_fresh = false; }

static inline void invalidate_factor(pgf_handle h) {
  h->fac.factored = false;
  h->cond.condensed_veto = false;
  h->guard.lu_active = false;
  h->guard.factor_clean = false;
  h->unsym.ulu_ok = false;
}

// ---- the banded driver, for handles created with PGF_CREATE_SPARSE ------------------------------
// pgf_api_band.hip: the solve driver (route dispatch, factor, step, refinement, linear solves,
// evaluation); pgf_api_band_setup.hip: the pgf_sparse_* setters, the debug hooks and the lifetimes
// of SparseDev's groups.  Each is the banded half of the dense function named beside it, which
// hands over in one line.
// doubles of a banded status block (SparseDev::vec.bred, a batch's slice): nred residual pairs, nred
// partial sums of the step update, four pivot flags
static inline size_t band_stat_stride(int nred) { return (size_t)3 * nred + 4; }
// (pgf_api_band_setup.hip)
void band_free(pgf_handle h);                                  // pgf_destroy
bool band_split_default();                                     // pgf_create (PGF_BW_SPLIT)
// (pgf_api_band.hip)
int band_factor_async(pgf_handle h);                           // factor_async
int band_step_async(pgf_handle h, bool *did_factor);           // newton_core_async
int band_status_sync(pgf_handle h);                            // factor_finish, pgf_qp_sync (no-op on dense handles)
int band_refine(pgf_handle h, bool swapped, bool with_step);   // refine_if_needed
int band_linear_solve(pgf_handle h, const double *rhs, double *sol);  // pgf_linear_solve
// pgf_linear_solve_multi: whether the handle takes the panel route, and that route
bool band_multi_panel(pgf_handle h);
int band_linear_solve_multi(pgf_handle h, const double *rhs, int nrhs, int64_t ld, double *sol);
// after a sync that brought the pivot flags to fac.h_flags: settle the wide band's kept factors
void band_kept_resolve(pgf_handle h);                          // finish_factor_state
void band_eval(pgf_handle h);                                  // qp_eval
void band_measures_eval(pgf_handle h);                         // pgf_qp_measures

// ---- the Globalized policy's line search (pgf_api_line_search.hip) -------------------------------
void ls_free(pgf_handle h);                 // pgf_destroy
int ls_reserve(pgf_handle h);               // ls_enter, batch_ls_attach
void ls_enter_names(pgf_handle h);          // ls_enter, batch_ls_handle_enter
int ls_enter(pgf_handle h);                 // pgf_qp_step_async, in front of enqueue_qp_step
void ls_leave(pgf_handle h);                // pgf_qp_step_async (on an error), pgf_qp_sync
int ls_search(pgf_handle h, double *diff);  // pgf_qp_sync, behind the settled step

// ---- the unsymmetric formulations (pgf_api_unsym.hip), for handles with h->unsym.form != 0 -------------
// Each is the unsymmetric half of the dense function named beside it, which hands over in one line.
int unsym_factor(pgf_handle h);                                           // pgf_factor, pgf_linear_solve
int unsym_step_core(pgf_handle h);                                        // pgf_newton_solve
void unsym_mask(pgf_handle h, double tau, const double *x, const double *g, uint8_t *out);  // pgf_residual
int unsym_refresh_mask(pgf_handle h, double tau, bool force, int *changed_out, bool wait_counts);  // pgf_qp_update_active_set
int unsym_qp_step_async(pgf_handle h, unsigned policy, double tau);       // pgf_qp_step_async
int unsym_qp_sync(pgf_handle h, int *n_neg, double *diff);                // pgf_qp_sync
// what they take from the dense handle's files
void tau_factors(pgf_handle h, double tau, int *use_tau, double *f_x, double *f_x0, double *f_d);  // unsym_mask (pgf_api.hip)
void qp_eval(pgf_handle h);                                               // unsym_qp_step_async (pgf_api_step.hip)
bool gram_build(pgf_handle h);                                            // unsym_gram (Standard: H + rho J^T J; pgf_api_factor.hip)
int check_ready(pgf_handle h);                                            // pgf_get_newton_matrix (pgf_api.hip)

// ---- what the batch driver (pgf_api_batch.hip) takes from the dense handle's files -------------
int residual_norms(pgf_handle h);           // batch_store_norms, pgf_batch_advance_outer_each (pgf_api_guard.hip)
// (pgf_api_factor.hip)
int condensed_mode();                       // pgf_batch_create
hipError_t condensed_reserve(pgf_handle h); // pgf_batch_create (and unsym_gram)
int64_t condensed_ldv(int m);               // pgf_batch_create, adopt_batch_factor
bool condensed_growth_ok(pgf_handle h);     // pgf_batch_advance_outer_each
bool eval_ahead();                          // pgf_batch_step_async (pgf_api_step.hip)
// batch_repair_instance: the single-instance accuracy guard on an instance's own handle
struct StepCondY;
void enqueue_residual(pgf_handle h, bool may_skip = false);                                  // (pgf_api_guard.hip)
int refine_if_needed(pgf_handle h, bool swapped, bool with_step = true);                     // (pgf_api_guard.hip)
void enqueue_step_update(pgf_handle h, bool expand = false, const StepCondY *cy = nullptr);  // (pgf_api_step.hip)

// ---- between the dense handle's own files ------------------------------------------------------
// One group per providing file, each beside its users.  (Hidden: these cross files, not the
// library's boundary -- its dynamic symbol table stays as it was.)
#pragma GCC visibility push(hidden)
// pgf_api.hip
int adopt_index_sets(pgf_handle h, bool spec);      // qp_refresh_mask
int refresh_index_sets(pgf_handle h, bool in_step); // qp_refresh_mask
void assemble(pgf_handle h, double *K, int64_t ldk);  // refine_if_needed (the LU's matrix)
// pgf_api_factor.hip
hipError_t kkt_solve_async(pgf_handle h, const double *rhs, double *sol);  // newton_core_async, refine_if_needed, chain_recover, pgf_linear_solve
hipError_t kkt_backsolve_async(pgf_handle h, double *sol, StepCondY *cy = nullptr);  // newton_core_async, chain_recover
int factor_async(pgf_handle h, bool with_rhs);      // newton_core_async
int finish_factor_state(pgf_handle h, hipError_t *e, bool awaited = false);  // pgf_qp_sync (awaited: hb_wait saw the step's word)
int factor_finish(pgf_handle h);                    // pgf_newton_solve
int factor_sync(pgf_handle h);                      // pgf_linear_solve
void gram_uncount(pgf_handle h);                    // settle_spec
// the batch's factor of an instance becomes the handle's own, for refine_if_needed
void adopt_batch_factor(pgf_handle h, int nI, int n_neg_reported, bool condensed, int cond_mp);  // batch_repair_instance
// pgf_api_guard.hip
int chain_recover(pgf_handle h, bool swapped);      // pgf_newton_solve, pgf_qp_sync
// pgf_api_step.hip
bool step_spec();                                   // refresh_index_sets
// pgf_api_band_setup.hip, for pgf_api_band.hip
int band_panel_reserve(pgf_handle h);               // band_linear_solve_multi
#pragma GCC visibility pop

// ---- the batch ---------------------------------------------------------------------------------
// pgf_api_batch.hip: lifecycle, the outer step and the host-driven Newton step (the dense half and
// the dispatch); pgf_api_band_batch.hip: the banded half of those; pgf_api_batch_ctl.hip: the
// device-resident controller, both halves; pgf_api_batch_line_search.hip: the Globalized policy;
// pgf_api_batch_read.hip: read-outs and hooks; pgf_api_comm.hip: the RCCL communicator.
struct pgf_batch_s {
  std::vector<pgf_handle> hs;
  int B = 0, n = 0, m = 0, device = 0;
  hipStream_t stream = nullptr;
  // the instances' BInst records on the device and as create wrote them (the renamed tables of the
  // refinement and the line search are copies of the host's); ctl: BCTL_STRIDE ints per instance
  BInst *tab = nullptr;
  std::vector<BInst> htab;
  int *ctl = nullptr;
  double *ps = nullptr, *h_ps = nullptr;      // per-instance [dt, lambda, rho, fact, delta, ...]
  uint8_t *bytes = nullptr, *h_bytes = nullptr;  // accept / frozen flags on their way to the device
  BatchScalars sc{};
  bool outer_set = false, eval_fresh = false, step_pending = false, have_mask = false;
  bool all_factored = false;
  bool stepped = false;  // a step was enqueued: the instances hold factors made in order cond.last
  // everything batch_alloc gave out (pointer, pinned), freed by pgf_batch_destroy
  std::vector<std::pair<void *, bool>> mem;
  PgfProfile prof;
  std::string err = "";

  // ---- what a step or a read-out leaves, and the pinned mirrors (pgf_api_batch.hip; the read-outs:
  // pgf_api_batch_read.hip) ---- flags / h_flags: BFL_STRIDE ints per instance (pgf_batch.h)
  struct {
    int *flags = nullptr, *h_flags = nullptr;
    double *diff = nullptr, *norm = nullptr, *h_diff = nullptr, *h_norm = nullptr;
    double *red4 = nullptr, *meas = nullptr, *h_meas = nullptr;
  } out;

  // ---- the condensed order (pgf_api_batch.hip) ----
  // (constraint block eliminated first, as condensed_wanted for one instance):
  // ok = the panels exist and the batch runs one of the chain schedules; wanted = the
  // growth bound holds for every instance's delta (decided per outer step on the host: the
  // device-resident controller, which moves lambda on the device, keeps the natural order);
  // last = how the factors the instances hold were made; free = the next step
  // refactorises every instance anyway and may choose
  struct {
    bool ok = false, wanted = false, last = false, free = true;
    int mp = 0;
  } cond;

  // ---- the device-resident step controller (pgf_api_batch_ctl.hip) ----
  // per-instance state, constants, and a log of (lambda used, lambda next, accepted) per outer
  // iteration and instance
  struct {
    double *cs = nullptr, *cp = nullptr, *log = nullptr;
    int log_cap = 0, logged = 0;
  } dctl;

  // ---- a banded batch (pgf_api_band_batch.hip; ctl, refine and what follows each:
  // pgf_api_batch_ctl.hip) ----
  // Banded handles of one pattern, all narrow or all wide.  tab / htab: the instances' BandInst
  // records beside the BInst ones; sh: what they share; stat / h_stat: ONE status block for the whole
  // batch, band_stat_stride(sh) doubles per instance (residual pairs, partial sums of the step
  // update, pivot flags) and its pinned mirror, read with one copy per step; frozen / last_neg: the
  // host's view of pgf_batch_set_frozen and of the inertia last reported.
  struct {
    bool on = false;
    BandInst *tab = nullptr;
    std::vector<BandInst> htab;
    BandShape sh{};
    double *stat = nullptr, *h_stat = nullptr;
    std::vector<uint8_t> frozen;
    std::vector<int> last_neg;
    // wide route: per instance (reductions, solve phases) counted on the device
    // (pgf_batch_debug_band_wide_stats)
    int *wcnt = nullptr;
    // bordered narrow route: per instance (factor phases, solve phases) counted on the device
    // (pgf_batch_debug_border_stats)
    int *bcnt = nullptr;
    // created with PGF_BATCH_BAND_CTL: the device-resident controller is open to this band batch.
    // out.flags / out.diff are allocated as for a dense batch and written by kbb_step_final;
    // guard: per instance (guard on, refine_tol) as pgf_batch_ctl_init found them on the handles;
    // rejects: per instance, steps the loop rejected for a pivot / by the guard
    bool ctl = false;
    double *guard = nullptr;
    int *rejects = nullptr;
    // created with PGF_BATCH_CTL_REFINE besides: guard has a third double per instance
    // (refine_fail), and every banded step of the loop enqueues two refinement rounds on rtab -- tab
    // over again, except that ctl points at the instance's refinement words in rctl ([0] stays 0: no
    // assembly, kept factors, no write of ctl[1]; [1] a round ran in this step; [2] the step missed
    // refine_tol as it came out of the solve; [3] sits this round out) -- rrel: the measure the next
    // round has to beat; rcnt: per instance (steps refined, rounds run)
    bool refine = false;
    BandInst *rtab = nullptr;
    int *rctl = nullptr, *rcnt = nullptr;
    double *rrel = nullptr;
  } band;

  // ---- the Globalized policy (pgf_api_batch_line_search.hip; created with PGF_BATCH_LINE_SEARCH) ----
  // otab / obtab: tab / band.tab over again, except that (x, y, g, c) name the instance's OUTER point
  // (xhat, yhat and its handle's ls.ghat, ls.chat) -- the step's residual, right-hand side and
  // update run on them; itab / ibtab (dense / band): (x, y, c, g, q, b) name (dx, dy, u, v, 0, 0),
  // so that the batch's evaluation launches form the direction's images; ltab: what the ladder and
  // the finish read; blk / h_blk: LSB_STRIDE doubles per instance and the pinned mirror; red: the
  // instances' partial-sum slices; guard / h_guard: (guard on, refine_tol) per instance of a band
  // batch, as the handles have them when the step is enqueued.  hat_fresh: g, c at the outer points
  // are current for the outer step; pending: the step in flight carries the bit.
  struct {
    bool on = false;
    double newton_tol = 1e-8;
    BInst *otab = nullptr, *itab = nullptr;
    BandInst *obtab = nullptr, *ibtab = nullptr;
    LsInst *ltab = nullptr;
    double *blk = nullptr, *h_blk = nullptr, *red = nullptr, *guard = nullptr, *h_guard = nullptr;
    bool hat_fresh = false, pending = false, have_stats = false;
    int stage_launches = 0, host_waits = 0;  // pgf_batch_debug_line_search_stats
  } ls;

  // ---- counters and hooks read or set only by pgf_api_batch_read.hip ----
  struct {
    int repaired = 0;  // instances whose step the host-side guard repaired (pgf_batch_refinement_stats)
    int inject_helper_failure = 0;  // test hook: instance 0's next factorisation reports failed helpers
    int band_reductions = 0, band_assemblies = 0;  // pgf_batch_debug_band_stats
    // steps enqueued without inversion launches (wide route) / without factor-phase launches
    // (bordered): pgf_batch_debug_band_wide_stats
    int band_lean = 0;
  } dbg;
};

static inline int bfail(pgf_batch b, int code, const char *msg) {
  if (b) b->err = msg;
  return code;
}

#define BHIPCHK(b, expr)                                                 \
  do {                                                                   \
    hipError_t e_ = (expr);                                              \
    if (e_ != hipSuccess) {                                              \
      (b)->err = std::string(#expr) + ": " + hipGetErrorString(e_);      \
      return PGF_HIP_ERROR + (int)e_;                                    \
    }                                                                    \
  } while (0)

// doubles per instance of a band batch's status block: the handle's own stride
static inline size_t band_stat_stride(const BandShape &sh) { return band_stat_stride(sh.nred); }

// a handle's host-side view of its outer step: lambda and what a step derives from it and rho
static inline void set_outer_scalars(pgf_handle h, double dt, double rho) {
  h->dt = dt;
  h->lamb = 1.0 / dt;
  h->rho = rho;
  h->fact = 1.0 / (1.0 + h->lamb * rho);
  h->delta = h->lamb / (1.0 + h->lamb * rho);
}

#pragma GCC visibility push(hidden)
// ---- pgf_api_batch.hip, for every file of the batch ----------------------------------------------
// One allocation of the batch: count elements, device memory or (BA_PINNED) pinned host memory,
// zeroed with BA_ZERO; pgf_batch_destroy frees it.  A create is a list of these behind one
// hipError_t: a call is a no-op once *e holds an error, so the list has a single failure exit.
enum { BA_DEVICE = 0, BA_PINNED = 1, BA_ZERO = 2 };
void batch_alloc_bytes(pgf_batch b, hipError_t *e, void **p, size_t bytes, unsigned kind);
template <typename T>
static inline void batch_alloc(pgf_batch b, hipError_t *e, T **p, size_t count, unsigned kind = BA_DEVICE) {
  batch_alloc_bytes(b, e, (void **)p, count * sizeof(T), kind);
}
// a device copy of the host table src with rename(entry, i) applied to every entry (band.rtab and
// the line search's tables)
template <typename T, typename F>
static inline void batch_renamed_table(pgf_batch b, hipError_t *e, T **dst, const std::vector<T> &src, F rename) {
  std::vector<T> t(src);
  for (size_t i = 0; i < t.size(); ++i) rename(t[i], i);
  batch_alloc(b, e, dst, t.size());
  if (*e == hipSuccess) *e = hipMemcpy(*dst, t.data(), t.size() * sizeof(T), hipMemcpyHostToDevice);
}
// What both creates ask of every handle, in two parts: the kind's own checks go between them.  0, or
// the refusal's code with its text in *msg.
int batch_check_shape(pgf_handle h, pgf_handle h0, const char **msg);   // pgf_batch_create_ex, band_batch_create
int batch_check_state(pgf_handle h, bool band, const char **msg);       // pgf_batch_create_ex, band_batch_create
// the new batch's scalars from its first handle, and its stream
hipError_t batch_begin(pgf_batch b, const pgf_handle *handles, int count);  // pgf_batch_create_ex, band_batch_create
// the vector part of instance i's records from its handle and its batch slots (the dense create
// adds the matrices and the factor's arrays; band_inst_of has filled the band's own)
void batch_fill_vectors(pgf_batch b, int i, BInst &t);     // pgf_batch_create_ex, band_batch_create
void batch_fill_vectors(pgf_batch b, int i, BandInst &u);  // band_batch_create
// the batch owns the device-side state of the handle from here on
void batch_own_handle(pgf_handle h);                        // pgf_batch_create_ex, band_batch_create
void batch_eval(pgf_batch b);  // band_batch_enqueue_step, band_batch_step_async, pgf_batch_ctl_iterate, the read-outs
// everything of one dense Newton step, enqueued
void batch_enqueue_step(pgf_batch b, unsigned policy, double tau, bool host_knows_factored);  // ctl_enqueue_step
// behind the step's wait: whether the step carried PGF_STEP_LINE_SEARCH, its counters settled
bool batch_ls_begin_sync(pgf_batch b);                      // pgf_batch_sync, band_batch_sync
// a chain helper or a chained solve failed its hand-over: both go off for the process, the
// publication halves of instance i (i < 0: of every instance) get their sentinels back, and the
// sticky word behind out.flags is cleared -- all enqueued on the batch's stream
hipError_t batch_chain_off(pgf_batch b, int i);             // pgf_batch_sync, pgf_batch_ctl_read
// ---- pgf_api_batch_read.hip ----
// two ints per instance, counted on the device in pairs (null: zeros), split into the two outputs
int batch_read_pairs(pgf_batch b, const int *pairs, int *first, int *second);  // the pgf_batch_debug_*_stats of both files

// ---- the banded half (pgf_api_band_batch.hip), each beside the entry point that hands over to it
// in one line ----
int band_batch_create(const pgf_handle *handles, int count, unsigned flags, pgf_batch *out);  // pgf_batch_create_ex
void band_batch_eval(pgf_batch b);                                            // batch_eval
int band_batch_step_async(pgf_batch b, unsigned policy, double tau);          // pgf_batch_step_async
int band_batch_sync(pgf_batch b, int *status, int *n_neg, double *diff);      // pgf_batch_sync
// the launches of one banded step, without the evaluation made ahead and the status copy;
// lean_allowed: the caller knows that every instance still live holds a clean factor of its band
void band_batch_enqueue_step(pgf_batch b, unsigned policy, double tau, bool lean_allowed);  // ctl_enqueue_step
void band_batch_measures_eval(pgf_batch b);                                   // pgf_batch_measures
// ---- the Globalized policy on a batch (pgf_api_batch_line_search.hip) -----------------------------
int batch_ls_attach(pgf_batch b);                       // pgf_batch_create_ex
// g, c at every instance's outer point, once per outer step (behind the evaluation at the current
// points and in front of the mask, as ls_enter orders them on the handle)
void batch_ls_eval_outer(pgf_batch b);                  // batch_enqueue_step, band_batch_enqueue_step
// behind the step update: the images, the ladder, the finish, and the copy of the blocks
int batch_ls_enqueue_stage(pgf_batch b);                // pgf_batch_step_async, band_batch_step_async
// An instance the guard repairs on its handle: the handle's (x, y, g, c) name its outer point's
// vectors for the repair's step update (enter / ls_leave); then ls_search on the handle, whose block
// becomes the instance's.  PGF_OK, PGF_LINE_SEARCH, or an error.
void batch_ls_handle_enter(pgf_batch b, int i);         // batch_repair_instance, band_batch_repair
int batch_ls_handle_search(pgf_batch b, int i, double *diff);
// after the step's wait: the instance's status and step length from its block
void batch_ls_report(pgf_batch b, int i, int *status, double *diff);  // pgf_batch_sync, band_batch_sync
#pragma GCC visibility pop
// what it takes from pgf_api_band.hip, the guard's measure over nred residual pairs, and from
// pgf_api_band_setup.hip the hash
// of a pattern as pgf_sparse_set_pattern receives it (kept in SparseDev::pat.hash)
double band_residual_rel_of(const double *pairs, int nred);
