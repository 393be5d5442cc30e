/*
 * pgf_hip.h -- C ABI of the MI355X-native semi-smooth Newton / KKT step.
 *
 * Drop-in boundary for ONE hot path of chrhansk/pygradflow (v0.5.24): everything
 * executed inside one NewtonMethod.step(iterate) with the default
 * StepSolverType.Symmetric.  Plain C: opaque handles,
 * raw pointers + sizes, int status returns, no callbacks, no exceptions.
 *
 * Each entry point cites the reference interface (file:line, relative to the
 * pygradflow checkout) whose arithmetic it replaces.  INTEGRATION.md shows the
 * ctypes stub a pygradflow maintainer would add.
 *
 * Conventions
 *   - all floating point is IEEE binary64 (Params.dtype, params.py:275-277);
 *   - masks are one byte per variable, 0 / 1 (numpy bool_);
 *   - `loc` says where an input pointer lives: PGF_HOST or PGF_DEVICE;
 *     outputs are host pointers unless the name says `_dev`;
 *   - one caller thread per handle; one HIP stream per handle;
 *   - caller owns every host buffer, the library owns every device buffer.
 *
 * Status codes (mapped by the Python shim):
 *   0 ok | 1 singular / zero pivot -> LinearSolverError
 *   2 inertia mismatch -> LinearSolverError | 3 invalid argument -> ValueError
 *   4 called out of order -> RuntimeError | >=100 HIP runtime error -> RuntimeError
 */
#ifndef PGF_HIP_H
#define PGF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PGF_OK 0
#define PGF_SINGULAR 1
#define PGF_INERTIA 2
#define PGF_INVALID 3
#define PGF_NOT_READY 4
/* PGF_STEP_LINE_SEARCH: none of the 30 trial step lengths was accepted (newton.py:291-292, the
 * reference's bare Exception("Line search failed to converge")); the device point has not moved */
#define PGF_LINE_SEARCH 5
#define PGF_HIP_ERROR 100

#define PGF_HOST 0
#define PGF_DEVICE 1

/* pgf_create flags */
#define PGF_CREATE_SPARSE 1u /* banded mode: CSR derivatives, no dense N x N storage */

/* pgf_qp_step policy bits (NewtonMethod policies, newton.py:35-60, 63-89, 181-215) */
#define PGF_STEP_RECOMPUTE_MASK 1u  /* Full, ActiveSet: mask from the current point  */
#define PGF_STEP_REFACTOR 2u        /* Full: assemble + factor every step             */
#define PGF_STEP_REFACTOR_ON_CHANGE 4u /* ActiveSet: refactor iff the mask changed     */
/* Globalized (GlobalizedNewtonMethod, newton.py:218-304): with PGF_STEP_RECOMPUTE_MASK |
 * PGF_STEP_REFACTOR only, on a dense Symmetric or a banded handle (anything else: PGF_INVALID).
 * The Newton direction is solved at the OUTER point with the device point's mask (:244-248), then
 * the Armijo line search on 1/2 ||F||^2 over alpha = 2^-k, k < 30 (:250-292), runs in one launch;
 * the new point is measured from the outer point (:296).  pgf_qp_sync waits twice, whatever the
 * number of trials; PGF_LINE_SEARCH when no trial is accepted. */
#define PGF_STEP_LINE_SEARCH 8u

typedef struct pgf_solver *pgf_handle;
typedef struct pgf_linsolver *pgf_ls_handle;

/* ---- library ---------------------------------------------------------- */
int pgf_version(void);
int pgf_device_count(int *count);
/* static description of the last error on this handle (never NULL) */
const char *pgf_last_error(pgf_handle h);

/* ---- step-solver handle: one per (n, m); reusable across outer steps --- */
/* replaces SymmetricStepSolver.__init__ (step/solver/symmetric_step_solver.py:14-25,
 * scaled_step_solver.py:16-33) -- allocation only */
int pgf_create(int n, int m, int device, unsigned flags, pgf_handle *out);
int pgf_destroy(pgf_handle h);

/* Problem.var_lb / var_ub (problem.py:57-62); +-inf allowed */
int pgf_set_bounds(pgf_handle h, const double *lb, const double *ub);

/* one outer step: x^, y^, dt, rho.  Pre-scales the bounds lamb*lb, lamb*ub
 * (ScaledImplicitFunc.__init__, implicit_func.py:211-216); drops mask, K, factor */
int pgf_set_outer(pgf_handle h, const double *xhat, const double *yhat, double dt, double rho);

/* ScaledStepSolver.update_derivs (scaled_step_solver.py:76-79,
 * symmetric_step_solver.py:41-43): H = lag_hess(x, y) (no rho J'J), J = cons_jac.
 * Dense row-major; only the lower triangle of H is read.  PGF_HOST pointers are
 * copied to HBM; PGF_DEVICE pointers are adopted (caller keeps them alive).
 * Invalidates K and its factor. */
int pgf_set_derivs_dense(pgf_handle h, const double *H, int64_t ldh, const double *J,
                         int64_t ldj, int loc);
/* The same matrices as scipy CSR (what Iterate.aug_lag_deriv_xx / _xy return,
 * iterate.py:99-110): host arrays, int32 indices, duplicates are summed.  Only the
 * non-zeros cross PCIe; the dense H, J the factorisation reads are rebuilt on the device.
 * For problems whose derivatives are sparse but not banded (the banded path has its own
 * entry points below). */
int pgf_set_derivs_csr(pgf_handle h, const int *Hptr, const int *Hidx, const double *Hval,
                       const int *Jptr, const int *Jidx, const double *Jval);

/* StepFunc.compute_active_set (implicit_func.py:72-74) =
 * projection_initial (:233-246, tau = NaN means None) + compute_active_set_box (:21-44).
 * x, g: current point and g = aug_lag_deriv_x(rho) (iterate.py:91-94). mask_out[n]. */
int pgf_active_set(pgf_handle h, const double *x, const double *g, double tau,
                   uint8_t *mask_out);

/* ScaledStepSolver.update_active_set (scaled_step_solver.py:81-83) */
int pgf_set_active_set(pgf_handle h, const uint8_t *mask);

/* SymmetricStepSolver._compute_deriv (:49-77) + linear_solver()/LUSolver.__init__
 * (:129-133, linear_solver/lu_solver.py:9-17): gather-assemble the reduced KKT matrix
 * for the current mask in HBM and factor it (LDL^T, K symmetric quasi-definite).
 * n_neg = number of negative pivots = LinearSolver.num_neg_eigvals().
 * Returns PGF_SINGULAR on a zero / non-finite pivot. */
int pgf_factor(pgf_handle h, int *n_neg);

/* ScaledStepSolver.solve (scaled_step_solver.py:85-107) for the current mask/factor:
 * residual (implicit_func.py:219-231), rhs split (:38-60), reduced rhs
 * (symmetric_step_solver.py:79-94), solve (:135-158), scatter (:115-121),
 * dy (:104), StepResult clipping and diff (step_solver.py:16-63).
 * c may be NULL when m == 0.  Factors first if needed (status as pgf_factor).
 * inertia_check != 0 and n_neg != m  ->  PGF_INERTIA (:146-153). */
int pgf_newton_solve(pgf_handle h, const double *x, const double *y, const double *g,
                     const double *c, int inertia_check, double *dx, double *dy,
                     double *xn, double *yn, double *diff);

/* ScaledImplicitFunc.value_at (implicit_func.py:219-231); mask NULL = recompute at p */
int pgf_residual(pgf_handle h, const double *x, const double *y, const double *g,
                 const double *c, const uint8_t *mask, double *F_out);

/* LinearSolver.solve(rhs, trans) (linear_solver/linear_solver.py:23-25) against the
 * current reduced KKT factor; rhs/sol have |I| + m entries */
int pgf_linear_solve(pgf_handle h, const double *rhs, int trans, double *sol);
/* nrhs right-hand sides against the same factor: column j at rhs + j * ld, its solution at
 * sol + j * ld (ld >= the system's size).  A wide band (B = 16, 32, 64) without a border and with the
 * factor / solve split on solves them as panels of at most 64 columns against the kept factors
 * (one factor-only reduction when there are none), checks every column's residual and solves a
 * column above the refinement tolerance again through pgf_linear_solve; every other handle loops
 * over pgf_linear_solve.  (LUSolver.solve with a 2-D right-hand side.) */
int pgf_linear_solve_multi(pgf_handle h, const double *rhs, int nrhs, int64_t ld, int trans,
                           double *sol);

/* size of the reduced system of the current mask: |I|, |I| + m */
int pgf_reduced_dims(pgf_handle h, int *n_inactive, int *n_reduced);
/* copy the assembled (pre-factor) lower triangle of K to host, row-major N x N
 * (debug / parity; re-assembles, does not disturb the factor) */
int pgf_get_kkt(pgf_handle h, double *K_out, int64_t ldk);

/* ---- sparse (banded) mode: handle created with PGF_CREATE_SPARSE --------------------- */
/* Fixed sparsity pattern of H (n x n CSR, both triangles) and J (m x n CSR) and the band
 * plan computed on the host (pygradflow_amd/sparse.py): pos[i] = row of variable i /
 * constraint n + r in the permuted banded KKT matrix, bw = half bandwidth, H/J slot =
 * linear index into the band array for each stored entry (H: -1 for the mirrored upper
 * duplicates), JT* = column-ordered copy of J's pattern (JTmap indexes Jval).  Replaces the
 * scipy fancy-slicing / bmat assembly of symmetric_step_solver.py:27-39, 49-77 for sparse
 * problems; active variables become identity rows instead of being sliced out. */
int pgf_sparse_set_pattern(pgf_handle h, int bw, const int *pos, int nnzH, const int *Hptr,
                           const int *Hrow, const int *Hcol, const int *Hslot, int nnzJ,
                           const int *Jptr, const int *Jcol, const int *Jslot, const int *JTptr,
                           const int *JTrow, const int *JTmap);
/* block size of the banded solve, after pgf_sparse_set_pattern (which selects B = 0):
 *   B = 0: automatic -- bw <= 8: 8 x 8 block cyclic reduction; bw 9 .. 64: block cyclic
 *          reduction with the smallest B in {16, 32, 64} >= bw (so 16 for bw 9 .. 10).  Every
 *          automatic route carries the accuracy guard;
 *   B = 8, 16, 32, 64: that block size (PGF_INVALID if B < bw).
 * Invalidates the factorisation; the work arrays are sized for the chosen B. */
int pgf_sparse_set_block_size(pgf_handle h, int B);
/* Factor / solve split of the wide block cyclic reduction (B = 16, 32, 64, no border): on (the
 * default; PGF_BW_SPLIT=0 in the environment makes off the default of new handles), the first
 * solve on a matrix runs the fused reduction and keeps its forward multipliers (2 B^2 doubles per
 * block more), and every further solve on the same matrix -- a back-solve step, a refinement
 * correction, pgf_linear_solve -- runs the solve phase against them without any inversion; off,
 * every solve runs the whole reduction and the multiplier store is not allocated.  The results
 * are the same bit for bit.  Drops the kept factors. */
int pgf_sparse_set_factor_split(pgf_handle h, int on);
/* Bordered band, after pgf_sparse_set_pattern (which declares none): the last k positions of
 * `pos` are border nodes -- dense rows / columns of the KKT pattern, variables or constraints --
 * and bw, the band slots and the block size describe the remaining n + m - k rows only.  With
 * kp = k rounded up to a multiple of 16, an entry between band row i and border node j has slot
 * (n + m - k + 1) * ldb + i * kp + j, one between border nodes a >= b the slot behind those,
 * + (n + m - k) * kp + a * kp + b (ldb = bw + 1 rounded up to even; pygradflow_amd/sparse.py).
 * The band is eliminated first: Y = inv(B) C and the L D L' of S = D - C' Y are formed once per
 * assembled matrix and kept while the factor is valid; a solve is one banded reduction plus the
 * border kernels (csrc/pgf_border.hip).  k = 0 removes the border.  PGF_INVALID for k > 64 and
 * for dense handles.  With PGF_BORDER_MULTI=0 in the environment Y is formed by k single
 * banded solves also at block size 8 (the only route at 16, 32, 64). */
int pgf_sparse_set_border(pgf_handle h, int k);
/* Large border: 65 <= k <= 1024 border nodes, after pgf_sparse_set_pattern, on a banded handle whose
 * remainder runs the wide route -- block size 16, 32 or 64 (pgf_sparse_set_block_size) with the
 * factor / solve split on.  The store is that of pgf_sparse_set_border with kp = k rounded up to a
 * multiple of 64.  Per assembled matrix: B is factorised once (the kept factors of the wide
 * reduction), Y = inv(B) C is one panel solve whose launches carry kp / 64 column slices, C' Y is
 * formed on the FP64 matrix pipes in 64 x 64 tiles over row chunks whose partial sums are added in
 * chunk order, and S = D - C' Y is factorised by a dense L D L' of size kp whose status the factor
 * phase awaits; a solve phase adds no host wait (csrc/pgf_border_large.hip).  Steps, line search,
 * pgf_linear_solve(_multi), the accuracy guard and the measures run as on any bordered handle.
 * PGF_INVALID: k outside 65..1024, a dense handle, block size 8, the split off; afterwards
 * pgf_sparse_set_factor_split(h, 0) and a change to block size 8 are PGF_INVALID, and
 * pgf_batch_create refuses the handle ("batch: a large border ...").  pgf_sparse_set_border(h, 0)
 * removes the border.  PGF_BORDER_MULTI=0 forms Y by k single solves, as above. */
int pgf_sparse_set_border_large(pgf_handle h, int k);
/* values of H = lag_hess(x, y) and J = cons_jac(x) in pattern order (update_derivs) */
int pgf_sparse_set_values(pgf_handle h, const double *Hval, const double *Jval);
/* q and b of a linear-quadratic problem whose Q, A were given through the sparse pattern */
int pgf_qp_set_vectors(pgf_handle h, const double *q, const double *b);

/* ---- device-resident linear-quadratic mode (bench, batched mode) -------- */
/* f = 1/2 x'Qx + q'x, c = Ax - b: H = Q and J = A stay in HBM; g and c are
 * evaluated on device (SURVEY.md 8d "Problem data device-resident"). */
int pgf_qp_set_problem(pgf_handle h, const double *Q, int64_t ldq, const double *q,
                       const double *A, int64_t lda, const double *b, int loc);
int pgf_qp_set_point(pgf_handle h, const double *x, const double *y);
int pgf_qp_get_point(pgf_handle h, double *x, double *y);
int pgf_qp_get_mask(pgf_handle h, uint8_t *mask);
/* mask <- compute_active_set at the device point (SimplifiedNewtonMethod.__init__,
 * newton.py:52-56: call once at (x^, y^)); *changed = 1 if the stored mask was replaced */
int pgf_qp_update_active_set(pgf_handle h, double tau, int *changed);
/* new outer step at the current device point: (x^, y^) <- (x, y) on device, then as
 * pgf_set_outer (what Solver.solve does between accepted steps, solver.py:357-378) */
int pgf_qp_advance_outer(pgf_handle h, double dt, double rho);
/* One NewtonMethod.step on the device-resident point (policy bits above; tau NaN = None).
 * (x, y) <- (xn, yn).  n_neg / diff may be NULL.  One host sync at the end
 * (plus one to read |I| when the mask is recomputed). */
int pgf_qp_step(pgf_handle h, unsigned policy, double tau, int inertia_check, int *n_neg,
                double *diff);
/* enqueue-only variant for timing loops: no host sync, status checked by pgf_qp_sync */
int pgf_qp_step_async(pgf_handle h, unsigned policy, double tau);
int pgf_qp_sync(pgf_handle h, int *n_neg, double *diff);
/* The line search of steps with PGF_STEP_LINE_SEARCH.  newton_tol: Params.newton_tol (params.py,
 * default 1e-8, the handle's default too): a merit at or below it ends the search (newton.py:254,
 * 281).  pgf_qp_line_search_stats: the last such step's accepted alpha (1 without a trial), the
 * number of trials evaluated (0: merit0 <= newton_tol, newton.py:254-255; 30 on PGF_LINE_SEARCH),
 * merit0 = 1/2 ||F(x, y)||^2 (:251-252), the slope F . dF d (:260-268) and all 30 trial merits of
 * the ladder (:273-279; trial_merits may be NULL, as any other pointer).  PGF_NOT_READY before the
 * first such step. */
int pgf_qp_set_line_search(pgf_handle h, double newton_tol);
/* (dx, dy) as the last settled step's update left them (dx rewritten where x - dx was clipped,
 * step_solver.py:25-48).  After a step with PGF_STEP_LINE_SEARCH: the FULL direction, measured from
 * the outer point (newton.py:248), which the search scaled by alpha.  Either pointer may be NULL. */
int pgf_qp_get_direction(pgf_handle h, double *dx, double *dy);
int pgf_qp_line_search_stats(pgf_handle h, double *alpha, int *trials, double *merit0, double *slope,
                             double *trial_merits);
/* ||F(z)||_2 of the UNSCALED residual (ImplicitFunc.value_at, implicit_func.py:150-161)
 * at the device point; host result, and optionally a device slot (RCCL all-gather input) */
int pgf_qp_residual_norm(pgf_handle h, double *norm_out, double *norm_out_dev);
/* Termination measures of the device point: out[0] = stat_res
 * (iterate.py:174-177, with bounds_dual :140-152 and the ActiveSet of active_set.py:4-29 at
 * tolerance active_tol), out[1] = cons_violation (:166-171), out[2] = bound_violation
 * (:155-163), out[3] = ||y||_inf (DualNormUpdate, penalty.py:60-74). */
int pgf_qp_measures(pgf_handle h, double active_tol, double *out);
/* HIP stream of the handle (void* = hipStream_t) for event timing by the caller */
int pgf_stream(pgf_handle h, void **stream_out);
/* device time (ms) spent in the factor's trailing-update launches since the last call,
 * their count and algorithmic flops -- measured with HIP events on the handle's stream */
int pgf_profile_enable(pgf_handle h, int on);
int pgf_profile_read(pgf_handle h, double *update_ms, int64_t *update_launches,
                     double *update_flops, double *factor_ms);
/* the same and more, as one array (count >= PGF_PROF_COUNT).  While profiling is enabled the
 * dense factorisation runs its kernels as separate launches (the production schedule fuses
 * the diagonal chain with the trailing update in one launch) so that each can be timed:
 * update (k_ldlt_update) ms / launches / algorithmic flops / algorithmic bytes, whole
 * factorisation ms, diagonal chain (k_diag_chain) ms / launches, TRSM below the diagonal
 * block (k_trsm_block) ms, diagonal-block update (k_update_diag) ms */
#define PGF_PROF_UPDATE_MS 0
#define PGF_PROF_UPDATE_LAUNCHES 1
#define PGF_PROF_UPDATE_FLOPS 2
#define PGF_PROF_UPDATE_BYTES 3
#define PGF_PROF_FACTOR_MS 4
#define PGF_PROF_CHAIN_MS 5
#define PGF_PROF_CHAIN_LAUNCHES 6
#define PGF_PROF_TRSM_MS 7
#define PGF_PROF_UDIAG_MS 8
#define PGF_PROF_COUNT 9
/* pgf_profile_enable(h, 2): the PRODUCTION launches are timed instead, one HIP-event span per
 * launch: k_chain_update (the diagonal chain beside the trailing-update tiles; flops / bytes =
 * the algorithmic work of its update jobs) and k_trsm_ud (T(k) with the next diagonal block's
 * update); read with count >= PGF_PROF_COUNT2 */
#define PGF_PROF_FUSED_MS 9
#define PGF_PROF_FUSED_LAUNCHES 10
#define PGF_PROF_FUSED_FLOPS 11
#define PGF_PROF_FUSED_BYTES 12
#define PGF_PROF_TRSMUD_MS 13
#define PGF_PROF_COUNT2 14
/* the assembly launches of the unsymmetric formulations (pgf_set_formulation) while profiling is
 * enabled (any mode): device ms and launches; read with count >= PGF_PROF_COUNT3 */
#define PGF_PROF_UNSYM_ASM_MS 14
#define PGF_PROF_UNSYM_ASM_LAUNCHES 15
#define PGF_PROF_COUNT3 16
int pgf_profile_read_ex(pgf_handle h, double *out, int count);

/* ---- batched mode: many device-resident instances advanced by ONE launch sequence ---- */
/* The reference's only parallelism is a process pool over independent instances
 * (runners/runner.py:107-153); BASELINE configs[3] is 256 instances of (n=1024, m=256).
 * A batch groups existing dense linear-quadratic handles of identical (n, m) on one
 * device (each set up through pgf_set_bounds / pgf_qp_set_problem / pgf_qp_set_point);
 * every kernel of the Newton step then runs over all instances at once (instance =
 * blockIdx.z, reduced sizes read on the device: no host round trip inside a step).
 * While a handle belongs to a batch, drive it only through the batch.
 *
 * A BAND batch: every handle banded (PGF_CREATE_SPARSE) on the narrow route -- half-bandwidth
 * <= 8, block size 8, no border (unless created with PGF_BATCH_BORDER, below) -- with pattern and values set, the same n, m and device, and ONE
 * sparsity pattern (the 64-bit hash of what pgf_sparse_set_pattern received, bw, the band's row
 * stride and the entry counts are compared).  Values of H and J, q, b, bounds, points, dt and rho
 * are the instance's own.  Every banded kernel of the step then runs over all instances at once
 * (instance = blockIdx.y), with one host synchronisation per step and one status copy for the
 * batch; an instance whose solve misses refine_tol is refined on its own handle
 * (pgf_batch_refinement_stats counts it), and only one that cannot be repaired or met a zero
 * pivot reports PGF_SINGULAR, its point unchanged.  Refused with PGF_INVALID and a message that
 * names the reason: dense and banded handles mixed, different patterns, a wide band (block size
 * above 8) or a border without its flag, an unsymmetric formulation.  On a band batch pgf_batch_ctl_* (unless it was
 * created with PGF_BATCH_BAND_CTL, below) and pgf_batch_debug_fail_next_helper return PGF_INVALID
 * and pgf_batch_debug_factor_kind 0.
 *
 * pgf_batch_create_ex takes flags; pgf_batch_create is pgf_batch_create_ex with flags 0, and unknown
 * flag bits are PGF_INVALID.  PGF_BATCH_WIDE_BAND also admits a band batch on the WIDE route:
 * every handle with block size 16, 32 or 64 (half-bandwidths up to 64), under the conditions above
 * and, in addition, ONE block size and ONE setting of the factor / solve split
 * (pgf_sparse_set_factor_split) -- refused otherwise with "batch: banded instances must share the
 * block size and the factor / solve split".  With the split on, each instance decides on the device
 * whether its step reduces (its matrix changed, or its last reduction met a bad pivot) or runs the
 * solve phase against the factors it kept, inside the one launch sequence of the batch; an
 * instance above refine_tol is refined on its handle by solve phases against those factors.  The
 * results are, bit for bit, those of the single handles.  Narrow and dense batches behave with the
 * flag as without it.
 *
 * PGF_BATCH_BAND_CTL (alone or with PGF_BATCH_WIDE_BAND) opens the device-resident controller
 * pgf_batch_ctl_* to a band batch, narrow or wide; without it they return PGF_INVALID as said above,
 * and on a dense batch the flag changes nothing.  Inside pgf_batch_ctl_iterate the banded step is
 * finished per instance on the device (kernel kbb_step_final): step length, pivot flag, and the
 * guard's measure against the refine_tol the instance's handle had at pgf_batch_ctl_init (never
 * when its refine_mode is off).  An instance above its tolerance cannot be refined on its handle
 * inside a loop without host round trips: without PGF_BATCH_CTL_REFINE (below, which refines it on
 * the device) its step counts as FAILED, the controller rejects it with
 * 2 lambda and the instance goes back to its outer point at the next iteration -- the reference's
 * own recovery, a larger lambda makes K quasi-definite again (step_control.py:80-107).
 * pgf_batch_debug_ctl_stats counts such steps.  pgf_batch_ctl_read brings the device's frozen
 * flags to the host, so that a pgf_batch_step_async behind it reports the instances the last
 * iteration froze as frozen (status PGF_OK, diff 0) until the next pgf_batch_advance_outer*.
 *
 * PGF_BATCH_BORDER admits BORDERED instances on the narrow route: a band of half-bandwidth <= 8
 * (block size 8) plus 1 <= k <= 64 border nodes (pgf_sparse_set_border), under the conditions above
 * and, in addition, ONE border size k for every handle -- refused otherwise with "batch: banded
 * instances must share the border size".  Each instance decides on the device whether its step
 * runs the factor phase (clear and assembly of band, C and D, Y = inv(B) C by the panel reduction,
 * S = D - C' Y and its factor): where its matrix changed or its last factor phase met a bad pivot
 * in B or S, which is where the single handle factors.  Every live instance runs the solve phase
 * every step, and a step behind a good one whose policy keeps the mask is enqueued without any
 * factor-phase launch.  An instance above refine_tol is refined on its handle by solve phases
 * against the Y and the factor of S the batch left there.  The results are, bit for bit, those of
 * the single handles on their panel route (PGF_BORDER_MULTI=0, the column-by-column cross-check,
 * stays a single-handle switch: under it the two are not bit-comparable).
 * pgf_batch_debug_border_stats counts the phases per instance.  Refused under these flags: a border
 * on a wide remainder, with or without PGF_BATCH_WIDE_BAND ("batch: a bordered band joins a device
 * batch on the narrow route only (block size 8)"; PGF_BATCH_WIDE_BORDER, below, admits it), and
 * PGF_BATCH_BORDER | PGF_BATCH_BAND_CTL without PGF_BATCH_BORDER_CTL (below) on handles that have a
 * border ("batch: the device-resident controller does not drive a bordered band batch").  Handles
 * without a border behave with the flag as without it.
 *
 * PGF_BATCH_WIDE_BORDER, valid only as PGF_BATCH_BORDER | PGF_BATCH_WIDE_BAND | PGF_BATCH_WIDE_BORDER
 * (the bit without both of the others is PGF_INVALID), admits BORDERED instances whose remainder
 * is on the WIDE route: block size 16, 32 or 64, ONE block size and ONE border size 1 <= k <= 64,
 * and the factor / solve split in force on every handle (refused otherwise with "batch: a bordered
 * wide band needs the factor / solve split").  The factor phase of an instance whose matrix
 * changed: assembly, B factorised once by the factor-only reduction that keeps its multipliers,
 * Y = inv(B) C as one panel solve against them on the FP64 matrix pipes, S and its factor.  The
 * solve phase of every live instance, every step: v = inv(B) r_a against the kept factors, then the
 * border part as on the narrow route.  Driven by pgf_batch_step_async / pgf_batch_sync; the results
 * are, bit for bit, those of the single handles (PGF_BORDER_MULTI=0 stays a single-handle switch:
 * the batch always takes the panel route).  pgf_batch_debug_border_stats counts the phases, and
 * pgf_batch_debug_band_wide_stats the factor-only reductions and kept-factor solve phases of B,
 * which equal them.  A border under PGF_BATCH_BAND_CTL without PGF_BATCH_BORDER_CTL stays refused as
 * above.  Narrow bordered instances and instances without a border behave with the bit as under the
 * other two alone.
 *
 * PGF_BATCH_BORDER_CTL, valid only together with PGF_BATCH_BORDER | PGF_BATCH_BAND_CTL (the bit
 * without both is PGF_INVALID before any handle is read; on a wide remainder PGF_BATCH_WIDE_BAND |
 * PGF_BATCH_WIDE_BORDER are needed as above), admits handles that have a border under
 * PGF_BATCH_BAND_CTL: pgf_batch_ctl_init / _iterate / _read drive the bordered batch on the narrow
 * route and on the wide route.  Step one of an iteration enqueues the factor phase and each
 * instance decides from its control word; step two under a policy that keeps the mask is enqueued
 * without factor-phase launches (a bad pivot in B or in S, or a miss of the guard, in step one has
 * frozen the instance, so every live instance holds valid Y, factor of S and kept factors of B).
 * The step is finished on the device as on an unbordered band batch: the pivot flag is that of B
 * or S, the inertia that of B plus S.  Handles without a border behave with the bit as under
 * PGF_BATCH_BAND_CTL alone.
 *
 * PGF_BATCH_CTL_REFINE, valid only with PGF_BATCH_BAND_CTL (PGF_INVALID otherwise; on a dense batch
 * it changes nothing): a banded step inside pgf_batch_ctl_iterate whose guard measure misses the
 * refine_tol its handle had at pgf_batch_ctl_init is REFINED on the device instead of rejected --
 * what pgf_batch_sync does on the instance's handle, by the same device functions in the same
 * order.  At most two rounds: a round runs while refine_tol < rel < 1 and stops when the measure
 * does not fall; each round keeps the solution, solves for the residual with the guard off (the
 * 8 x 8 reduction on the intact band; the solve phase against the kept factors on a wide band with
 * the split on, the whole reduction with it off; with a border the solve phase against Y and the
 * factor of S), adds the correction, takes the residual and the step again from the point the step
 * started from.  Afterwards the step is a miss -- bit 2, counted by pgf_batch_debug_ctl_stats,
 * rejected with 2 lambda -- if and only if the measure is still above the refine_fail the handle
 * had at pgf_batch_ctl_init.  Both rounds are enqueued at every banded step of the loop; the
 * workgroups of instances that do not refine return at once.  No factor is touched, so the lean
 * second step stays lean.  pgf_batch_debug_ctl_refine_stats counts refined steps and rounds;
 * pgf_batch_debug_band_wide_stats and pgf_batch_debug_border_stats count a round's solve phase as
 * a solve phase (split off: its reduction as a reduction).
 *
 * PGF_BATCH_LINE_SEARCH opens the Globalized policy (GlobalizedNewtonMethod.step, newton.py:218-304)
 * to a device batch: dense instances, banded ones on the narrow route and, with PGF_BATCH_WIDE_BAND,
 * on the wide route.  Together with any of PGF_BATCH_BORDER, PGF_BATCH_WIDE_BORDER,
 * PGF_BATCH_BAND_CTL, PGF_BATCH_BORDER_CTL, PGF_BATCH_CTL_REFINE it is PGF_INVALID with a message on
 * the first handle, before any handle is read further; an unsymmetric formulation is refused as for
 * every batch.  Creation reserves each handle's line-search vectors and the batch's blocks.  On
 * such a batch pgf_batch_step_async takes PGF_STEP_RECOMPUTE_MASK | PGF_STEP_REFACTOR |
 * PGF_STEP_LINE_SEARCH (the bit without both companions: PGF_INVALID, as on the handle) besides
 * the other policies; pgf_batch_ctl_iterate refuses the bit.  Per instance, as on the single handle
 * (pgf_qp_step above): the mask from the instance's current point with the caller's tau
 * (newton.py:244), the direction solved at its OUTER point (:248), the merits with the tau-less
 * mask of their own point (:251, :277), the Armijo term with the reference's sign and 1e-4 (:281-285),
 * the ladder alpha = 2^-k with 30 trials (:270-289), no trial when merit0 <= newton_tol (:254), the
 * new point measured from the outer point and clipped (:296, step_solver.py:25-48).  Every
 * instance's search runs in the same launches behind the step update: the step takes ONE stream
 * wait, in pgf_batch_sync, whatever the batch size and the trial counts.  pgf_batch_sync reports
 * status[i] = PGF_LINE_SEARCH when no trial was accepted (newton.py:291-292): the instance's point
 * has not moved, bit for bit, and diff[i] = 0; PGF_SINGULAR as for the other policies (no search is
 * applied, the point stays); a frozen instance sits the step out, and keeps its statistics.  An
 * instance the accuracy guard repairs on its handle runs its search there (extra waits).  Without
 * the flag the bit is refused as before ("served by single handles only").
 * pgf_batch_set_line_search: newton_tol (Params.newton_tol, default 1e-8) for the batch and its
 * handles; negative or NaN, or a batch without the flag: PGF_INVALID.
 * pgf_batch_line_search_stats: pgf_qp_line_search_stats per instance for the last such step --
 * arrays of B, trial_merits B x 30; any pointer may be NULL; PGF_NOT_READY before the first one. */
typedef struct pgf_batch_s *pgf_batch;
#define PGF_BATCH_WIDE_BAND 1u
#define PGF_BATCH_BAND_CTL 2u
#define PGF_BATCH_BORDER 4u
#define PGF_BATCH_WIDE_BORDER 8u
#define PGF_BATCH_BORDER_CTL 16u /* with PGF_BATCH_BORDER | PGF_BATCH_BAND_CTL */
#define PGF_BATCH_CTL_REFINE 32u /* with PGF_BATCH_BAND_CTL */
#define PGF_BATCH_LINE_SEARCH 64u /* alone or with PGF_BATCH_WIDE_BAND */
int pgf_batch_set_line_search(pgf_batch b, double newton_tol);
int pgf_batch_line_search_stats(pgf_batch b, double *alpha, int *trials, double *merit0, double *slope,
                                double *trial_merits);
int pgf_batch_create(const pgf_handle *handles, int count, pgf_batch *out);
int pgf_batch_create_ex(const pgf_handle *handles, int count, unsigned flags, pgf_batch *out);
int pgf_batch_destroy(pgf_batch b);
const char *pgf_batch_last_error(pgf_batch b);
/* pgf_qp_advance_outer for every instance: (x^, y^) <- (x, y), new dt and rho */
int pgf_batch_advance_outer(pgf_batch b, double dt, double rho);
/* the same with per-instance dt[i], rho[i] -- every instance runs its own step-size
 * controller -- and accept[i]: nonzero (or accept == NULL) = the instance's last steps were
 * accepted; zero = rejected, the instance goes back to its outer point (x, y) <- (x^, y^) and
 * retries with the new dt[i] (StepController.compute_step, step_control.py:80-107) */
int pgf_batch_advance_outer_each(pgf_batch b, const double *dt, const double *rho,
                                 const uint8_t *accept);
/* frozen[i] != 0: instance i sits out the following Newton steps until the next
 * pgf_batch_advance_outer* (the controller's early exits: converged after the first step,
 * distance_ratio_control.py:36-45, or a failed factorisation); NULL clears all */
int pgf_batch_set_frozen(pgf_batch b, const uint8_t *frozen);
/* pgf_qp_update_active_set for every instance (SimplifiedNewtonMethod.__init__) */
int pgf_batch_update_active_set(pgf_batch b, double tau);
/* one NewtonMethod.step per instance (policy bits as pgf_qp_step); enqueue only */
int pgf_batch_step_async(pgf_batch b, unsigned policy, double tau);
/* wait; per instance: status (PGF_OK / PGF_SINGULAR), negative pivots of the factor in
 * use, ||(dx, dy)||.  Any output may be NULL.  Returns PGF_OK even when single instances
 * failed -- their status says so (the reference would reject only those steps). */
int pgf_batch_sync(pgf_batch b, int *status, int *n_neg, double *diff);
/* unscaled residual norms of all instances: host array and / or device array (the
 * rank-local block of the RCCL all-gather) */
int pgf_batch_residual_norms(pgf_batch b, double *norms_out, double *norms_out_dev);
/* ---- device-resident step controller -------------------------------
 * The reference's default DistanceRatioController (step/distance_ratio_control.py:12-78: two
 * Newton steps per outer iteration, theta = |step 2| / |step 1|, accept iff theta <= theta_max,
 * PI law on log(theta) for lambda, controller.py:54-77; early exits :34-45; a failed
 * factorisation = rejected step with 2 lambda, step_control.py:103-107) for every instance of
 * the batch, decided ON THE DEVICE: pgf_batch_ctl_iterate enqueues `iterations` outer
 * iterations back to back with no host synchronisation in between (per-instance lambda, PI
 * integral, accept flag and frozen flags live in HBM).  params: newton_tol, lamb_red,
 * lamb_min, lamb_inc, theta_max, K_P, K_I, theta_ref (Params fields of the same names).
 * pgf_batch_ctl_read waits and returns the next lambda and the last accept flag of every
 * instance and, per outer iteration and instance, (lambda used, lambda next, accepted). */
int pgf_batch_ctl_init(pgf_batch b, double lamb_init, double rho, const double *params,
                       int max_iterations);
int pgf_batch_ctl_iterate(pgf_batch b, unsigned policy, double tau, int iterations);
int pgf_batch_ctl_read(pgf_batch b, double *lamb, uint8_t *accepted, double *log3, int log_rows);

/* all points / masks, instance-major: x[count][n], y[count][m], mask[count][n] */
int pgf_batch_get_points(pgf_batch b, double *x, double *y);
int pgf_batch_get_masks(pgf_batch b, uint8_t *mask);
/* pgf_qp_measures for every instance: out[count][4] */
int pgf_batch_measures(pgf_batch b, double active_tol, double *out);
int pgf_batch_stream(pgf_batch b, void **stream_out);
/* Instances whose step the accuracy guard REPAIRED inside pgf_batch_sync since the batch was
 * created: the sampled residual of the batched solve failed, and the single-instance guard on the
 * instance's handle (full residual, refinement, pivoted LU) produced the step. */
int pgf_batch_refinement_stats(pgf_batch b, int *repaired);
/* ---- the batched mode's one collective, without Python ----------------
 * One process per GPU; every rank advances its shard of the instances as a device batch and the
 * residual norms of ALL instances are all-gathered once per step (the reference gathers per-
 * instance results from its process pool, runners/runner.py:107-153).  pygradflow_amd/batched.py
 * does this through torch.distributed (backend "nccl" = RCCL); these entry points do the same for
 * a host without PyTorch: librccl.so is opened at run time (dlopen; the library has no link-time
 * dependency on it), rank 0 creates the 128-byte id and hands it to the other ranks by whatever
 * means the host has, every rank creates its communicator on its own device.
 * pgf_batch_allgather_norms: ||F|| of the batch's current points (as pgf_batch_residual_norms)
 * into slot `rank' of all_dev -- a DEVICE array of nranks * count doubles -- and one
 * ncclAllGather on the batch's stream; returns after the stream has drained.  Every rank must
 * hold the same number of instances.  PGF_NOT_READY if librccl.so cannot be loaded. */
typedef struct pgf_comm_s *pgf_comm;
#define PGF_COMM_ID_BYTES 128
int pgf_comm_unique_id(void *id_out);
int pgf_comm_create(int nranks, int rank, const void *id, int device, pgf_comm *out);
int pgf_comm_destroy(pgf_comm c);
int pgf_batch_allgather_norms(pgf_batch b, pgf_comm c, double *all_dev);
/* as pgf_profile_enable / pgf_profile_read, for the batch's trailing-update launches */
int pgf_batch_profile_enable(pgf_batch b, int on);
int pgf_batch_profile_read(pgf_batch b, double *update_ms, int64_t *update_launches,
                           double *update_flops);

/* ---- stand-alone dense linear solver (LinearSolver ABC) ------------------ */
/* LinearSolver.__init__ factorises in the constructor
 * (linear_solver/linear_solver.py:18-21, lu_solver.py:9-17).  A: dense row-major N x N.
 * symmetric != 0: LDL^T on the lower triangle; symmetric == 0: LU with partial pivoting of the
 * full matrix (what the reference's LUSolver does for every matrix; needed by its Standard /
 * Extended / Asymmetric step-solver formulations, step/solver/).  PGF_SINGULAR on failure.
 * pgf_ls_solve(trans != 0) solves with A^T (cond_estimate.py:82).  pgf_ls_num_neg: LDL^T only
 * (PGF_NOT_READY for an LU: LUSolver.num_neg_eigvals() is None).  pgf_ls_get_factor copies
 * L below / D on the diagonal, or for the LU: unit-lower L below, U on and above. */
int pgf_ls_create_dense(int N, const double *A, int64_t lda, int symmetric, int device,
                        pgf_ls_handle *out);
int pgf_ls_solve(pgf_ls_handle ls, const double *rhs, int trans, double *sol);
int pgf_ls_num_neg(pgf_ls_handle ls, int *out);
/* debug / parity: copy the factor (unit-lower L below the diagonal, D on it) to host */
int pgf_ls_get_factor(pgf_ls_handle ls, double *LD_out, int64_t ld);
/* debug / parity, LU handles only (PGF_NOT_READY for an LDL^T): perm_out[N] -- row i of P A is
 * row perm_out[i] of A; the number of 32-column panels the last factorisation took with the rows
 * in registers (k_lu_panel_reg) / through the streaming kernel (k_lu_panel: panels taller than
 * 5120 rows, or all of them under PGF_LU_PANEL=1).  Any pointer may be NULL. */
int pgf_ls_debug_lu(pgf_ls_handle ls, int *perm_out, int *reg_panels, int *streamed_panels);
int pgf_ls_destroy(pgf_ls_handle ls);

/* ---- kernel micro-benchmark hook (tools/, bench diagnostics) ------------------ */
/* Times `reps` launches of the factorisation's trailing-update kernel on a synthetic
 * N x N lower-triangular region with K-depth KB (variant selects the tile kernel);
 * returns the mean launch time in ms and the algorithmic flops of one launch. */
int pgf_bench_update(int N, int KB, int variant, int reps, int device, double *ms_out,
                     double *flops_out);

/* out <- K v: the reduced KKT matrix of the current active set applied to a host vector of
 * length N = |I| + m on the device, from H, J and the mask (symmetric: K' v is the same).
 * These are the `mat @ x` / `mat.T @ x` products of the reference's ConditionEstimator
 * (step/cond_estimate.py:60-82); dense mode only. */
int pgf_kkt_apply(pgf_handle h, const double *v, double *out);

/* ---- the reference's unsymmetric step-solver formulations --------------------------------
 * StandardStepSolver (step/solver/standard_step_solver.py:15-92), ExtendedStepSolver
 * (extended_step_solver.py:13-112) and AsymmetricStepSolver (asymmetric_step_solver.py:15-173)
 * take the same Newton step through an unsymmetric (n + m) x (n + m) matrix and a pivoted LU.
 * pgf_set_formulation selects one on a DENSE handle (PGF_INVALID on a PGF_CREATE_SPARSE handle
 * and for unknown values) and invalidates the factor; a handle that never calls it is Symmetric
 * and behaves as described everywhere else in this header.  With another formulation the matrix
 * is assembled in HBM from the resident H, J, mask and index lists and factorised in place by
 * the LU of pgf_lu.hip; no (n + m)^2 matrix crosses PCIe.  The entry points keep their meaning
 * over the (n + m) system:
 *   pgf_factor          assemble + LU; *n_neg = -1 (LUSolver.num_neg_eigvals() is None)
 *   pgf_newton_solve    residual, right-hand side in the formulation's row order, solve,
 *                       dy = fact (s_y - rho b2) (Standard: s_y), clipping, diff;
 *                       inertia_check != 0 -> PGF_INVALID
 *   pgf_residual, pgf_active_set   Standard: the UNSCALED residual / mask (ImplicitFunc,
 *                       implicit_func.py:102-199); Extended / Asymmetric: the scaled ones
 *   pgf_linear_solve    rhs / sol have n + m entries, trans != 0 solves with the transpose
 *   pgf_reduced_dims    |I|, n + m
 *   pgf_qp_update_active_set, pgf_qp_step / _async / pgf_qp_sync   all policy bits; n_neg = -1;
 *                       pgf_qp_step with inertia_check != 0 -> PGF_INVALID.  A step that
 *                       factorises waits once inside pgf_qp_step_async (the LU reads its pivots).
 * Standard needs H + rho J^T J (aug_lag_deriv_xx(rho), standard_step_solver.py:52): a caller of
 * pgf_set_derivs_* uploads that matrix as H; after pgf_qp_set_problem (H = Q) the rho J^T J term
 * comes from the resident Gram matrix (pgf_debug_gram_stats), built once per derivative upload.
 * The LDL^T accuracy guard does not apply (the LU pivots).  Batched (pgf_batch_create refuses a
 * handle whose formulation is not Symmetric) and banded unsymmetric formulations are out of scope. */
#define PGF_FORM_SYMMETRIC 0 /* default */
#define PGF_FORM_STANDARD 1
#define PGF_FORM_EXTENDED 2
#define PGF_FORM_ASYMMETRIC 3
int pgf_set_formulation(pgf_handle h, int form);
/* the assembled (pre-factor) Newton matrix of the current formulation, row-major (n + m) x
 * (n + m) (debug / parity, like pgf_get_kkt; re-assembles, does not disturb the factor);
 * PGF_INVALID on a Symmetric handle */
int pgf_get_newton_matrix(pgf_handle h, double *M_out, int64_t ld);
/* counters since pgf_create: device assemblies made for a factorisation, LU factorisations, and
 * the bytes of (n + m)^2 matrices that crossed PCIe for this handle -- 0 on the device path; the
 * host-assembly path of the Python classes (PGF_UNSYM_HOST=1) reports each matrix
 * it sends to the stand-alone LU with pgf_debug_unsym_note_upload */
int pgf_debug_unsym_stats(pgf_handle h, int *assemblies, int *lu_factorisations,
                          int64_t *matrix_bytes_from_host);
int pgf_debug_unsym_note_upload(pgf_handle h, int64_t bytes);

/* ---- accuracy guard of the dense path ---------------------------------------------- */
/* The reference factorises the reduced KKT matrix with a PIVOTED sparse LU (SuperLU through
 * scipy.sparse.linalg.splu, linear_solver/lu_solver.py:14) and therefore stays accurate when
 * H[I,I] + lambda I is indefinite (symmetric_step_solver.py:146-153 only checks the inertia on
 * request).  The unpivoted LDL^T used here is checked instead: after every solve
 * max |rhs - K s| is compared with tol * max |rhs| (K applied from H, J and the mask); beyond
 * that, up to two steps of iterative refinement, then a dense LU with partial pivoting of the
 * same matrix; PGF_SINGULAR only if that fails as well.  mode 0 switches the check off;
 * tol / fail_tol <= 0 keep the defaults (1e-11, 1e-7). */
int pgf_set_refinement(pgf_handle h, int mode, double tol, double fail_tol);
/* counters since pgf_create: refinement steps taken, LU factorisations, and the relative
 * residual of the last checked solve */
int pgf_refinement_stats(pgf_handle h, int *refined, int *lu_fallbacks, double *last_rel_residual);

/* ---- test hooks ------------------------------------------------------------------ */
/* The triangular solves of the dense path run as ONE launch whose workgroups hand the
 * solution over block by block; every such solve checks itself (placement of its workers,
 * bounded waits).  A failed check never surfaces: the call that notices it repeats the solve
 * with the per-block kernels before it returns and the chained kernels stay off for the
 * rest of the process.  pgf_debug_fail_next_chain makes the next chained solve of the
 * handle look failed (status word set, solution overwritten with NaN) so that the recovery
 * can be tested; pgf_debug_chain_enable(1) switches the chained kernels back on. */
int pgf_debug_fail_next_chain(pgf_handle h);
int pgf_debug_chain_enable(int on);
/* The dense factorisation's diagonal chain hands work to two helper workgroups of the same
 * launch; a failed placement check or a timed-out hand-over switches them off
 * for the rest of the process and the factorisation (and the step built on it) is repeated
 * inside the call that notices.  pgf_debug_fail_next_helper makes the next factorisation of
 * this handle report such a failure; pgf_debug_chain_helpers(1 / 0) switches the helpers on /
 * off, (-1) only queries; returns the previous state (1 = on). */
int pgf_debug_fail_next_helper(pgf_handle h);
/* batched mode (chains with helpers up to 32 instances): instance 0's next factorisation reports
 * failed helpers -- its step comes back as failed (status PGF_SINGULAR), which the controllers
 * reject and repeat, and the helpers are switched off */
int pgf_batch_debug_fail_next_helper(pgf_batch b);
int pgf_debug_chain_helpers(int on);
/* Which factorisation the handle's current dense factor is (tests, tools/check_condensed.py):
 * 0 none / stale, 1 LDL^T of the reduced KKT matrix in its natural order, 2 LDL^T of the
 * condensed system (constraint block eliminated first: condensed_wanted in csrc/pgf_api_factor.hip), 3 the
 * pivoted LU that took over after a failed residual check. */
int pgf_debug_factor_kind(pgf_handle h);
/* The pivot order of the factors a device batch's instances hold (tests): 0 none (no step yet),
 * 1 the natural order, 2 the condensed system; the same for every instance of the batch. */
int pgf_batch_debug_factor_kind(pgf_batch b);
/* Counters of the dense qp steps (tests): host_syncs -- host synchronisations made for the
 * index-set sizes and the step's status (a Full step: one while |I| keeps its size, two with
 * PGF_STEP_SPEC=0; an ActiveSet step waits once more for the mask difference before it is
 * enqueued); redone_steps -- steps enqueued with the previous |I|, |A| that were discarded and
 * enqueued again by pgf_qp_sync because the sizes had changed.  Either pointer may be NULL. */
int pgf_debug_step_stats(pgf_handle h, int *host_syncs, int *redone_steps);
/* Counters of the waits of the dense qp steps that end in the hand-back launch (tests; DESIGN.md
 * 4d, PGF_STEP_HANDBACK): by_word -- waits satisfied by the sequence word the step's last launch
 * stores into host memory, without a runtime call; fell_back -- waits whose spin bound expired (or
 * was zero) and that ended in hipStreamSynchronize.  A wait already taken for the same step (pgf_qp_sync
 * behind pgf_qp_residual_norm) counts in neither.  Either pointer may be NULL. */
int pgf_debug_handback_stats(pgf_handle h, int *by_word, int *fell_back);
/* Test hook: the wall-clock bound of that spin in seconds; 0: no spin, every wait falls back;
 * negative: the bound derived from the previous step's duration again. */
int pgf_debug_handback_spin_bound(pgf_handle h, double seconds);
/* Counters of the mask refreshes of the dense qp steps and of pgf_qp_update_active_set (tests;
 * DESIGN.md 4d, PGF_UNBOUNDED_FRONT): general -- those that evaluated the mask (and compacted it or
 * waited for its difference); unbounded -- those of a handle without a finite bound, which launch
 * nothing once the empty mask and the identity lists are on the device.  Either pointer may be NULL. */
int pgf_debug_front_stats(pgf_handle h, int *general, int *unbounded);
/* Device time (ms) of the last line-search stage -- the direction's images, k_ls_ladder,
 * k_ls_finish -- of a step with PGF_STEP_LINE_SEARCH made while profiling was enabled
 * (pgf_profile_enable); 0 before. */
int pgf_debug_line_search_ms(pgf_handle h, double *ms);
/* Counters of the resident Gram matrix G = J^T J of the condensed dense factorisation (tests;
 * DESIGN.md 4.0, PGF_CONDENSED_GRAM): builds -- how often G was formed for this handle (at most
 * once per derivative upload); factorisations_with_gram -- condensed factorisations that took
 * their rank-m term from G instead of the virtual column blocks (a factorisation that was
 * discarded and enqueued again counts once).  Either pointer may be NULL. */
int pgf_debug_gram_stats(pgf_handle h, int *builds, int *factorisations_with_gram);
/* Counters of the dense factorisations by how the step's head -- K's assembly and the condensed
 * system's panel -- was enqueued (tests; DESIGN.md 4.1b, PGF_HEAD_FUSED): fused -- beside the
 * first diagonal chain, in its launch; plain -- as launches of their own in front of it (a
 * factorisation that was discarded and enqueued again counts once).  Either pointer may be NULL. */
int pgf_debug_head_stats(pgf_handle h, int *fused, int *plain);
/* Counters of the qp steps enqueued with the residual check and the evaluation ahead, by their
 * launch sequence behind the back-solve (tests; DESIGN.md 4d, PGF_STEP_FUSED): fused_steps -- s_y in
 * the step update, one row launch over J and H, one combine launch; plain_steps -- the separate
 * launches (a step that was discarded and enqueued again counts twice).  Either pointer may be NULL. */
int pgf_debug_tail_stats(pgf_handle h, int *fused_steps, int *plain_steps);
/* The unit list of the fused head, walked on the host (no GPU) for a reduced size: nI inactive
 * variables, m constraints, condensed != 0: N = nI and a panel V of m columns padded to mp = a
 * multiple of 32; else N = nI + m and no panel.  Counts are ADDED per entry: k_units (N x N) --
 * units of the chain's launch that write the entry of K; k_head (N x N) -- the same for the head
 * launch in front; v_units ((nI + 1) x mp, the tail row last) -- units that write the entry of V;
 * n_units -- the length of the list (for N <= 256 the panel's tiles alone; no head is fused for
 * such a size).  Any pointer may be NULL. */
int pgf_debug_head_plan(int nI, int m, int condensed, int *k_units, int *k_head, int *v_units, int *n_units);
/* The lazy trailing-update plan of the dense LDL^T, walked on the host: no handle,
 * no GPU.  N x N lower triangle plus rows up to nrows (N or N + 1), a pre-eliminated block of depth
 * vdepth (a multiple of 32, 0: none).  budget: tile-blocks per launch, 0 = no limit (the eager
 * plan), with `cap' pending blocks per optional job; budget < 0: the plan production factorises this
 * size with -- the same selection and caches, PGF_LAZY_BUDGET and PGF_LAZY_CAP ignored, cap ignored.
 * Stage -1 runs beside the first diagonal chain (virtual blocks only), stage k >= 0 beside the chain
 * of column block k + 1.
 *   jobs      PGF_UPDATE_PLAN_JOB_INTS ints per job, at most jobs_cap jobs: stage, col0, ntc,
 *             rowstart, kc0v, KBv, kc0, KB, first tile number, one past its last -- stage by stage, in
 *             the order of the stage's job table
 *   tiles     4 ints per tile, at most tiles_cap tiles: stage, job (index in its stage), i0, j0 --
 *             every tile number of every stage from 0 until the device's own numbering (one shared
 *             host / device function) reports the end; NULL or tiles_cap <= 0: not walked
 *   n_jobs, n_tiles   the numbers there are (whatever the capacities)
 *   stage_jobs        ceil(N / 256) ints: the jobs of stage -1, 0, 1, ...
 *   budget_out        the budget of the plan returned (0: no limit)
 * Any pointer may be NULL. */
#define PGF_UPDATE_PLAN_JOB_INTS 10
int pgf_debug_update_plan(int N, int nrows, int vdepth, int budget, int cap, int *jobs, int jobs_cap,
                          int *n_jobs, int *tiles, int tiles_cap, int *n_tiles, int *stage_jobs,
                          int *budget_out);
/* the handle's border size and the factor / solve phases of the bordered route enqueued since
 * pgf_sparse_set_border (tests: a step that keeps its factor runs the solve phase only) */
int pgf_debug_border_stats(pgf_handle h, int *k, int *border_factorisations, int *border_solves);
/* large border: C and Y = inv(B) C (Nb x kp each, row-major, Nb = n + m - k) and G = C' Y (kp x kp,
 * lower triangle, zero above) of the last factor phase.  Any pointer may be NULL.  PGF_NOT_READY
 * before the first factor phase, PGF_INVALID without a large border. */
int pgf_debug_border_gram(pgf_handle h, double *C, double *Y, double *G);
/* large border: the Gram kernel's launch plan on this handle -- rows per chunk, row chunks and
 * 64 x 64 tiles of the lower triangle; the grid is tiles x chunks.  Any pointer may be NULL.
 * PGF_INVALID without a large border. */
int pgf_debug_border_gram_plan(pgf_handle h, int *rows, int *chunks, int *tiles);
/* measurement (tools/time_border.py): device time in ms per launch, over `reps` launches, of the
 * Gram launch alone on the C and Y of the last factor phase of a bordered handle whose kp is a
 * multiple of 64 -- *ms_mfma: the large border's MFMA kernel; *ms_fma: the small border's FMA
 * kernel (kp = 64 only, -1 beyond).  Production at kp <= 64 runs the FMA kernel. */
int pgf_debug_border_gram_time(pgf_handle h, int reps, double *ms_mfma, double *ms_fma);
/* phases of the wide band (B = 16, 32, 64) enqueued on the handle since its creation: reductions
 * (fused or factor-only), solve phases for one right-hand side against kept factors, panel
 * solves.  Any pointer may be NULL. */
int pgf_debug_band_stats(pgf_handle h, int *reductions, int *solve_phases, int *panel_solves);
/* A band batch's batched launch sequences enqueued since its creation (tests: the batched route
 * ran, not a loop over the handles): reductions -- one per step, for all instances; assemblies --
 * steps that enqueued the band assembly.  Zeros on a dense batch.  Any pointer may be NULL. */
int pgf_batch_debug_band_stats(pgf_batch b, int *reductions, int *assemblies);
/* per instance: wide reductions and solve phases the instance's workgroups ran since the batch was
 * created (arrays of `count` ints, synchronises); *lean_steps: steps enqueued without inversion
 * launches.  Zeros on a dense or narrow batch.  Any pointer may be NULL. */
int pgf_batch_debug_band_wide_stats(pgf_batch b, int *reductions, int *solve_phases, int *lean_steps);
/* per instance: Newton steps that pgf_batch_ctl_iterate's loop on a band batch (PGF_BATCH_BAND_CTL)
 * rejected for a zero or non-finite pivot, and steps it rejected because the guard's measure missed
 * the instance's refine_tol, since the batch was created (arrays of `count` ints, synchronises).
 * Zeros on a dense batch and on a band batch without the flag.  Any pointer may be NULL. */
int pgf_batch_debug_ctl_stats(pgf_batch b, int *pivot_rejects, int *guard_rejects);
/* per instance: steps of pgf_batch_ctl_iterate's loop that were refined on the device
 * (PGF_BATCH_CTL_REFINE) and the refinement rounds they ran, since the batch was created (arrays of
 * `count` ints, synchronises).  Zeros on a batch without the flag.  Any pointer may be NULL;
 * b == NULL is PGF_INVALID and leaves the outputs alone. */
int pgf_batch_debug_ctl_refine_stats(pgf_batch b, int *refined_steps, int *rounds);
/* per instance: factor phases and solve phases of the bordered route the instance ran since the
 * batch was created (PGF_BATCH_BORDER; arrays of `count` ints, counted on the device, synchronises).
 * Zeros on a batch that is not bordered.  Any pointer may be NULL. */
int pgf_batch_debug_border_stats(pgf_batch b, int *factor_phases, int *solve_phases);
/* The last step with PGF_STEP_LINE_SEARCH of a batch (PGF_BATCH_LINE_SEARCH): *stage_launches -- the
 * launches its line-search stage enqueued for the whole batch (the direction's images u = A dx,
 * v = Q dx + A'(rho u + dy), the ladder, the finish; newton.py:259-296 in one pass), which depend
 * neither on the batch size nor on any trial count; *host_waits -- the stream waits from
 * pgf_batch_step_async to the end of pgf_batch_sync, 1 unless an instance was repaired on its
 * handle.  Zeros before the first such step.  Either pointer may be NULL. */
int pgf_batch_debug_line_search_stats(pgf_batch b, int *stage_launches, int *host_waits);
/* The 64-bit hash a banded handle keeps of its pattern (host only, no device needed): FNV-1a over
 * n, m, bw, the entry counts and every index array as pgf_sparse_set_pattern receives them. */
int pgf_sparse_pattern_hash(int n, int m, int bw, const int *pos, int nnzH, const int *Hptr,
                            const int *Hrow, const int *Hcol, const int *Hslot, int nnzJ,
                            const int *Jptr, const int *Jcol, const int *Jslot, const int *JTptr,
                            const int *JTrow, const int *JTmap, uint64_t *hash_out);

#ifdef __cplusplus
}
#endif
#endif /* PGF_HIP_H */
