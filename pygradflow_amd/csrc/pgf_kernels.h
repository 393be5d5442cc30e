// Launch wrappers of the single-handle step kernels (all asynchronous on the given stream).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// 1-D grid of ceil(n / b) workgroups
static inline dim3 g1(int n, int b = 256) { return dim3((n + b - 1) / b); }

// ---- pgf_kernels.hip: the step ----------------------------------------------
void launch_scale_bounds(hipStream_t s, int n, double lamb, const double *lb, const double *ub,
                         double *slb, double *sub);
void launch_active_set(hipStream_t s, int n, int use_tau, double lamb, double f_x, double f_x0,
                       double f_d, const double *xhat, const double *x, const double *g,
                       const double *slb, const double *sub, uint8_t *mask);
// counts[0, 1] <- |I|, |A|; counts[3] <- (|I| != expect) for expect >= 0, else 0
void launch_compact(hipStream_t s, int n, const uint8_t *mask, int *idxI, int *idxA, int *pos,
                    int *counts, int expect);
// launch_active_set into `mask' and launch_compact of it in one single-workgroup launch
void launch_mask_compact(hipStream_t s, int n, int use_tau, double lamb, double f_x, double f_x0,
                         double f_d, const double *xhat, const double *x, const double *g,
                         const double *slb, const double *sub, uint8_t *mask, int *idxI, int *idxA,
                         int *pos, int *counts, int expect);
// launch_mask_compact and launch_residual_rhs (nI: the count the step is enqueued with) in the one launch
void launch_mask_compact_rhs(hipStream_t s, int n, int m, int nI, int use_tau, double lamb, double f_x,
                             double f_x0, double f_d, double dt, double fact, const double *xhat,
                             const double *yhat, const double *x, const double *y, const double *g,
                             const double *c, const double *slb, const double *sub, uint8_t *mask, int *idxI,
                             int *idxA, int *pos, int *counts, int expect, double *F, double *b0full,
                             double *rhs);
// mask <- 0, idxI = pos <- the identity, counts <- (n, 0, ., 0): a handle without a finite bound
void launch_unbounded_sets(hipStream_t s, int n, uint8_t *mask, int *idxI, int *pos, int *counts);
// xhat <- x, yhat <- y, (slb, sub) <- lamb (lb, ub) in one launch
void launch_advance_outer(hipStream_t s, int n, int m, double lamb, const double *x, const double *y,
                          const double *lb, const double *ub, double *xhat, double *yhat, double *slb,
                          double *sub);
void launch_residual(hipStream_t s, int n, int m, double lamb, double dt, const double *xhat,
                     const double *yhat, const double *x, const double *y, const double *g,
                     const double *c, const double *slb, const double *sub, const uint8_t *mask,
                     double *F, double *b0full);
// launch_residual and, for |A| = 0, launch_reduced_rhs in one launch
void launch_residual_rhs(hipStream_t s, int n, int m, int nI, double lamb, double dt, double fact,
                         const double *xhat, const double *yhat, const double *x, const double *y,
                         const double *g, const double *c, const double *slb, const double *sub,
                         const uint8_t *mask, const int *idxI, double *F, double *b0full, double *rhs);
void launch_reduced_rhs(hipStream_t s, int n, int m, int nI, int nA, double fact, const double *F,
                        const int *idxI, const int *idxA, const double *H, int64_t ldh, const double *J,
                        int64_t ldj, const double *b0full, double *partial, int nparts, double *rhs);
void launch_assemble_kkt(hipStream_t s, double *K, int64_t ldk, const double *H, int64_t ldh,
                         const double *J, int64_t ldj, const int *idxI, int nI, int m,
                         double lamb, double delta, int *zero = nullptr, int nzero = 0,
                         const double *row_src = nullptr, double *row_dst = nullptr, int row_n = 0,
                         const double *G = nullptr, int64_t ldg = 0);
// the first diagonal block's rows of the assembly described by hw (pgf_ldlt.h), the zeroing of
// `zero' and the rhs row: the launch in front of a first chain that carries the rest (k_chain_head)
struct LdltHead;
void launch_assemble_kkt_head(hipStream_t s, double *K, int64_t ldk, const LdltHead &hw, int *zero, int nzero);
void launch_copy(hipStream_t s, double *dst, const double *src, int n);
void launch_copy_u8(hipStream_t s, uint8_t *dst, const uint8_t *src, int n);
void launch_mask_diff(hipStream_t s, int n, const uint8_t *a, const uint8_t *b, int *out);
int step_update_blocks(int n, int m);
// cy: the y rows form the condensed step's s_y = (sum_p partial[p][r] - rhs_y[r]) / delta themselves
// (k_cond_y's order; partial as launch_cond_y_partial left it) and store it to sol_y
struct StepCondY {
  const double *partial, *rhs_y;
  double *sol_y;
  double delta;
  int nparts;
};
void launch_step_update(hipStream_t s, int n, int m, int nI, double fact, double rho,
                        const double *x, const double *y, const double *lb, const double *ub,
                        const uint8_t *mask, const int *pos, const double *b0full,
                        const double *F, const double *sol, double *dx, double *dy, double *xn,
                        double *yn, double *red, double *diff_out, unsigned *ticket, double lamb = 0.0,
                        double *v = nullptr, double *lv = nullptr, double *zero3 = nullptr,
                        const int *flags_src = nullptr, const int *chain_src = nullptr,
                        int *status = nullptr, const StepCondY *cy = nullptr);
void launch_gemv_rows(hipStream_t s, int rows, int cols, const double *M, int64_t ld,
                      const double *v, const double *add, double sgn, double *out);
void launch_gemvT(hipStream_t s, int rows, int cols, const double *M, int64_t ld,
                  const double *w, const double *base, double *partial, int nparts, double *out);
void launch_mult_vec(hipStream_t s, int m, double rho, const double *c, const double *y,
                     double *w);
void launch_unscaled_res_norm(hipStream_t s, int n, int m, double dt, const double *xhat,
                              const double *yhat, const double *x, const double *y,
                              const double *g, const double *c, const double *lb,
                              const double *ub, double *red, double *out, double *out2,
                              unsigned *ticket);
void launch_final_reduce(hipStream_t s, const double *red, int cnt, double *out, int take_sqrt);
void launch_measures(hipStream_t s, int n, int m, double active_tol, const double *x,
                     const double *y, const double *r, const double *c, const double *lb,
                     const double *ub, double *red, double *out);
void launch_csr_to_dense(hipStream_t s, int rows, const int *ptr, const int *idx, const double *val,
                         double *dst, int64_t ld);
// condensed KKT system (constraint block eliminated first; pgf_kernels.hip, pgf_api_factor.hip):
// V <- J[:, I]^T zero-padded to mp columns, row nI <- rhs_y (or 0), vd <- -1 / delta
void launch_cond_panel(hipStream_t s, double *V, int64_t ldv, int mp, double *vd, const double *J,
                       int64_t ldj, const int *idxI, int nI, int m, double delta, const double *rhs_y);
// out <- rhs_x + V rhs_y / delta
void launch_cond_rhs(hipStream_t s, int nI, int m, const double *V, int64_t ldv, const double *rhs,
                     double delta, double *out);
// sol_y <- (V^T sol_x - rhs_y) / delta
void launch_cond_y(hipStream_t s, int nI, int m, const double *V, int64_t ldv, const double *solx,
                   const double *rhs_y, double delta, double *partial, size_t partial_cap, double *sol_y);
// launch_cond_y's first launch alone (the partial products); returns the number of chunks written,
// for StepCondY::nparts
int launch_cond_y_partial(hipStream_t s, int nI, int m, const double *V, int64_t ldv, const double *solx,
                          double *partial, size_t partial_cap);

// ---- pgf_guard_kernels.hip: residual guard and evaluation ahead --------------
// r = rhs - K s of the reduced KKT system, K applied from H, J and the mask (never assembled);
// red3 <- max |r|, max |rhs|, max |s|.  v, lv, u: n-vectors of scratch, wy: m, r: nI + m.
void launch_kkt_residual(hipStream_t s, int n, int m, int nI, double lamb, double delta,
                         const double *H, int64_t ldh, const double *J, int64_t ldj,
                         const int *idxI, const int *pos, const uint8_t *mask, const double *rhs,
                         const double *sol, double *v, double *lv, double *u, double *wy,
                         double *partial, int nparts, double *r, double *red3,
                         bool prepared = false);
void launch_axpy1(hipStream_t s, int N, const double *d, double *x);
void launch_symmetrize(hipStream_t s, double *A, int64_t ld, int N);
// ||H||_inf, ||J||_inf, ||J||_1 -> norms3 (device), for the normwise backward error of the guard
void launch_matrix_norms(hipStream_t s, int n, int m, const double *H, int64_t ldh, const double *J,
                         int64_t ldj, double *norms3);
// What k_tail_combine takes to leave the new point's unscaled residual norm and hand the step's
// status block back to the host (launch_residual_and_eval_fused; x, y: the NEW point): red --
// (n + m + 255) / 256 partials; norm_out -- inside the block stat[0, nstat); h_stat -- coherent host
// memory, nstat doubles and the sequence word behind them, which receives seq
struct TailHandback {
  double dt;
  const double *xhat, *yhat, *x, *y, *c, *lb, *ub;
  double *red, *norm_out;
  unsigned *ticket;
  const double *stat;
  int nstat;
  double *h_stat;
  unsigned long long seq;
};
// launch_residual_and_eval(..., prepared = true) with the row passes over J and H in one launch and
// the sums, the H pass's epilogue and the residual in another: at most three launches, same values
void launch_residual_and_eval_fused(hipStream_t s, int n, int m, int nI, double delta, const double *H, int64_t ldh,
                                    const double *J, int64_t ldj, const int *pos, const uint8_t *mask,
                                    const double *rhs, const double *sol, const double *v, double *lv, double *u,
                                    double *wy, double *partial, int nparts, double *r, double *red3,
                                    const double *xn, const double *yn, const double *b, const double *q,
                                    double rho, double *c, double *w, double *tmpn, double *g,
                                    const TailHandback *th = nullptr);
// the status block (nstat doubles, the norm at norm_at) to coherent host memory, the norm to slot
// (device, may be null), then the sequence word h_stat[nstat] <- seq: one workgroup
void launch_handback_store(hipStream_t s, const double *stat, int nstat, int norm_at, double *h_stat,
                           unsigned long long seq, double *slot);
// launch_kkt_residual of the solve just made AND the evaluation of g, c at the new point (xn, yn)
// in one pass over H and two over J (the separate kernels: two and four); partial: 2 * nparts * n
void launch_residual_and_eval(hipStream_t s, int n, int m, int nI, double lamb, double delta, const double *H,
                              int64_t ldh, const double *J, int64_t ldj, const int *idxI, const int *pos,
                              const uint8_t *mask, const double *rhs, const double *sol, double *v, double *lv,
                              double *u, double *wy, double *partial, int nparts, double *r, double *red3,
                              const double *xn, const double *yn, const double *b, const double *q, double rho,
                              double *c, double *w, double *tmpn, double *g, bool prepared = false);
