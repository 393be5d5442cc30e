// Kernels and launchers of the single-handle Newton step: elementwise, compaction, gather-assembly,
// matrix-vector and step-update kernels, CSR -> dense, and the condensed KKT system's panel kernels.
// The device bodies are in pgf_step_dev.h (shared with the batched twins, pgf_batch_kernels.hip);
// the residual guard and the evaluation ahead are in pgf_guard_kernels.hip.
// Compiled with -ffp-contract=off (the contraction rule: pgf_step_dev.h).
#include "pgf_kernels.h"

#include <algorithm>

#include "pgf_head_dev.h"
#include "pgf_ldlt.h"
#include "pgf_step_dev.h"

// ---------------------------------------------------------------- single-instance kernels
__global__ void k_scale_bounds(int n, double lamb, const double *__restrict__ lb,
    const double *__restrict__ ub, double *__restrict__ slb, double *__restrict__ sub) {
  b_scale_bounds(n, lamb, lb, ub, slb, sub);
}

__global__ void k_active_set(int n, int use_tau, double lamb, double f_x, double f_x0, double f_d,
    const double *__restrict__ xhat, const double *__restrict__ x, const double *__restrict__ g,
    const double *__restrict__ slb, const double *__restrict__ sub, uint8_t *__restrict__ mask) {
  b_active_set(n, use_tau, lamb, f_x, f_x0, f_d, xhat, x, g, slb, sub, mask);
}

__global__ __launch_bounds__(1024) void k_compact(int n, const uint8_t *__restrict__ mask,
    int *__restrict__ idxI, int *__restrict__ idxA, int *__restrict__ pos,
    int *__restrict__ counts, int expect) {
  b_compact(n, mask, idxI, idxA, pos, counts, expect);
}

__global__ __launch_bounds__(1024) void k_mask_compact(int n, ActiveArgs a, uint8_t *__restrict__ mask,
    int *__restrict__ idxI, int *__restrict__ idxA, int *__restrict__ pos,
    int *__restrict__ counts, int expect) {
  b_compact(n, nullptr, idxI, idxA, pos, counts, expect, &a, mask);
}

__global__ void k_residual(int n, int m, double lamb, double dt, const double *__restrict__ xhat,
    const double *__restrict__ yhat, const double *__restrict__ x, const double *__restrict__ y,
    const double *__restrict__ g, const double *__restrict__ c, const double *__restrict__ slb,
    const double *__restrict__ sub, const uint8_t *__restrict__ mask, double *__restrict__ F,
    double *__restrict__ b0full) {
  b_residual(n, m, lamb, dt, xhat, yhat, x, y, g, c, slb, sub, mask, F, b0full,
             blockIdx.x * blockDim.x + threadIdx.x);
}

// k_residual and, for |A| = 0 (b0full = 0: no correction terms), k_reduced_rhs in one launch: the
// rows of the reduced rhs take F at their index from the same per-element functions (bit-identical
// to reading it back; F - 0.0 == F), so no workgroup waits for another.  256 lanes per workgroup
// run the elementwise part, its 4 wavefronts one rhs row each.
__global__ __launch_bounds__(256) void k_residual_rhs(int n, int m, int nI, double lamb, double dt,
    double fact, const double *__restrict__ xhat, const double *__restrict__ yhat,
    const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ g,
    const double *__restrict__ c, const double *__restrict__ slb, const double *__restrict__ sub,
    const uint8_t *__restrict__ mask, const int *__restrict__ idxI, double *__restrict__ F,
    double *__restrict__ b0full, double *__restrict__ rhs) {
  b_residual(n, m, lamb, dt, xhat, yhat, x, y, g, c, slb, sub, mask, F, b0full,
             blockIdx.x * 256 + threadIdx.x);
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if ((threadIdx.x & 63) != 0 || i >= nI + m) return;
  if (i < nI) {
    rhs[i] = residual_x(idxI[i], lamb, xhat, x, g, slb, sub, mask) - 0.0;
  } else {
    const int r = i - nI;
    rhs[i] = fact * residual_y(r, lamb, yhat, y, c) - 0.0;
  }
}

// k_mask_compact and, for a step enqueued with |A| = 0, k_residual_rhs's work in the one workgroup:
// the constraint rows first (nI: the count the step is enqueued with), the variable rows in the
// compaction's own pass (FrontArgs), by the same per-element functions.
__global__ __launch_bounds__(1024) void k_mask_compact_rhs(int n, ActiveArgs a, uint8_t *__restrict__ mask,
    int *__restrict__ idxI, int *__restrict__ idxA, int *__restrict__ pos, int *__restrict__ counts,
    int expect, int m, int nI, double dt, double fact, const double *__restrict__ yhat,
    const double *__restrict__ y, const double *__restrict__ c, double *__restrict__ F,
    double *__restrict__ b0full, double *__restrict__ rhs) {
  for (int r = threadIdx.x; r < m; r += 1024) {
    F[n + r] = residual_y(r, a.lamb, yhat, y, c);
    rhs[nI + r] = fact * residual_y(r, a.lamb, yhat, y, c) - 0.0;
  }
  const FrontArgs front{dt, F, b0full, rhs};
  b_compact(n, nullptr, idxI, idxA, pos, counts, expect, &a, mask, &front);
}

// pgf_qp_advance_outer's two copies and the scaling of the bounds in one launch
__global__ void k_advance_outer(int n, int m, double lamb, const double *__restrict__ x,
    const double *__restrict__ y, const double *__restrict__ lb, const double *__restrict__ ub,
    double *__restrict__ xhat, double *__restrict__ yhat, double *__restrict__ slb,
    double *__restrict__ sub) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) xhat[i] = x[i];
  if (i < m) yhat[i] = y[i];
  b_scale_bounds(n, lamb, lb, ub, slb, sub);
}

__global__ __launch_bounds__(256) void k_active_rows_partial(int n, int nA, const int *__restrict__ idxA,
    const double *__restrict__ H, int64_t ldh, const double *__restrict__ b0full, int nparts,
    double *__restrict__ partial) {
  b_active_rows_partial(n, nA, idxA, H, ldh, b0full, nparts, partial);
}
__global__ __launch_bounds__(256) void k_reduced_rhs(int n, int m, int nI, int nA, double fact,
    const double *__restrict__ F, const int *__restrict__ idxI, const double *__restrict__ J,
    int64_t ldj, const double *__restrict__ b0full, const double *__restrict__ partial, int nparts,
    double *__restrict__ rhs) {
  b_reduced_rhs(n, m, nI, nA, fact, F, idxI, J, ldj, b0full, partial, nparts, rhs);
}

// (zero: words cleared by the first workgroup -- the factorisation's flags and tile counters;
// row_src: copied to row_dst[0, row_n) by the workgroups of the first row group)
__global__ __launch_bounds__(256) void k_assemble_kkt(double *__restrict__ K, int64_t ldk,
    const double *__restrict__ H, int64_t ldh, const double *__restrict__ J, int64_t ldj,
    const int *__restrict__ idxI, int nI, int m, double lamb, double delta, int *__restrict__ zero,
    int nzero, const double *__restrict__ row_src, double *__restrict__ row_dst, int row_n) {
  if (blockIdx.y == 0) {
    if (zero && blockIdx.x == 0)
      for (int t = threadIdx.x; t < nzero; t += 256) zero[t] = 0;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (row_src && j < row_n) row_dst[j] = row_src[j];
  }
  b_assemble_kkt(blockIdx.x, blockIdx.y, threadIdx.x, K, ldk, H, ldh, J, ldj, idxI, nI, m, lamb, delta);
}
// the same with the Gram operand (a kernel of its own: k_assemble_kkt keeps its code and its
// argument list)
__global__ __launch_bounds__(256) void k_assemble_kkt_gram(double *__restrict__ K, int64_t ldk,
    const double *__restrict__ H, int64_t ldh, const double *__restrict__ J, int64_t ldj,
    const int *__restrict__ idxI, int nI, int m, double lamb, double delta, int *__restrict__ zero,
    int nzero, const double *__restrict__ row_src, double *__restrict__ row_dst, int row_n,
    const double *__restrict__ G, int64_t ldg, double ginv) {
  if (blockIdx.y == 0) {
    if (zero && blockIdx.x == 0)
      for (int t = threadIdx.x; t < nzero; t += 256) zero[t] = 0;
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (row_src && j < row_n) row_dst[j] = row_src[j];
  }
  b_assemble_kkt<ASM_ROWS, true>(blockIdx.x, blockIdx.y, threadIdx.x, K, ldk, H, ldh, J, ldj, idxI, nI, m, lamb, delta, G, ldg, ginv);
}

// The head of a step whose assembly runs beside the first diagonal chain (LdltHead,
// pgf_ldlt.h): only the row groups of the first diagonal block, rows [0, min(256, N)) -- one
// column block --, the zeroing of the factorisation's words, which the chain's own launch cannot
// do for itself, and the rhs row, copied by all workgroups together.  Grid (1, row groups).
template <bool GRAM>
__global__ __launch_bounds__(256) void k_assemble_kkt_head(double *__restrict__ K, int64_t ldk,
    const double *__restrict__ H, int64_t ldh, const double *__restrict__ J, int64_t ldj,
    const int *__restrict__ idxI, int nI, int m, double lamb, double delta, int *__restrict__ zero,
    int nzero, const double *__restrict__ row_src, double *__restrict__ row_dst, int row_n,
    const double *__restrict__ G, int64_t ldg, double ginv) {
  if (zero && blockIdx.y == 0)
    for (int t = threadIdx.x; t < nzero; t += 256) zero[t] = 0;
  if (row_src)
    for (int j = blockIdx.y * 256 + threadIdx.x; j < row_n; j += gridDim.y * 256) row_dst[j] = row_src[j];
  b_assemble_kkt<ASM_ROWS, GRAM>(0, blockIdx.y, threadIdx.x, K, ldk, H, ldh, J, ldj, idxI, nI, m, lamb, delta, G,
                                 ldg, ginv);
}

__global__ void k_copy(double *__restrict__ dst, const double *__restrict__ src, int n) {
  b_copy(dst, src, n);
}

__global__ void k_copy_u8(uint8_t *__restrict__ dst, const uint8_t *__restrict__ src, int n) {
  b_copy_u8(dst, src, n);
}

__global__ void k_mask_diff(int n, const uint8_t *__restrict__ a, const uint8_t *__restrict__ b,
    int *__restrict__ out) {
  b_mask_diff(n, a, b, out);
}

// (last_block_reduce: pgf_step_dev.h)

// A handle without a finite bound (pgf_solver::unb): what k_mask_compact writes for an empty active
// set, whatever the point -- mask 0, idxI = pos = the identity, counts (n, 0, ., 0) -- written once
__global__ __launch_bounds__(256) void k_unbounded_sets(int n, uint8_t *__restrict__ mask,
    int *__restrict__ idxI, int *__restrict__ pos, int *__restrict__ counts) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < n) {
    mask[j] = 0;
    idxI[j] = j;
    pos[j] = j;
  }
  if (j == 0) {
    counts[0] = n;
    counts[1] = 0;
    counts[3] = 0;
  }
}

// Optional extras of the step-update launch (StepExtras, nullptr members are skipped):
//   v, lv      the residual check's expansion of the solution (k_expand_sol)
//   zero3      words cleared before the residual check's atomics (red3)
//   flags_src  -> status[0, 4): the factorisation's flag words;  chain_src -> status[3]: the
//              chained solve's status word (both copied by the last workgroup, so the host reads
//              them with the rest of the step's status block)
//   cy_partial the condensed step's s_y formed by the y rows themselves (StepCondY, in place of
//              k_cond_y in front of this launch) and stored to cy_sol = sol + nI
struct StepExtras {
  double lamb;
  double *v, *lv, *zero3;
  const int *flags_src, *chain_src;
  int *status;
  unsigned *ticket;
  const double *cy_partial, *cy_rhs;
  double *cy_sol;
  double cy_delta;
  int cy_parts;
};
// k_cond_y's value for row r in one lane: the chunks p = g, g + 4, ... summed in four sequential
// groups, combined as ((g0 + g1) + (g2 + g3)), the same expression after that
__device__ __forceinline__ double cond_y_row(int m, int nparts, const double *__restrict__ partial,
                                             const double *__restrict__ rhs_y, double delta, int r) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  const double *col = partial + r;
  int p = 0;
#pragma unroll 8
  for (; p + 3 < nparts; p += 4) {
    s0 += col[(int64_t)p * m];
    s1 += col[(int64_t)(p + 1) * m];
    s2 += col[(int64_t)(p + 2) * m];
    s3 += col[(int64_t)(p + 3) * m];
  }
  if (p < nparts) s0 += col[(int64_t)p * m];
  if (p + 1 < nparts) s1 += col[(int64_t)(p + 1) * m];
  if (p + 2 < nparts) s2 += col[(int64_t)(p + 2) * m];
  return (((s0 + s1) + (s2 + s3)) - rhs_y[r]) / delta;
}
__global__ __launch_bounds__(256) void k_step_update(int n, int m, int nI, double fact,
    double rho, const double *__restrict__ x, const double *__restrict__ y,
    const double *__restrict__ lb, const double *__restrict__ ub,
    const uint8_t *__restrict__ mask, const int *__restrict__ pos,
    const double *__restrict__ b0full, const double *__restrict__ F,
    const double *__restrict__ sol, double *__restrict__ dx, double *__restrict__ dy,
    double *__restrict__ xn, double *__restrict__ yn, double *__restrict__ red,
    double *__restrict__ diff_out, StepExtras ex) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  double sy = 0.0;
  if (ex.cy_partial && i >= n && i < n + m) {
    sy = cond_y_row(m, ex.cy_parts, ex.cy_partial, ex.cy_rhs, ex.cy_delta, i - n);
    ex.cy_sol[i - n] = sy;  // (the residual check reads it)
  }
  b_step_update(n, m, nI, fact, rho, x, y, lb, ub, mask, pos, b0full, F, sol, dx, dy, xn, yn, red,
                ex.cy_partial != nullptr, sy);
  if (ex.v && i < n) {
    const double val = mask[i] ? 0.0 : sol[pos[i]];
    ex.v[i] = val;
    ex.lv[i] = ex.lamb * val;
  }
  if (ex.zero3 && blockIdx.x == 0 && threadIdx.x < 3) ex.zero3[threadIdx.x] = 0.0;
  if (!last_block_reduce(red, gridDim.x, diff_out, ex.ticket)) return;
  if (threadIdx.x < 4) {
    int w = ex.flags_src ? ex.flags_src[threadIdx.x] : 0;
    if (threadIdx.x == 3 && ex.chain_src) w = *ex.chain_src;
    if (ex.flags_src || (threadIdx.x == 3 && ex.chain_src)) ex.status[threadIdx.x] = w;
  }
}

__global__ __launch_bounds__(256) void k_unscaled_res_norm(int n, int m, double dt,
    const double *__restrict__ xhat, const double *__restrict__ yhat,
    const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ g,
    const double *__restrict__ c, const double *__restrict__ lb, const double *__restrict__ ub,
    double *__restrict__ red, double *__restrict__ out, double *__restrict__ out2,
    unsigned *__restrict__ ticket) {
  b_unscaled_res_sq(n, m, dt, xhat, yhat, x, y, g, c, lb, ub, red);
  if (last_block_reduce(red, gridDim.x, out, ticket) && out2 && threadIdx.x == 0) out2[0] = out[0];
}

__global__ __launch_bounds__(256) void k_final_reduce(const double *__restrict__ red, int cnt,
    double *__restrict__ out, int take_sqrt) {
  b_final_reduce(red, cnt, out, take_sqrt);
}

__global__ __launch_bounds__(256) void k_gemv_rows(int rows, int cols,
    const double *__restrict__ M, int64_t ld, const double *__restrict__ v,
    const double *__restrict__ add, double sgn, double *__restrict__ out) {
  b_gemv_rows(rows, cols, M, ld, v, add, sgn, out);
}

__global__ __launch_bounds__(256) void k_gemvT_partial(int rows, int cols,
    const double *__restrict__ M, int64_t ld, const double *__restrict__ w, int chunk,
    double *__restrict__ partial) {
  b_gemvT_partial(rows, cols, M, ld, w, chunk, partial);
}

__global__ void k_sum_partials(int cols, int nparts, const double *__restrict__ partial,
    const double *__restrict__ base, double *__restrict__ out) {
  b_sum_partials(cols, nparts, partial, base, out);
}

__global__ void k_mult_vec(int m, double rho, const double *__restrict__ c,
    const double *__restrict__ y, double *__restrict__ w) {
  b_mult_vec(m, rho, c, y, w);
}

// ---------------------------------------------------------------- launch wrappers
void launch_scale_bounds(hipStream_t s, int n, double lamb, const double *lb, const double *ub,
                         double *slb, double *sub) {
  if (n) hipLaunchKernelGGL(k_scale_bounds, g1(n), dim3(256), 0, s, n, lamb, lb, ub, slb, sub);
}

void launch_active_set(hipStream_t s, int n, int use_tau, double lamb, double f_x, double f_x0,
                       double f_d, const double *xhat, const double *x, const double *g,
                       const double *slb, const double *sub, uint8_t *mask) {
  if (n)
    hipLaunchKernelGGL(k_active_set, g1(n), dim3(256), 0, s, n, use_tau, lamb, f_x, f_x0, f_d,
                       xhat, x, g, slb, sub, mask);
}

void launch_compact(hipStream_t s, int n, const uint8_t *mask, int *idxI, int *idxA, int *pos,
                    int *counts, int expect) {
  hipLaunchKernelGGL(k_compact, dim3(1), dim3(1024), 0, s, n, mask, idxI, idxA, pos, counts, expect);
}

void launch_mask_compact(hipStream_t s, int n, int use_tau, double lamb, double f_x, double f_x0,
                         double f_d, const double *xhat, const double *x, const double *g,
                         const double *slb, const double *sub, uint8_t *mask, int *idxI, int *idxA,
                         int *pos, int *counts, int expect) {
  const ActiveArgs a{use_tau, lamb, f_x, f_x0, f_d, xhat, x, g, slb, sub};
  hipLaunchKernelGGL(k_mask_compact, dim3(1), dim3(1024), 0, s, n, a, mask, idxI, idxA, pos, counts,
                     expect);
}

void launch_mask_compact_rhs(hipStream_t s, int n, int m, int nI, int use_tau, double lamb, double f_x,
                             double f_x0, double f_d, double dt, double fact, const double *xhat,
                             const double *yhat, const double *x, const double *y, const double *g,
                             const double *c, const double *slb, const double *sub, uint8_t *mask, int *idxI,
                             int *idxA, int *pos, int *counts, int expect, double *F, double *b0full,
                             double *rhs) {
  const ActiveArgs a{use_tau, lamb, f_x, f_x0, f_d, xhat, x, g, slb, sub};
  hipLaunchKernelGGL(k_mask_compact_rhs, dim3(1), dim3(1024), 0, s, n, a, mask, idxI, idxA, pos, counts, expect,
                     m, nI, dt, fact, yhat, y, c, F, b0full, rhs);
}

void launch_unbounded_sets(hipStream_t s, int n, uint8_t *mask, int *idxI, int *pos, int *counts) {
  hipLaunchKernelGGL(k_unbounded_sets, dim3(n ? (n + 255) / 256 : 1), dim3(256), 0, s, n, mask, idxI, pos, counts);
}

void launch_advance_outer(hipStream_t s, int n, int m, double lamb, const double *x, const double *y,
                          const double *lb, const double *ub, double *xhat, double *yhat, double *slb,
                          double *sub) {
  const int k = std::max(n, m);
  if (k) hipLaunchKernelGGL(k_advance_outer, g1(k), dim3(256), 0, s, n, m, lamb, x, y, lb, ub, xhat, yhat, slb, sub);
}

void launch_residual(hipStream_t s, int n, int m, double lamb, double dt, const double *xhat,
                     const double *yhat, const double *x, const double *y, const double *g,
                     const double *c, const double *slb, const double *sub, const uint8_t *mask,
                     double *F, double *b0full) {
  if (n + m)
    hipLaunchKernelGGL(k_residual, g1(n + m), dim3(256), 0, s, n, m, lamb, dt, xhat, yhat, x, y,
                       g, c, slb, sub, mask, F, b0full);
}

void launch_residual_rhs(hipStream_t s, int n, int m, int nI, double lamb, double dt, double fact,
                         const double *xhat, const double *yhat, const double *x, const double *y,
                         const double *g, const double *c, const double *slb, const double *sub,
                         const uint8_t *mask, const int *idxI, double *F, double *b0full, double *rhs) {
  const int nb = std::max((n + m + 255) / 256, (nI + m + 3) / 4);
  if (nb)
    hipLaunchKernelGGL(k_residual_rhs, dim3(nb), dim3(256), 0, s, n, m, nI, lamb, dt, fact, xhat, yhat, x, y,
                       g, c, slb, sub, mask, idxI, F, b0full, rhs);
}

void launch_reduced_rhs(hipStream_t s, int n, int m, int nI, int nA, double fact, const double *F,
                        const int *idxI, const int *idxA, const double *H, int64_t ldh, const double *J,
                        int64_t ldj, const double *b0full, double *partial, int nparts, double *rhs) {
  const int N = nI + m;
  if (!N) return;
  if (nA > 0 && nI > 0)
    hipLaunchKernelGGL(k_active_rows_partial, dim3((n + 255) / 256, nparts), dim3(256), 0, s, n, nA, idxA,
                       H, ldh, b0full, nparts, partial);
  hipLaunchKernelGGL(k_reduced_rhs, dim3((N + 3) / 4), dim3(256), 0, s, n, m, nI, nA, fact, F, idxI, J,
                     ldj, b0full, partial, nparts, rhs);
}

void launch_assemble_kkt(hipStream_t s, double *K, int64_t ldk, const double *H, int64_t ldh,
                         const double *J, int64_t ldj, const int *idxI, int nI, int m,
                         double lamb, double delta, int *zero, int nzero, const double *row_src,
                         double *row_dst, int row_n, const double *G, int64_t ldg) {
  const int N = nI + m;
  if (!N) return;
  const dim3 grid((N + 255) / 256, (N + ASM_ROWS - 1) / ASM_ROWS);
  if (G)
    hipLaunchKernelGGL(k_assemble_kkt_gram, grid, dim3(256), 0, s, K, ldk, H, ldh, J, ldj, idxI, nI, m, lamb,
                       delta, zero, nzero, row_src, row_dst, std::min(row_n, N), G, ldg, 1.0 / delta);
  else
    hipLaunchKernelGGL(k_assemble_kkt, grid, dim3(256), 0, s, K, ldk, H, ldh, J, ldj, idxI, nI, m, lamb, delta,
                       zero, nzero, row_src, row_dst, std::min(row_n, N));
}

void launch_assemble_kkt_head(hipStream_t s, double *K, int64_t ldk, const LdltHead &hw, int *zero, int nzero) {
  const int N = hw.nI + hw.m;
  if (!N) return;
  const dim3 grid(1, (std::min(N, LDLT_OB) + ASM_ROWS - 1) / ASM_ROWS);
  if (hw.G)
    hipLaunchKernelGGL(k_assemble_kkt_head<true>, grid, dim3(256), 0, s, K, ldk, hw.H, hw.ldh, hw.J, hw.ldj,
                       hw.idxI, hw.nI, hw.m, hw.lamb, hw.delta, zero, nzero, hw.row_src, hw.row_dst,
                       std::min(hw.row_n, N), hw.G, hw.ldg, 1.0 / hw.delta);
  else
    hipLaunchKernelGGL(k_assemble_kkt_head<false>, grid, dim3(256), 0, s, K, ldk, hw.H, hw.ldh, hw.J, hw.ldj,
                       hw.idxI, hw.nI, hw.m, hw.lamb, hw.delta, zero, nzero, hw.row_src, hw.row_dst,
                       std::min(hw.row_n, N), (const double *)nullptr, (int64_t)0, 0.0);
}

void launch_copy(hipStream_t s, double *dst, const double *src, int n) {
  if (n) hipLaunchKernelGGL(k_copy, g1(n), dim3(256), 0, s, dst, src, n);
}

void launch_copy_u8(hipStream_t s, uint8_t *dst, const uint8_t *src, int n) {
  if (n) hipLaunchKernelGGL(k_copy_u8, g1(n), dim3(256), 0, s, dst, src, n);
}

void launch_mask_diff(hipStream_t s, int n, const uint8_t *a, const uint8_t *b, int *out) {
  if (n) hipLaunchKernelGGL(k_mask_diff, g1(n), dim3(256), 0, s, n, a, b, out);
}

int step_update_blocks(int n, int m) { return (n + m + 255) / 256; }

void launch_step_update(hipStream_t s, int n, int m, int nI, double fact, double rho,
                        const double *x, const double *y, const double *lb, const double *ub,
                        const uint8_t *mask, const int *pos, const double *b0full,
                        const double *F, const double *sol, double *dx, double *dy, double *xn,
                        double *yn, double *red, double *diff_out, unsigned *ticket, double lamb,
                        double *v, double *lv, double *zero3, const int *flags_src,
                        const int *chain_src, int *status, const StepCondY *cy) {
  const int nb = step_update_blocks(n, m);
  StepExtras ex{lamb, v, lv, zero3, flags_src, chain_src, status, ticket, nullptr, nullptr, nullptr, 0.0, 0};
  if (cy && m) {
    ex.cy_partial = cy->partial;
    ex.cy_rhs = cy->rhs_y;
    ex.cy_sol = cy->sol_y;
    ex.cy_delta = cy->delta;
    ex.cy_parts = cy->nparts;
  }
  if (nb) {
    hipLaunchKernelGGL(k_step_update, dim3(nb), dim3(256), 0, s, n, m, nI, fact, rho, x, y, lb, ub,
                       mask, pos, b0full, F, sol, dx, dy, xn, yn, red, diff_out, ex);
    return;
  }
  hipLaunchKernelGGL(k_final_reduce, dim3(1), dim3(256), 0, s, red, nb, diff_out, 1);
}

void launch_gemv_rows(hipStream_t s, int rows, int cols, const double *M, int64_t ld,
                      const double *v, const double *add, double sgn, double *out) {
  if (rows)
    hipLaunchKernelGGL(k_gemv_rows, dim3((rows + 3) / 4), dim3(256), 0, s, rows, cols, M, ld, v,
                       add, sgn, out);
}

void launch_gemvT(hipStream_t s, int rows, int cols, const double *M, int64_t ld,
                  const double *w, const double *base, double *partial, int nparts, double *out) {
  // out = base + M' w, in nparts fixed row chunks
  if (!cols) return;
  if (rows == 0) {
    launch_copy(s, out, base, cols);
    return;
  }
  const int chunk = (rows + nparts - 1) / nparts;
  const int used = (rows + chunk - 1) / chunk;
  hipLaunchKernelGGL(k_gemvT_partial, dim3((cols + 255) / 256, used), dim3(256), 0, s, rows, cols,
                     M, ld, w, chunk, partial);
  hipLaunchKernelGGL(k_sum_partials, g1(cols), dim3(256), 0, s, cols, used, partial, base, out);
}

void launch_mult_vec(hipStream_t s, int m, double rho, const double *c, const double *y,
                     double *w) {
  if (m) hipLaunchKernelGGL(k_mult_vec, g1(m), dim3(256), 0, s, m, rho, c, y, w);
}

void launch_unscaled_res_norm(hipStream_t s, int n, int m, double dt, const double *xhat,
                              const double *yhat, const double *x, const double *y,
                              const double *g, const double *c, const double *lb,
                              const double *ub, double *red, double *out, double *out2,
                              unsigned *ticket) {
  const int nb = (n + m + 255) / 256;
  if (nb) {
    hipLaunchKernelGGL(k_unscaled_res_norm, dim3(nb), dim3(256), 0, s, n, m, dt, xhat, yhat, x, y, g,
                       c, lb, ub, red, out, out2, ticket);
    return;
  }
  hipLaunchKernelGGL(k_final_reduce, dim3(1), dim3(256), 0, s, red, nb, out, 1);
  if (out2) (void)hipMemcpyAsync(out2, out, sizeof(double), hipMemcpyDeviceToDevice, s);
}

void launch_final_reduce(hipStream_t s, const double *red, int cnt, double *out, int take_sqrt) {
  hipLaunchKernelGGL(k_final_reduce, dim3(1), dim3(256), 0, s, red, cnt, out, take_sqrt);
}

__global__ __launch_bounds__(256) void k_measures(int n, int m, double active_tol,
                                                  const double *__restrict__ x,
                                                  const double *__restrict__ y,
                                                  const double *__restrict__ r,
                                                  const double *__restrict__ c,
                                                  const double *__restrict__ lb,
                                                  const double *__restrict__ ub,
                                                  double *__restrict__ red) {
  b_measures(n, m, active_tol, x, y, r, c, lb, ub, red);
}

__global__ __launch_bounds__(256) void k_measures_final(const double *__restrict__ red, int nb,
                                                        double *__restrict__ out) {
  b_measures_final(red, nb, out);
}

void launch_measures(hipStream_t s, int n, int m, double active_tol, const double *x,
                     const double *y, const double *r, const double *c, const double *lb,
                     const double *ub, double *red, double *out) {
  const int nb = (n + m + 255) / 256;
  if (nb)
    hipLaunchKernelGGL(k_measures, dim3(nb), dim3(256), 0, s, n, m, active_tol, x, y, r, c, lb, ub,
                       red);
  hipLaunchKernelGGL(k_measures_final, dim3(1), dim3(256), 0, s, red, nb, out);
}

// ---------------------------------------------------------------- CSR -> dense (plugin path)
// dst (rows x ld, zeroed beforehand) += CSR entries; one wavefront per row.  Duplicate entries
// of a row are summed in storage order by lane 0 ... in practice scipy's canonical CSR has
// none, and a plain store per entry would drop them silently, so entries are accumulated.
__global__ __launch_bounds__(256) void k_csr_to_dense(int rows, const int *__restrict__ ptr,
                                                      const int *__restrict__ idx,
                                                      const double *__restrict__ val,
                                                      double *__restrict__ dst, int64_t ld) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const int p0 = ptr[r], p1 = ptr[r + 1];
  double *row = dst + (int64_t)r * ld;
  for (int p = p0 + lane; p < p1; p += 64) atomicAdd(row + idx[p], val[p]);
}

void launch_csr_to_dense(hipStream_t s, int rows, const int *ptr, const int *idx, const double *val,
                         double *dst, int64_t ld) {
  if (rows)
    hipLaunchKernelGGL(k_csr_to_dense, dim3((rows + 3) / 4), dim3(256), 0, s, rows, ptr, idx, val,
                       dst, ld);
}

// ---------------------------------------------------------------- condensed KKT system
// With the constraint block -delta I eliminated first (block elimination of
// [[H[I,I] + lamb I, J_I^T], [J_I, -delta I]], the reference's SymmetricStepSolver matrix,
// step/solver/symmetric_step_solver.py:35-76) what is factorised is the nI x nI Schur complement
//     S = H[I,I] + lamb I + J_I^T J_I / delta,
// applied by the factorisation itself from the panel V = J_I^T (nI x m, row-major, zero-padded to
// a multiple of 32 columns) with D-scaling vd = -1 / delta (DenseLdlt::V, pgf_factor2.hip).
// Row nI of V carries the constraint rows of the right-hand side, so that the elimination turns
// row nI of K (b_x) into b_x + J_I^T b_y / delta on the way.
//   S s_x = b_x + J_I^T b_y / delta,      s_y = (J_I s_x - b_y) / delta.

// (b_cond_tail and the tile body: pgf_head_dev.h)
__global__ __launch_bounds__(256) void k_cond_panel(double *__restrict__ V, int64_t ldv, int mp,
                                                    const double *__restrict__ J, int64_t ldj,
                                                    const int *__restrict__ idxI, int nI, int m,
                                                    double *__restrict__ vd, const double *__restrict__ rhs_y,
                                                    double delta) {
  __shared__ CondTile tile;
  b_cond_panel_load(tile, blockIdx.x, blockIdx.y, threadIdx.x, V, ldv, mp, J, ldj, idxI, nI, m, vd, rhs_y, delta);
  __syncthreads();
  b_cond_panel_store(tile, blockIdx.x, blockIdx.y, threadIdx.x, V, ldv, mp, nI);
}

// row nI of V <- the constraint part of the right-hand side (or zeros), vd <- -1 / delta
__global__ void k_cond_tail(double *__restrict__ Vrow, double *__restrict__ vd, int mp, int m,
                            const double *__restrict__ rhs_y, double delta) {
  b_cond_tail(Vrow, vd, blockIdx.x * blockDim.x + threadIdx.x, mp, m, rhs_y, delta);
}

// out[i] = rhs[i] + dot(V[i][0:m], rhs[nI:nI+m]) / delta
__global__ __launch_bounds__(256) void k_cond_rhs(int nI, int m, const double *__restrict__ V, int64_t ldv,
                                                  const double *__restrict__ rhs, double delta,
                                                  double *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nI) return;
  const double d = row_dot(V + (int64_t)i * ldv, rhs + nI, m, lane);
  if (lane == 0) out[i] = rhs[i] + d / delta;
}

// sol_y[r] = (sum_p partial[p][r] - rhs_y[r]) / delta   (partial: V^T s_x in fixed row chunks);
// 64 columns per workgroup, four groups of lanes take the chunks p = g, g + 4, ... and are summed
// in a fixed order
__global__ __launch_bounds__(256) void k_cond_y(int m, int nparts, const double *__restrict__ partial,
                                                const double *__restrict__ rhs_y, double delta,
                                                double *__restrict__ sol_y) {
  __shared__ double part[4][64];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int r = blockIdx.x * 64 + c;
  double s = 0.0;
  if (r < m)
    for (int p = g; p < nparts; p += 4) s += partial[(int64_t)p * m + r];
  part[g][c] = s;
  __syncthreads();
  if (g == 0 && r < m) sol_y[r] = (((part[0][c] + part[1][c]) + (part[2][c] + part[3][c])) - rhs_y[r]) / delta;
}

void launch_cond_panel(hipStream_t s, double *V, int64_t ldv, int mp, double *vd, const double *J,
                       int64_t ldj, const int *idxI, int nI, int m, double delta, const double *rhs_y) {
  if (nI > 0 && mp > 0)
    hipLaunchKernelGGL(k_cond_panel, dim3((nI + 31) / 32, mp / 32), dim3(256), 0, s, V, ldv, mp, J, ldj,
                       idxI, nI, m, vd, rhs_y, delta);
  else if (mp > 0)
    hipLaunchKernelGGL(k_cond_tail, g1(mp), dim3(256), 0, s, V + (int64_t)nI * ldv, vd, mp, m, rhs_y, delta);
}

void launch_cond_rhs(hipStream_t s, int nI, int m, const double *V, int64_t ldv, const double *rhs,
                     double delta, double *out) {
  if (nI) hipLaunchKernelGGL(k_cond_rhs, dim3((nI + 3) / 4), dim3(256), 0, s, nI, m, V, ldv, rhs, delta, out);
}

int launch_cond_y_partial(hipStream_t s, int nI, int m, const double *V, int64_t ldv, const double *solx,
                          double *partial, size_t partial_cap) {
  if (!m) return 0;
  // as many row chunks as the scratch holds (up to 128): the product reads V once, 8 m nI bytes
  const int nparts = (int)std::max<size_t>(1, std::min<size_t>(128, partial_cap / (size_t)m));
  const int chunk = (std::max(nI, 1) + nparts - 1) / nparts;
  const int used = nI > 0 ? (nI + chunk - 1) / chunk : 0;
  if (used)
    hipLaunchKernelGGL(k_gemvT_partial, dim3((m + 255) / 256, used), dim3(256), 0, s, nI, m, V, ldv, solx,
                       chunk, partial);
  return used;
}

void launch_cond_y(hipStream_t s, int nI, int m, const double *V, int64_t ldv, const double *solx,
                   const double *rhs_y, double delta, double *partial, size_t partial_cap, double *sol_y) {
  if (!m) return;
  const int used = launch_cond_y_partial(s, nI, m, V, ldv, solx, partial, partial_cap);
  hipLaunchKernelGGL(k_cond_y, dim3((m + 63) / 64), dim3(256), 0, s, m, used, partial, rhs_y, delta, sol_y);
}
