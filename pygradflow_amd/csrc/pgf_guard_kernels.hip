// The residual guard of the single-handle step and the evaluation ahead: r = rhs - K s with K applied
// from H, J and the mask, alone (launch_kkt_residual) or in the same matrix passes as g, c at the
// new point (launch_residual_and_eval, launch_residual_and_eval_fused); the matrix norms of the
// guard's normwise backward error; axpy and symmetrize for the refinement and the LU fallback.
// Launch declarations: pgf_kernels.h.  Compiled with -ffp-contract=off like the step kernels it
// shares dot products with (pgf_reduce_dev.h).
#include "pgf_kernels.h"
#include "pgf_reduce_dev.h"
#include "pgf_step_dev.h"

// ---------------------------------------------------------------- residual of the reduced system
// v <- the reduced solution's variable part scattered to the full index set (zero on the
// active set), lv <- lambda v
__global__ void k_expand_sol(int n, int nI, const int *__restrict__ pos, const uint8_t *__restrict__ mask,
                             const double *__restrict__ sol, double lamb, double *__restrict__ v,
                             double *__restrict__ lv) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const double val = mask[j] ? 0.0 : sol[pos[j]];
  v[j] = val;
  lv[j] = lamb * val;
}

// r = rhs - K s from u = H v + lambda v + J' s_y (full length n) and wy = J v - delta s_y;
// red[0..2] <- max |r|, max |rhs|, max |s| (bit patterns of non-negative doubles order like
// integers; red zeroed by the caller)
__global__ __launch_bounds__(256) void k_kkt_residual(int N, int nI, const int *__restrict__ idxI,
                                                      const double *rhs,  // may alias r
                                                      const double *__restrict__ sol,
                                                      const double *__restrict__ u,
                                                      const double *__restrict__ wy, double *r,
                                                      unsigned long long *__restrict__ red) {
  __shared__ double sh[3][256];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double ar = 0.0, ab = 0.0, as = 0.0;
  if (i < N) {
    const double ks = i < nI ? u[idxI[i]] : wy[i - nI];
    const double ri = rhs[i] - ks;
    r[i] = ri;
    ar = fabs(ri);
    ab = fabs(rhs[i]);
    as = fabs(sol[i]);
    if (ar != ar) ar = __builtin_inf();  // a NaN must not vanish in the max
  }
  sh[0][threadIdx.x] = ar;
  sh[1][threadIdx.x] = ab;
  sh[2][threadIdx.x] = as;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o)
      for (int q = 0; q < 3; ++q)
        sh[q][threadIdx.x] = fmax(sh[q][threadIdx.x], sh[q][threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x < 3) atomicMax(&red[threadIdx.x], (unsigned long long)__double_as_longlong(sh[threadIdx.x][0]));
}

__global__ void k_axpy1(int N, const double *__restrict__ d, double *__restrict__ s) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) s[i] += d[i];
}

// full symmetric matrix from its lower triangle (LU fallback of the reduced KKT system)
__global__ void k_symmetrize(double *__restrict__ A, int64_t ld, int N) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
  if (i < N && j < N && j > i) A[(int64_t)i * ld + j] = A[(int64_t)j * ld + i];
}

void launch_kkt_residual(hipStream_t s, int n, int m, int nI, double lamb, double delta,
                         const double *H, int64_t ldh, const double *J, int64_t ldj,
                         const int *idxI, const int *pos, const uint8_t *mask, const double *rhs,
                         const double *sol, double *v, double *lv, double *u, double *wy,
                         double *partial, int nparts, double *r, double *red3, bool prepared) {
  const int N = nI + m;
  if (!prepared) (void)hipMemsetAsync(red3, 0, 3 * sizeof(double), s);
  if (N == 0) return;
  if (n && !prepared) hipLaunchKernelGGL(k_expand_sol, g1(n), dim3(256), 0, s, n, nI, pos, mask, sol, lamb, v, lv);
  // u = H v + (lambda v + J' s_y)
  launch_gemvT(s, m, n, J, ldj, sol + nI, lv, partial, nparts, u);
  launch_gemv_rows(s, n, n, H, ldh, v, u, 1.0, lv);  // lv is free again: it receives H v + u
  // wy = J v - delta s_y
  launch_gemv_rows(s, m, n, J, ldj, v, sol + nI, -delta, wy);
  hipLaunchKernelGGL(k_kkt_residual, g1(N), dim3(256), 0, s, N, nI, idxI, rhs, sol, lv, wy, r,
                     reinterpret_cast<unsigned long long *>(red3));
}

// ---- residual check of this step's solve AND g, c at the new point in one pass over H and J ----
// The check applies K from H, J and the mask to the solution; the next step's evaluation applies
// the same matrices to the new point: streamed separately they read H once and J twice EACH
// (336 MB at config 2).  Two right-hand vectors per matrix pass instead: every dot product is the
// row_dot / b_gemvT_partial arithmetic of the separate kernels, in the same order (bit-identical
// g, c and residual), the matrices are read once.
__device__ __forceinline__ void row_dot2(const double *__restrict__ row, const double *__restrict__ v1,
                                         const double *__restrict__ v2, int cols, int lane, double &d1,
                                         double &d2) {
  double a1 = 0.0, a2 = 0.0;
  int j = lane * 2;
  if ((((uintptr_t)row) & 15) == 0) {
    for (; j + 1 < cols; j += 128) {
      const double2 a = *reinterpret_cast<const double2 *>(row + j);
      const double2 b1 = *reinterpret_cast<const double2 *>(v1 + j);
      const double2 b2 = *reinterpret_cast<const double2 *>(v2 + j);
      a1 = fma(a.x, b1.x, a1);
      a1 = fma(a.y, b1.y, a1);
      a2 = fma(a.x, b2.x, a2);
      a2 = fma(a.y, b2.y, a2);
    }
    if (j < cols) {
      a1 = fma(row[j], v1[j], a1);
      a2 = fma(row[j], v2[j], a2);
    }
  } else {
    for (j = lane; j < cols; j += 64) {
      a1 = fma(row[j], v1[j], a1);
      a2 = fma(row[j], v2[j], a2);
    }
  }
  d1 = wave_sum(a1);
  d2 = wave_sum(a2);
}
// out1 = M v1 + sgn1 add1, out2 = M v2 + sgn2 add2 (b_gemv_rows twice, one read of M)
__global__ __launch_bounds__(256) void k_gemv_rows2(int rows, int cols, const double *__restrict__ M, int64_t ld,
                                                    const double *__restrict__ v1, const double *__restrict__ add1,
                                                    double sgn1, double *__restrict__ out1,
                                                    const double *__restrict__ v2, const double *__restrict__ add2,
                                                    double sgn2, double *__restrict__ out2) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  double d1, d2;
  row_dot2(M + (int64_t)r * ld, v1, v2, cols, lane, d1, d2);
  if (lane == 0) {
    out1[r] = d1 + sgn1 * add1[r];
    out2[r] = d2 + sgn2 * add2[r];
  }
}
// partial1[rb][j] = sum_{r in chunk rb} M[r][j] w1[r], partial2 likewise with w2
// w1 = rho c + y1 (b_mult_vec's expression) is formed here, row by row, and stored by the first
// column of workgroups
__global__ __launch_bounds__(256) void k_gemvT_partial2(int rows, int cols, const double *__restrict__ M,
                                                        int64_t ld, double rho, const double *__restrict__ c,
                                                        const double *__restrict__ y1, double *__restrict__ w1,
                                                        const double *__restrict__ w2, int chunk,
                                                        double *__restrict__ partial1,
                                                        double *__restrict__ partial2) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  const int r0 = blockIdx.y * chunk;
  const int r1 = min(rows, r0 + chunk);
  if (blockIdx.x == 0)
    for (int r = r0 + (int)threadIdx.x; r < r1; r += 256) w1[r] = rho * c[r] + y1[r];
  if (j >= cols) return;
  double a1 = 0.0, a2 = 0.0;
  for (int r = r0; r < r1; ++r) {
    const double mv = M[(int64_t)r * ld + j];
    a1 = fma(mv, rho * c[r] + y1[r], a1);
    a2 = fma(mv, w2[r], a2);
  }
  partial1[(int64_t)blockIdx.y * cols + j] = a1;
  partial2[(int64_t)blockIdx.y * cols + j] = a2;
}
__global__ void k_sum_partials2(int cols, int nparts, const double *__restrict__ partial1,
                                const double *__restrict__ base1, double *__restrict__ out1,
                                const double *__restrict__ partial2, const double *__restrict__ base2,
                                double *__restrict__ out2) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cols) return;
  double s1 = 0.0, s2 = 0.0;
  for (int p = 0; p < nparts; ++p) {
    s1 += partial1[(int64_t)p * cols + j];
    s2 += partial2[(int64_t)p * cols + j];
  }
  out1[j] = base1[j] + s1;
  out2[j] = base2[j] + s2;
}

// launch_kkt_residual (solution sol of the system rhs; r, red3 as there) and the evaluation
//   c = J xn - b ; w = rho c + yn ; tmpn = q + J' w ; g = H xn + tmpn
// at the point (xn, yn) the step update has just produced.  partial: 2 * nparts * n doubles.
void launch_residual_and_eval(hipStream_t s, int n, int m, int nI, double lamb, double delta, const double *H,
                              int64_t ldh, const double *J, int64_t ldj, const int *idxI, const int *pos,
                              const uint8_t *mask, const double *rhs, const double *sol, double *v, double *lv,
                              double *u, double *wy, double *partial, int nparts, double *r, double *red3,
                              const double *xn, const double *yn, const double *b, const double *q, double rho,
                              double *c, double *w, double *tmpn, double *g, bool prepared) {
  const int N = nI + m;
  if (!prepared) (void)hipMemsetAsync(red3, 0, 3 * sizeof(double), s);
  if (n && !prepared) hipLaunchKernelGGL(k_expand_sol, g1(n), dim3(256), 0, s, n, nI, pos, mask, sol, lamb, v, lv);
  // one pass over J: c = J xn - b, wy = J v - delta s_y
  if (m)
    hipLaunchKernelGGL(k_gemv_rows2, dim3((m + 3) / 4), dim3(256), 0, s, m, n, J, ldj, xn, b, -1.0, c, v,
                       sol + nI, -delta, wy);
  // one pass over J (transposed): tmpn = q + J' w, u = lambda v + J' s_y (w = rho c + yn formed on the way)
  if (n == 0) launch_mult_vec(s, m, rho, c, yn, w);
  if (n) {
    if (m == 0) {
      launch_copy(s, tmpn, q, n);
      launch_copy(s, u, lv, n);
    } else {
      const int chunk = (m + nparts - 1) / nparts;
      const int used = (m + chunk - 1) / chunk;
      double *p2 = partial + (size_t)nparts * n;
      hipLaunchKernelGGL(k_gemvT_partial2, dim3((n + 255) / 256, used), dim3(256), 0, s, m, n, J, ldj, rho, c,
                         yn, w, sol + nI, chunk, partial, p2);
      hipLaunchKernelGGL(k_sum_partials2, g1(n), dim3(256), 0, s, n, used, partial, q, tmpn, p2, lv, u);
    }
    // one pass over H: g = H xn + tmpn, lv <- H v + u
    hipLaunchKernelGGL(k_gemv_rows2, dim3((n + 3) / 4), dim3(256), 0, s, n, n, H, ldh, xn, tmpn, 1.0, g, v, u,
                       1.0, lv);
  }
  if (N)
    hipLaunchKernelGGL(k_kkt_residual, g1(N), dim3(256), 0, s, N, nI, idxI, rhs, sol, lv, wy, r,
                       reinterpret_cast<unsigned long long *>(red3));
}

// ---- the same in three launches (PGF_STEP_FUSED, pgf_api_step.hip): every value is computed by the
// expressions above in the same order, only the launch it is computed in changes.
// The row passes over J and H in one launch: the first jb workgroups are k_gemv_rows2 over J
// (c = J xn - b, wy = J v - delta s_y, complete), the others row_dot2 of H with (xn, v), stored raw
// to dot1, dot2 -- they need nothing from the J passes, the combine launch adds tmpn and u.
__global__ __launch_bounds__(256) void k_rows_jh(int m, int n, int jb, const double *__restrict__ J, int64_t ldj,
                                                 const double *__restrict__ H, int64_t ldh,
                                                 const double *__restrict__ xn, const double *__restrict__ v,
                                                 const double *__restrict__ b, double *__restrict__ c,
                                                 const double *__restrict__ sy, double delta,
                                                 double *__restrict__ wy, double *__restrict__ dot1,
                                                 double *__restrict__ dot2) {
  const int lane = threadIdx.x & 63;
  double d1, d2;
  if ((int)blockIdx.x < jb) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= m) return;
    row_dot2(J + (int64_t)r * ldj, xn, v, n, lane, d1, d2);
    if (lane == 0) {
      c[r] = d1 + -1.0 * b[r];
      wy[r] = d2 + -delta * sy[r];
    }
    return;
  }
  const int r = ((int)blockIdx.x - jb) * 4 + (threadIdx.x >> 6);
  if (r >= n) return;
  row_dot2(H + (int64_t)r * ldh, xn, v, n, lane, d1, d2);
  if (lane == 0) {
    dot1[r] = d1;
    dot2[r] = d2;
  }
}

// k_sum_partials2, the epilogue of the H pass and k_kkt_residual in one launch of 64-lane
// workgroups.  Lane t < n takes column t: its own chunks summed sequentially over p,
//   tmpn = q + sum_p partial1, u = lv + sum_p partial2, g = dot1 + 1.0 tmpn, lv <- dot2 + 1.0 u
// (dot1 arrives in g, dot2 in u; nparts == 0: the plain copies of the m == 0 branch), and
// r[pos[t]] = rhs[pos[t]] - lv[t] where the variable is inactive; lane n + k takes the constraint row
// k from wy.  The maxima: atomicMax on bit patterns (red zeroed by k_step_update).
//
// The hand-back of a dense qp step (TailHandback, pgf_solver::hb): the `nstat' doubles of the status
// block go to coherent host memory, the norm besides to `slot' (device memory, may be null), and
// behind a system-scope fence the sequence word h_stat[nstat] -- plain vector stores by one
// workgroup; the host spins on the word.  (Agent-scope loads: the maxima were written by atomics
// of other workgroups of the same launch when k_tail_combine's last workgroup gets here.)
__device__ __forceinline__ void handback_store(const double *stat, int nstat, int norm_at, double *h_stat,
                                               unsigned long long seq, double *slot) {
  if ((int)threadIdx.x < nstat) {
    const unsigned long long w = __hip_atomic_load(reinterpret_cast<const unsigned long long *>(stat) + threadIdx.x,
                                                   __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    reinterpret_cast<unsigned long long *>(h_stat)[threadIdx.x] = w;
    if (slot && (int)threadIdx.x == norm_at) slot[0] = __longlong_as_double((long long)w);
    __threadfence_system();
  }
  __syncthreads();
  if (threadIdx.x == 0)
    __hip_atomic_store(reinterpret_cast<unsigned long long *>(h_stat) + nstat, seq, __ATOMIC_RELEASE,
                       __HIP_MEMORY_SCOPE_SYSTEM);
}
// the step's last launch when pgf_qp_residual_norm was given a device slot: one workgroup
__global__ __launch_bounds__(64) void k_handback_store(const double *stat, int nstat, int norm_at, double *h_stat,
                                                       unsigned long long seq, double *slot) {
  handback_store(stat, nstat, norm_at, h_stat, seq, slot);
}
void launch_handback_store(hipStream_t s, const double *stat, int nstat, int norm_at, double *h_stat,
                           unsigned long long seq, double *slot) {
  hipLaunchKernelGGL(k_handback_store, dim3(1), dim3(64), 0, s, stat, nstat, norm_at, h_stat, seq, slot);
}

// NORM (256 lanes: workgroup b owns the entries [256 b, 256 b + 256) of the n + m concatenation,
// k_unscaled_res_norm's partition): each workgroup besides forms its partial of the unscaled
// residual's squares at the new point -- b_unscaled_res_sq's expressions and in-block order, with the
// g its lanes have just stored and the c k_rows_jh left complete -- and the last one to finish sums
// the partials (last_block_reduce, a ticket of its own) into th.norm_out, the value
// k_unscaled_res_norm gives at that point bit for bit, and hands the status block back.
template <int LANES, bool NORM>
__global__ __launch_bounds__(LANES) void k_tail_combine(int n, int m, int nI, int nparts,
                                                     const double *__restrict__ partial1,
                                                     const double *__restrict__ partial2,
                                                     const double *__restrict__ q, double *__restrict__ tmpn,
                                                     double *__restrict__ g, double *__restrict__ u,
                                                     double *__restrict__ lv, const uint8_t *__restrict__ mask,
                                                     const int *__restrict__ pos, const double *rhs,  // may alias r
                                                     const double *__restrict__ sol,
                                                     const double *__restrict__ wy, double *r,
                                                     unsigned long long *red,  // (inside th.stat)
                                                     TailHandback th) {
  const int t = blockIdx.x * LANES + threadIdx.x;
  double ar = 0.0, ab = 0.0, as = 0.0;
  int i = -1;
  double ks = 0.0, gnew = 0.0;
  if (t < n) {
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 8
    for (int p = 0; p < nparts; ++p) {
      s1 += partial1[(int64_t)p * n + t];
      s2 += partial2[(int64_t)p * n + t];
    }
    const double sgn = 1.0;
    const double tv = nparts ? q[t] + s1 : q[t];
    const double uv = nparts ? lv[t] + s2 : lv[t];
    const double d1 = g[t], d2 = u[t];
    tmpn[t] = tv;
    u[t] = uv;
    gnew = d1 + sgn * tv;
    g[t] = gnew;
    ks = d2 + sgn * uv;
    lv[t] = ks;
    if (!mask[t]) i = pos[t];
  } else if (t < n + m) {
    i = nI + (t - n);
    ks = wy[t - n];
  }
  if (i >= 0) {
    const double bi = rhs[i];
    const double ri = bi - ks;
    r[i] = ri;
    ar = fabs(ri);
    ab = fabs(bi);
    as = fabs(sol[i]);
    if (ar != ar) ar = __builtin_inf();  // a NaN must not vanish in the max
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    ar = fmax(ar, __shfl_down(ar, off));
    ab = fmax(ab, __shfl_down(ab, off));
    as = fmax(as, __shfl_down(as, off));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&red[0], (unsigned long long)__double_as_longlong(ar));
    atomicMax(&red[1], (unsigned long long)__double_as_longlong(ab));
    atomicMax(&red[2], (unsigned long long)__double_as_longlong(as));
    if (NORM) __threadfence();  // (performed before this workgroup's ticket: the last one reads them)
  }
  if constexpr (NORM) {
    double sq = 0.0;
    if (t < n)
      sq = unscaled_sq_x(th.dt, th.xhat[t], th.x[t], gnew, th.lb[t], th.ub[t]);
    else if (t < n + m)
      sq = unscaled_sq_y(th.dt, th.yhat[t - n], th.y[t - n], th.c[t - n]);
    block_sq_partial(sq, th.red);
    if (!last_block_reduce(th.red, gridDim.x, th.norm_out, th.ticket)) return;
    __syncthreads();  // (lane 0 has just stored the norm into the block)
    handback_store(th.stat, th.nstat, -1, th.h_stat, th.seq, nullptr);
  }
}

// launch_residual_and_eval(..., prepared = true) in at most three launches
void launch_residual_and_eval_fused(hipStream_t s, int n, int m, int nI, double delta, const double *H, int64_t ldh,
                                    const double *J, int64_t ldj, const int *pos, const uint8_t *mask,
                                    const double *rhs, const double *sol, const double *v, double *lv, double *u,
                                    double *wy, double *partial, int nparts, double *r, double *red3,
                                    const double *xn, const double *yn, const double *b, const double *q,
                                    double rho, double *c, double *w, double *tmpn, double *g,
                                    const TailHandback *th) {
  const int N = nI + m;
  const int jb = (m + 3) / 4, hb = (n + 3) / 4;
  if (jb + hb)
    hipLaunchKernelGGL(k_rows_jh, dim3(jb + hb), dim3(256), 0, s, m, n, jb, J, ldj, H, ldh, xn, v, b, c, sol + nI,
                       delta, wy, g, u);
  if (n == 0) launch_mult_vec(s, m, rho, c, yn, w);
  int used = 0;
  double *p2 = partial + (size_t)nparts * n;
  if (n && m) {
    const int chunk = (m + nparts - 1) / nparts;
    used = (m + chunk - 1) / chunk;
    hipLaunchKernelGGL(k_gemvT_partial2, dim3((n + 255) / 256, used), dim3(256), 0, s, m, n, J, ldj, rho, c, yn, w,
                       sol + nI, chunk, partial, p2);
  }
  if (th && (n || N))
    hipLaunchKernelGGL((k_tail_combine<256, true>), dim3((n + m + 255) / 256), dim3(256), 0, s, n, m, nI, used,
                       partial, p2, q, tmpn, g, u, lv, mask, pos, rhs, sol, wy, r,
                       reinterpret_cast<unsigned long long *>(red3), *th);
  else if (n || N)
    hipLaunchKernelGGL((k_tail_combine<64, false>), dim3((n + m + 63) / 64), dim3(64), 0, s, n, m, nI, used, partial,
                       p2, q, tmpn, g, u, lv, mask, pos, rhs, sol, wy, r,
                       reinterpret_cast<unsigned long long *>(red3), TailHandback{});
}

// ---- matrix norms for the normwise backward error of the residual guard (pgf_api_guard.hip)
// out[0] = max_i sum_j |A_ij| (rows x cols, row-major): one workgroup per row; non-negative
// doubles order like their bit patterns, so atomicMax on the 64-bit words does the reduction
__global__ __launch_bounds__(256) void k_abs_rowsum_max(int cols, const double *__restrict__ A, int64_t ld,
                                                        unsigned long long *__restrict__ out) {
  __shared__ double part[4];
  const double *row = A + (int64_t)blockIdx.x * ld;
  double acc = 0.0;
  for (int j = threadIdx.x; j < cols; j += 256) acc += fabs(row[j]);
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double t = part[0] + part[1] + part[2] + part[3];
    if (t == t) atomicMax(out, (unsigned long long)__double_as_longlong(t));
  }
}
// out[0] = max_j sum_i |A_ij|: one thread per column (coalesced across the threads of a row)
__global__ __launch_bounds__(256) void k_abs_colsum_max(int rows, int cols, const double *__restrict__ A,
                                                        int64_t ld, unsigned long long *__restrict__ out) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  double acc = 0.0;
  if (j < cols)
    for (int i = 0; i < rows; ++i) acc += fabs(A[(int64_t)i * ld + j]);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) acc = fmax(acc, __shfl_down(acc, off));
  if ((threadIdx.x & 63) == 0 && acc == acc) atomicMax(out, (unsigned long long)__double_as_longlong(acc));
}
// norms3: ||H||_inf, ||J||_inf, ||J||_1 (zeroed here)
void launch_matrix_norms(hipStream_t s, int n, int m, const double *H, int64_t ldh, const double *J,
                         int64_t ldj, double *norms3) {
  (void)hipMemsetAsync(norms3, 0, 3 * sizeof(double), s);
  unsigned long long *o = reinterpret_cast<unsigned long long *>(norms3);
  if (n && H) hipLaunchKernelGGL(k_abs_rowsum_max, dim3(n), dim3(256), 0, s, n, H, ldh, o);
  if (n && m && J) {
    hipLaunchKernelGGL(k_abs_rowsum_max, dim3(m), dim3(256), 0, s, n, J, ldj, o + 1);
    hipLaunchKernelGGL(k_abs_colsum_max, g1(n), dim3(256), 0, s, m, n, J, ldj, o + 2);
  }
}

void launch_axpy1(hipStream_t s, int N, const double *d, double *x) {
  if (N) hipLaunchKernelGGL(k_axpy1, g1(N), dim3(256), 0, s, N, d, x);
}

void launch_symmetrize(hipStream_t s, double *A, int64_t ld, int N) {
  if (N) hipLaunchKernelGGL(k_symmetrize, dim3((N + 255) / 256, N), dim3(256), 0, s, A, ld, N);
}
