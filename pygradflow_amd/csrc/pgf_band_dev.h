// Device bodies of the narrow banded step (half-bandwidth <= 8, 8 x 8 block cyclic reduction).
// pgf_sparse.hip wraps each in the kernel of a single handle and, further down, in its batched
// twin (instance = blockIdx.y, pointers from the instance's BandInst): the same function with the
// same arguments in the same order, so that both routes compute the same bits.  The bodies index
// their work with blockIdx.x / threadIdx.x only.
//
// Compiled with -ffp-contract=off in both files (explicit fma() only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgf_bcr_dev.h"

// ---------------------------------------------------------------- CSR products
// One row (or column) per lane: acc = step(k, acc) over the entries [k0, k1) of the lane's row.  Rows
// are short -- except the dense rows and columns of a bordered band (a budget constraint over all
// variables, a global parameter's column of J): one lane walking n dependent entries took 4 ms at
// n = 16 384.  A row of more than SP_LONG_ROW entries is therefore summed by the whole wavefront, 64
// entries at a time, and reduced in a fixed order; shorter rows are summed by their lane in entry
// order, as ever.  EVERY lane of the wavefront must call this (lanes without a row: k0 == k1).
#define SP_LONG_ROW 256
template <class Step>
__device__ __forceinline__ double sp_row_dot(int k0, int k1, Step step) {
  const int lane = threadIdx.x & 63;
  const bool longrow = k1 - k0 > SP_LONG_ROW;
  double acc = 0.0;
  if (!longrow)
    for (int k = k0; k < k1; ++k) acc = step(k, acc);
  unsigned long long pending = __ballot(longrow);
  while (pending) {
    const int src = __ffsll((long long)pending) - 1;
    pending &= pending - 1;
    const int a0 = __shfl(k0, src), a1 = __shfl(k1, src);
    double part = 0.0;
    for (int k = a0 + lane; k < a1; k += 64) part = step(k, part);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_down(part, off);
    part = __shfl(part, 0);
    if (lane == src) acc = part;
  }
  return acc;
}

// y[r] = sum_k val[k] * x[col[k]]  (+ sgn * add[r]);  rows are short: one lane per row
__device__ __forceinline__ void b_csr_spmv(int rows, const int *__restrict__ ptr, const int *__restrict__ col,
                                           const double *__restrict__ val, const double *__restrict__ x,
                                           const double *__restrict__ add, double sgn, double *__restrict__ y) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  double acc = 0.0;
  for (int k = ptr[r]; k < ptr[r + 1]; ++k) acc = fma(val[k], x[col[k]], acc);
  y[r] = add ? acc + sgn * add[r] : acc;
}

// out[j] = base[j] + sum_k val[map[k]] * w[row[k]] over the entries of column j
// (transposed product through the column-ordered copy of the pattern: no atomics)
__device__ __forceinline__ void b_csc_spmvT(int cols, const int *__restrict__ tptr, const int *__restrict__ trow,
                                            const int *__restrict__ tmap, const double *__restrict__ val,
                                            const double *__restrict__ w, const double *__restrict__ base,
                                            double *__restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cols) return;
  double acc = 0.0;
  for (int k = tptr[j]; k < tptr[j + 1]; ++k) acc = fma(val[tmap[k]], w[trow[k]], acc);
  out[j] = base[j] + acc;
}

// The evaluation of the device-resident sparse mode in two launches instead of four (the banded
// path is bound by the number of its small dependent launches, not by their arithmetic):
//   c = J x - b ; w = rho c + y                  (one lane per constraint row)
//   g = H x + (q + J' w)                         (one lane per variable: row of H, column of J)
// Operation order as in the separate kernels (b_csr_spmv, k_mult_vec, b_csc_spmvT): the active-set
// mask computed from g is compared bit for bit.
__device__ __forceinline__ void b_sp_eval_c(int m, const int *__restrict__ ptr, const int *__restrict__ col,
                                            const double *__restrict__ val, const double *__restrict__ x,
                                            const double *__restrict__ b, double rho, const double *__restrict__ y,
                                            double *__restrict__ c, double *__restrict__ w) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = r < m;
  const double acc = sp_row_dot(in ? ptr[r] : 0, in ? ptr[r + 1] : 0,
                                [&](int k, double a) { return fma(val[k], x[col[k]], a); });
  if (!in) return;
  const double cr = acc + -1.0 * b[r];
  c[r] = cr;
  w[r] = rho * cr + y[r];
}

__device__ __forceinline__ void b_sp_eval_g(int n, const int *__restrict__ hptr, const int *__restrict__ hcol,
                                            const double *__restrict__ hval, const int *__restrict__ tptr,
                                            const int *__restrict__ trow, const int *__restrict__ tmap,
                                            const double *__restrict__ jval, const double *__restrict__ x,
                                            const double *__restrict__ w, const double *__restrict__ q,
                                            double *__restrict__ g) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = j < n;
  const double at = sp_row_dot(in ? tptr[j] : 0, in ? tptr[j + 1] : 0,
                               [&](int k, double a) { return fma(jval[tmap[k]], w[trow[k]], a); });
  const double acc = sp_row_dot(in ? hptr[j] : 0, in ? hptr[j + 1] : 0,
                                [&](int k, double a) { return fma(hval[k], x[hcol[k]], a); });
  if (!in) return;
  const double base = q[j] + at;  // = tmpn[j] of the separate kernels
  g[j] = acc + 1.0 * base;
}

// permuted right-hand side with the products H b0, J b0 formed on the fly (one launch for
// b_csr_spmv x 2 + b_band_rhs)
__device__ __forceinline__ void b_band_rhs_fused(int n, int m, const uint8_t *__restrict__ mask,
                                                 const double *__restrict__ F, const double *__restrict__ b0full,
                                                 const int *__restrict__ hptr, const int *__restrict__ hcol,
                                                 const double *__restrict__ hval, const int *__restrict__ jptr,
                                                 const int *__restrict__ jcol, const double *__restrict__ jval,
                                                 double fact, const int *__restrict__ pos,
                                                 double *__restrict__ brhs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  // (both products by every lane of the wavefront, sp_row_dot: a lane of the other kind has no entries)
  const bool isvar = i < n, iscon = i >= n && i < n + m;
  const int r = i - n;
  const double hacc = sp_row_dot(isvar ? hptr[i] : 0, isvar ? hptr[i + 1] : 0,
                                 [&](int k, double a) { return fma(hval[k], b0full[hcol[k]], a); });
  const double jacc = sp_row_dot(iscon ? jptr[r] : 0, iscon ? jptr[r + 1] : 0,
                                 [&](int k, double a) { return fma(jval[k], b0full[jcol[k]], a); });
  if (i >= n + m) return;
  double v;
  if (isvar)
    v = mask[i] ? b0full[i] : F[i] - hacc;
  else
    v = fact * F[i] - jacc;
  brhs[pos[i]] = v;
}

// full-size right-hand side in permuted order:
//   variable i inactive: F_i - (H b0)_i     active: b0_i = dt F_i
//   constraint r       : fact F_{n+r} - (J b0)_r
__device__ __forceinline__ void b_band_rhs(int n, int m, const uint8_t *__restrict__ mask,
                                           const double *__restrict__ F, const double *__restrict__ b0full,
                                           const double *__restrict__ Hb0, const double *__restrict__ Jb0,
                                           double fact, const int *__restrict__ pos, double *__restrict__ brhs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n + m) return;
  double v;
  if (i < n)
    v = mask[i] ? b0full[i] : F[i] - Hb0[i];
  else
    v = fact * F[i] - Jb0[i - n];
  brhs[pos[i]] = v;
}

// ---------------------------------------------------------------- band assembly
// diagonal: lamb (inactive variable), 1 (active variable), -delta (constraint)
__device__ __forceinline__ void b_band_set_diag(int n, int m, const int *__restrict__ pos,
                                                const uint8_t *__restrict__ mask, double lamb, double delta,
                                                double *__restrict__ band, int ldb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n + m) return;
  double v;
  if (i < n)
    v = mask[i] ? 1.0 : lamb;
  else
    v = -delta;
  band[(int64_t)pos[i] * ldb] = v;
}

// H entries (lower part in permuted order; slot < 0 marks the mirrored duplicates)
__device__ __forceinline__ void b_band_scatter_H(int nnz, const int *__restrict__ row, const int *__restrict__ col,
                                                 const double *__restrict__ val, const int *__restrict__ slot,
                                                 const uint8_t *__restrict__ mask, double *__restrict__ band) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nnz) return;
  const int s = slot[k];
  if (s < 0) return;
  if (mask[row[k]] || mask[col[k]]) return;
  band[s] += val[k];  // slots are unique per entry; the diagonal was set before this launch
}

__device__ __forceinline__ void b_band_scatter_J(int nnz, const int *__restrict__ col,
                                                 const double *__restrict__ val, const int *__restrict__ slot,
                                                 const uint8_t *__restrict__ mask, double *__restrict__ band) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= nnz) return;
  if (mask[col[k]]) return;
  band[slot[k]] = val[k];
}

// ---------------------------------------------------------------- step update (a9, a15, a16)
// 256 threads; red[blockIdx.x]: the workgroup's share of ||d||^2
__device__ __forceinline__ void b_band_step_update(
    int n, int m, const int *__restrict__ pos, const double *__restrict__ sol, double fact,
    double rho, const double *__restrict__ x, const double *__restrict__ y,
    const double *__restrict__ lb, const double *__restrict__ ub, const double *__restrict__ F,
    double *__restrict__ dx, double *__restrict__ dy, double *__restrict__ xn,
    double *__restrict__ yn, double *__restrict__ red) {
  __shared__ double part[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double sq = 0.0;
  if (i < n) {
    double d = sol[pos[i]];
    const double xi = x[i];
    double v = xi - d;
    const double lo = lb[i], hi = ub[i];
    if (v < lo) {
      v = lo;
      d = xi - lo;
    }
    if (v > hi) {
      v = hi;
      d = xi - hi;
    }
    dx[i] = d;
    xn[i] = v;
    sq = d * d;
  } else if (i < n + m) {
    const int r = i - n;
    const double t = rho * F[i];
    const double d = fact * (sol[pos[i]] - t);
    dy[r] = d;
    yn[r] = y[r] - d;
    sq = d * d;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) sq += __shfl_down(sq, off);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) red[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// ================================================================= block cyclic reduction
// The permuted KKT matrix has half-bandwidth bw <= 8, i.e. it is block tridiagonal with
// 8 x 8 blocks: D_i (diagonal), L_i (coupling to the left neighbour), U_i = L_{i+1}^T.
// Cyclic reduction eliminates every other block row per level (all of them in parallel):
//   kept block i, eliminated neighbours i-s, i+s:
//     alpha = L_i inv(D_{i-s}),  gamma = U_i inv(D_{i+s})
//     D_i -= alpha U_{i-s} + gamma L_{i+s};  f_i -= alpha f_{i-s} + gamma f_{i+s}
//     L_i <- -alpha L_{i-s}  (now couples to i-2s);  U_i <- -gamma U_{i+s}
// log2(N/8) levels instead of N sequential pivots; back-substitution walks the levels in
// reverse.  Every principal block and Schur complement of a symmetric quasi-definite matrix
// is again quasi-definite, so the 8 x 8 pivots D_i are invertible without pivoting, and by
// Haynsworth's inertia additivity the number of negative eigenvalues of K is the sum of the
// negative pivots met while inverting the D_i.  One wavefront per block, lane <-> (row, col).
#define BCR_B 8

// block extraction from the band (+ identity padding of the last block); 64 threads, block blockIdx.x
__device__ __forceinline__ void b_bcr_extract(const double *__restrict__ band, int ldb, int bw,
                                              const double *__restrict__ rhs, int N, int nb,
                                              double *__restrict__ D, double *__restrict__ L,
                                              double *__restrict__ U, double *__restrict__ F,
                                              double *__restrict__ rhs0, int *__restrict__ flags) {
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i == 0 && lane < 4) flags[lane] = 0;  // (every kernel that sets them runs after this one)
  // accuracy guard (b_band_residual): the right-hand side survives the solve in rhs0
  if (rhs0 && lane < 8 && i * 8 + lane < N) rhs0[i * 8 + lane] = rhs[i * 8 + lane];
  const int r = lane >> 3, c = lane & 7;
  const int gr = i * 8 + r, gc = i * 8 + c;
  // diagonal block, symmetric fill
  double d = (r == c) ? 1.0 : 0.0;
  if (gr < N && gc < N) {
    const int hi = max(gr, gc), lo = min(gr, gc);
    d = (hi - lo <= bw) ? band[(int64_t)hi * ldb + (hi - lo)] : 0.0;
  }
  D[(int64_t)i * 64 + lane] = d;
  // L_i[r][c] = K[8i + r][8(i-1) + c]
  double l = 0.0;
  if (i > 0 && gr < N) {
    const int cc = (i - 1) * 8 + c;
    const int dist = gr - cc;
    if (dist <= bw) l = band[(int64_t)gr * ldb + dist];
  }
  L[(int64_t)i * 64 + lane] = l;
  // U_i[r][c] = K[8i + r][8(i+1) + c] = K[8(i+1) + c][8i + r]
  double u = 0.0;
  if (i + 1 < nb && gr < N) {
    const int rr = (i + 1) * 8 + c;
    const int dist = rr - gr;
    if (rr < N && dist <= bw) u = band[(int64_t)rr * ldb + dist];
  }
  U[(int64_t)i * 64 + lane] = u;
  if (lane < 8) F[(int64_t)i * 8 + lane] = (i * 8 + lane < N) ? rhs[i * 8 + lane] : 0.0;
}

// ---- per-block work of one wavefront (lane = threadIdx.x & 63); `sm` is the wavefront's own
// LDS scratch of BCR_SCRATCH doubles.  Used by the one-block-per-workgroup kernels of the
// large levels and by the fused tail kernel below.
#define BCR_SCRATCH (3 * 64 + 8)

// The negative-pivot count goes to negcnt[gi] (gi = the block's global index), NOT to one
// atomic counter: in a KKT matrix nearly every block has negative pivots, and 9 375
// workgroups adding to the same word serialised in L2 (110 us for the first level alone).
__device__ __forceinline__ void bcr_invert_block(const double *__restrict__ D,
                                                 double *__restrict__ Dinv, int i, int lane,
                                                 double *sm, int *__restrict__ flags,
                                                 int *__restrict__ negcnt, int gi) {
  double *M = sm;
  M[lane] = D[(int64_t)i * 64 + lane];
  int bad = 0;
  const int neg = gj_inverse8(M, lane, &bad);
  Dinv[(int64_t)i * 64 + lane] = M[lane];
  if (lane == 0) {
    if (bad) atomicOr(&flags[0], 1);
    negcnt[gi] = neg;
  }
}

// kept block i of the level with stride s (neighbours i - s, i + s are eliminated)
__device__ __forceinline__ void bcr_reduce_block(double *__restrict__ D, double *__restrict__ L,
                                                 double *__restrict__ U, double *__restrict__ F,
                                                 const double *__restrict__ Dinv, int nb, int s,
                                                 int i, int lane, double *sm) {
  double *A = sm, *B = sm + 64, *T = sm + 128, *fs = sm + 192;
  const int r = lane >> 3, c = lane & 7;
  double dv = D[(int64_t)i * 64 + lane];
  double fv = (lane < 8) ? F[(int64_t)i * 8 + lane] : 0.0;
  double lnew = 0.0, unew = 0.0;
  const int le = i - s, ri = i + s;
  if (le >= 0) {
    A[lane] = L[(int64_t)i * 64 + lane];
    B[lane] = Dinv[(int64_t)le * 64 + lane];
    const double al = mm8(A, B, r, c);  // alpha = L_i inv(D_left)
    T[lane] = al;
    B[lane] = U[(int64_t)le * 64 + lane];
    if (lane < 8) fs[lane] = F[(int64_t)le * 8 + lane];
    dv -= mm8(T, B, r, c);              // D_i -= alpha U_left
    if (lane < 8) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 8; ++k) acc = fma(T[lane * 8 + k], fs[k], acc);
      fv -= acc;                        // f_i -= alpha f_left
    }
    B[lane] = L[(int64_t)le * 64 + lane];
    lnew = -mm8(T, B, r, c);            // couples i to i - 2s
  }
  if (ri < nb) {
    A[lane] = U[(int64_t)i * 64 + lane];
    B[lane] = Dinv[(int64_t)ri * 64 + lane];
    const double ga = mm8(A, B, r, c);  // gamma = U_i inv(D_right)
    T[lane] = ga;
    B[lane] = L[(int64_t)ri * 64 + lane];
    if (lane < 8) fs[lane] = F[(int64_t)ri * 8 + lane];
    dv -= mm8(T, B, r, c);              // D_i -= gamma L_right
    if (lane < 8) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 8; ++k) acc = fma(T[lane * 8 + k], fs[k], acc);
      fv -= acc;
    }
    B[lane] = U[(int64_t)ri * 64 + lane];
    unew = -mm8(T, B, r, c);            // couples i to i + 2s
  }
  D[(int64_t)i * 64 + lane] = dv;
  L[(int64_t)i * 64 + lane] = lnew;
  U[(int64_t)i * 64 + lane] = unew;
  if (lane < 8) F[(int64_t)i * 8 + lane] = fv;
}

// One level in ONE launch: kept block i inverts its two eliminated neighbours itself (each
// eliminated block is inverted twice, by its left and by its right kept neighbour -- 2 x 1.5 us
// of redundant work against a dependent launch of ~5 us per level) and then reduces.  The
// left kept neighbour of an eliminated block always exists, so IT stores the inverse for the
// back-substitution and reports the block's pivots.
// Result to (Do, Lo, Uo, Fo)[io] -- the block itself for the one-level launches, an LDS slot
// or the other block set for the two-level ones; `report`: store the right neighbour's inverse
// and pivot count (exactly one caller per eliminated block does).  (io0, gr): index of the
// right neighbour in Dinv / negcnt (differs from ri when the inputs are LDS slots).
__device__ __forceinline__ void bcr_level_block(const double *D, const double *L, const double *U,
                                                const double *F, double *__restrict__ Dinv, int nb,
                                                int s, int i, int lane, double *sm,
                                                int *__restrict__ flags, int *__restrict__ negcnt,
                                                double *Do, double *Lo, double *Uo, double *Fo, int io,
                                                bool report, int gr) {
  double *A = sm, *B = sm + 64, *T = sm + 128, *fs = sm + 192;
  const int r = lane >> 3, c = lane & 7;
  double dv = D[(int64_t)i * 64 + lane];
  double fv = (lane < 8) ? F[(int64_t)i * 8 + lane] : 0.0;
  double lnew = 0.0, unew = 0.0;
  const int le = i - s, ri = i + s;
  if (le >= 0) {
    A[lane] = L[(int64_t)i * 64 + lane];
    B[lane] = D[(int64_t)le * 64 + lane];
    int bad = 0;
    (void)gj_inverse8(B, lane, &bad);   // reported by the kept block to the left of `le`
    const double al = mm8(A, B, r, c);  // alpha = L_i inv(D_left)
    T[lane] = al;
    B[lane] = U[(int64_t)le * 64 + lane];
    if (lane < 8) fs[lane] = F[(int64_t)le * 8 + lane];
    dv -= mm8(T, B, r, c);              // D_i -= alpha U_left
    if (lane < 8) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 8; ++k) acc = fma(T[lane * 8 + k], fs[k], acc);
      fv -= acc;                        // f_i -= alpha f_left
    }
    B[lane] = L[(int64_t)le * 64 + lane];
    lnew = -mm8(T, B, r, c);            // couples i to i - 2s
  }
  if (ri < nb) {
    A[lane] = U[(int64_t)i * 64 + lane];
    B[lane] = D[(int64_t)ri * 64 + lane];
    int bad = 0;
    const int neg = gj_inverse8(B, lane, &bad);
    if (report) {
      Dinv[(int64_t)gr * 64 + lane] = B[lane];
      if (lane == 0) {
        if (bad) atomicOr(&flags[0], 1);
        negcnt[gr] = neg;
      }
    }
    const double ga = mm8(A, B, r, c);  // gamma = U_i inv(D_right)
    T[lane] = ga;
    B[lane] = L[(int64_t)ri * 64 + lane];
    if (lane < 8) fs[lane] = F[(int64_t)ri * 8 + lane];
    dv -= mm8(T, B, r, c);              // D_i -= gamma L_right
    if (lane < 8) {
      double acc = 0.0;
#pragma unroll
      for (int k = 0; k < 8; ++k) acc = fma(T[lane * 8 + k], fs[k], acc);
      fv -= acc;
    }
    B[lane] = U[(int64_t)ri * 64 + lane];
    unew = -mm8(T, B, r, c);            // couples i to i + 2s
  }
  Do[(int64_t)io * 64 + lane] = dv;
  Lo[(int64_t)io * 64 + lane] = lnew;
  Uo[(int64_t)io * 64 + lane] = unew;
  if (lane < 8) Fo[(int64_t)io * 8 + lane] = fv;
}

// x_i = inv(D_i) (f_i - L_i x_{i-s} - U_i x_{i+s});  s == 0: the last remaining block
__device__ __forceinline__ void bcr_back_block(const double *__restrict__ Dinv,
                                               const double *__restrict__ L,
                                               const double *__restrict__ U,
                                               const double *__restrict__ F,
                                               double *__restrict__ X, int nb, int s, int i,
                                               int lane, double *sm) {
  double *t = sm, *xl = sm + 8, *xr = sm + 16;
  const int le = i - s, ri = i + s;
  const bool hl = (s > 0) && le >= 0, hr = (s > 0) && ri < nb;
  if (lane < 8) {
    // L1-bypassing loads: in the two-level launch x of a neighbour comes from another
    // wavefront of the same workgroup a moment ago
    xl[lane] = hl ? __hip_atomic_load(X + (int64_t)le * 8 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
    xr[lane] = hr ? __hip_atomic_load(X + (int64_t)ri * 8 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0.0;
  }
  if (lane < 8) {
    double acc = F[(int64_t)i * 8 + lane];
    if (hl)
#pragma unroll
      for (int k = 0; k < 8; ++k) acc = fma(-L[(int64_t)i * 64 + lane * 8 + k], xl[k], acc);
    if (hr)
#pragma unroll
      for (int k = 0; k < 8; ++k) acc = fma(-U[(int64_t)i * 64 + lane * 8 + k], xr[k], acc);
    t[lane] = acc;
  }
  if (lane < 8) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc = fma(Dinv[(int64_t)i * 64 + lane * 8 + k], t[k], acc);
    X[(int64_t)i * 8 + lane] = acc;
  }
}

// TWO levels (strides s and 2 s) in one launch: the workgroup of block k = 4 s j keeps k through
// both.  Its three wavefronts reduce k - 2 s, k and k + 2 s by one level side by side (from the
// input set into LDS slots; the outer two are also reduced by the neighbouring workgroups: a
// level of this size is bound by its launch, not by its arithmetic), then wavefront 0 reduces k
// by the second level from the slots.  Nothing is updated in place -- the neighbours still
// read the input set -- so the results go to the OTHER block set: k's new blocks and, for the
// back-substitution, the level-one blocks of k + 2 s (eliminated at the second level; k - 2 s
// is the left neighbour's k + 2 s).  Inverses and pivot counts of the eliminated blocks
// k + s, k + 3 s (first level) and k + 2 s (second level) are this workgroup's to report.
// 192 threads, workgroup blockIdx.x.
__device__ __forceinline__ void b_bcr_level2(const double *__restrict__ Di, const double *__restrict__ Li,
                                             const double *__restrict__ Ui, const double *__restrict__ Fi,
                                             double *__restrict__ Do, double *__restrict__ Lo,
                                             double *__restrict__ Uo, double *__restrict__ Fo,
                                             double *__restrict__ Dinv, int nb, int s,
                                             int *__restrict__ flags, int *__restrict__ negcnt) {
  __shared__ double sm[3][BCR_SCRATCH];
  __shared__ double Ds[3 * 64], Ls[3 * 64], Us[3 * 64], Fs[3 * 8];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int k = (int)blockIdx.x * 4 * s;
  if (k >= nb) return;
  const int i = k + (w - 1) * 2 * s;  // k - 2 s, k, k + 2 s
  if (i >= 0 && i < nb)
    bcr_level_block(Di, Li, Ui, Fi, Dinv, nb, s, i, lane, sm[w], flags, negcnt, Ds, Ls, Us, Fs, w,
                    /*report=*/w >= 1, i + s);
  __syncthreads();
  if (w == 0) {
    // second level on the slots: slot 1 = k, its neighbours slots 0 and 2 where they exist
    const int lo = (k - 2 * s >= 0) ? 0 : 1;
    const int cnt = ((k + 2 * s < nb) ? 3 : 2) - lo;
    bcr_level_block(Ds + lo * 64, Ls + lo * 64, Us + lo * 64, Fs + lo * 8, Dinv, cnt, 1, 1 - lo, lane,
                    sm[0], flags, negcnt, Do, Lo, Uo, Fo, k, /*report=*/true, k + 2 * s);
  } else if (w == 2 && k + 2 * s < nb) {
    // what the back-substitution of k + 2 s needs (its inverse comes from wavefront 0)
    const int64_t g = (int64_t)(k + 2 * s);
    Lo[g * 64 + lane] = Ls[2 * 64 + lane];
    Uo[g * 64 + lane] = Us[2 * 64 + lane];
    if (lane < 8) Fo[g * 8 + lane] = Fs[2 * 8 + lane];
  }
}

// Back-substitution of TWO levels in one launch (the mirror of b_bcr_level2): the workgroup of
// block j = 2 s (mod 4 s) solves j at stride 2 s (blocks of set 2: level-one values), then its
// two wavefronts solve j - s and j + s at stride s (set 1: the input set of that launch), which
// only need x_j and the already known x_{j -+ 2 s}.  A workgroup whose j lies beyond the last
// block still owns j - s.  128 threads, workgroup blockIdx.x.
__device__ __forceinline__ void b_bcr_back2(const double *__restrict__ Dinv, const double *__restrict__ L1,
                                            const double *__restrict__ U1, const double *__restrict__ F1,
                                            const double *__restrict__ L2, const double *__restrict__ U2,
                                            const double *__restrict__ F2, double *__restrict__ X, int nb,
                                            int s) {
  __shared__ double sm[2][BCR_SCRATCH];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int j = 2 * s + (int)blockIdx.x * 4 * s;
  if (j - s >= nb) return;
  if (w == 0 && j < nb) {
    bcr_back_block(Dinv, L2, U2, F2, X, nb, 2 * s, j, lane, sm[0]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // x_j has reached L2 before the barrier
  }
  __syncthreads();
  const int i = j + (w == 0 ? -s : s);
  if (i < nb) bcr_back_block(Dinv, L1, U1, F1, X, nb, s, i, lane, sm[w]);
}

// All levels from stride s0 upwards, the last block, and the matching back-substitution
// levels in ONE workgroup: at most BCR_TAIL_BLOCKS blocks are still in play there, every level
// was two dependent launches of a few microseconds each (launch-bound), and the whole
// remaining system fits in LDS.  The in-play blocks (global index j * s0) are copied to LDS
// in compact order, reduced with strides 1, 2, 4, ... of the compact index by 16 wavefronts
// taking blocks round-robin (a workgroup barrier between the invert / reduce / back phases),
// and only their solution X goes back to HBM for the lower back-substitution levels.
// (A first version ran the tail on the global arrays with up to 512 blocks: every block
// operation is a chain of dependent HBM round trips, one CU working through them was 3x
// slower than the launches it replaced.)  1024 threads; 94 KB of LDS: one tail per CU.
#define BCR_TAIL_BLOCKS 32
__device__ __forceinline__ void b_bcr_tail(const double *__restrict__ D, const double *__restrict__ L,
                                           const double *__restrict__ U, const double *__restrict__ F,
                                           double *__restrict__ X, int nb, int s0,
                                           int *__restrict__ flags, int *__restrict__ negcnt) {
  __shared__ double Dl[BCR_TAIL_BLOCKS * 64], Ll[BCR_TAIL_BLOCKS * 64], Ul[BCR_TAIL_BLOCKS * 64];
  __shared__ double Il[BCR_TAIL_BLOCKS * 64], Fl[BCR_TAIL_BLOCKS * 8], Xl[BCR_TAIL_BLOCKS * 8];
  __shared__ double smem[16 * BCR_SCRATCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double *sm = smem + wave * BCR_SCRATCH;
  const int nc = (nb + s0 - 1) / s0;  // compact block count (<= BCR_TAIL_BLOCKS)
  for (int p = tid; p < nc * 64; p += 1024) {
    const int64_t g = (int64_t)(p >> 6) * s0 * 64 + (p & 63);
    Dl[p] = D[g];
    Ll[p] = L[g];
    Ul[p] = U[g];
  }
  for (int p = tid; p < nc * 8; p += 1024) Fl[p] = F[(int64_t)(p >> 3) * s0 * 8 + (p & 7)];
  __syncthreads();
  int top = 0;
  for (int st = 1; st < nc; st *= 2) {
    const int ne = (nc - st + 2 * st - 1) / (2 * st);
    for (int e = wave; e < ne; e += 16) {
      const int j = st + e * 2 * st;
      bcr_invert_block(Dl, Il, j, lane, sm, flags, negcnt, j * s0);
    }
    __syncthreads();
    const int nk = (nc + 2 * st - 1) / (2 * st);
    for (int k = wave; k < nk; k += 16)
      bcr_reduce_block(Dl, Ll, Ul, Fl, Il, nc, st, k * 2 * st, lane, sm);
    __syncthreads();
    top = st;
  }
  if (wave == 0) {
    bcr_invert_block(Dl, Il, 0, lane, sm, flags, negcnt, 0);
    bcr_back_block(Il, Ll, Ul, Fl, Xl, nc, 0, 0, lane, sm);
  }
  __syncthreads();
  for (int st = top; st >= 1; st /= 2) {
    const int ne = (nc - st + 2 * st - 1) / (2 * st);
    for (int e = wave; e < ne; e += 16)
      bcr_back_block(Il, Ll, Ul, Fl, Xl, nc, st, st + e * 2 * st, lane, sm);
    __syncthreads();
  }
  for (int p = tid; p < nc * 8; p += 1024) X[(int64_t)(p >> 3) * s0 * 8 + (p & 7)] = Xl[p];
  // inertia: every block has been inverted exactly once by now (earlier launches or above)
  __shared__ int part[16];
  int cnt = 0;
  for (int i = tid; i < nb; i += 1024) cnt += negcnt[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
  if (lane == 0) part[wave] = cnt;
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
    for (int w = 0; w < 16; ++w) tot += part[w];
    flags[1] = tot;
  }
}

// Accuracy guard of the banded path: r = rhs0 - K x with K read from the assembled band (cyclic
// reduction leaves it intact; lower band, row i holds K[i][i - d] at [i][d]), max |r| and
// max (|K| |x| + |rhs0|) per workgroup.  256 threads, rows [256 blockIdx.x, + 256).
__device__ __forceinline__ void b_band_residual(const double *__restrict__ band, int ldb, int bw, int N,
                                                const double *__restrict__ x,
                                                const double *__restrict__ rhs0, double *__restrict__ r,
                                                double *__restrict__ rsmax,
                                                const int *__restrict__ flags, int nred) {
  // the pivot flags of the solve ride along behind the pairs and the step update's partial sums
  // (one device-to-host copy for all three, pgf_api_band.hip)
  if (blockIdx.x == 0 && threadIdx.x < 4) rsmax[3 * nred + threadIdx.x] = (double)flags[threadIdx.x];
  // rows [i0, i0 + 256 + bw) of the band (contiguous in memory: coalesced) and x[i0 - bw,
  // i0 + 256 + bw) staged in LDS: row i needs its own band row and, for the upper triangle, the
  // rows i + 1 .. i + bw of its neighbours (bw <= 10, ldb <= 12)
  __shared__ double bs[(256 + 10) * 12];
  __shared__ double xs[256 + 20];
  __shared__ double pr[4], pb[4];
  const int i0 = blockIdx.x * 256, tid = threadIdx.x;
  const int nrow = min(256 + bw, N - i0);
  for (int p = tid; p < nrow * ldb; p += 256) bs[p] = band[(int64_t)i0 * ldb + p];
  for (int p = tid; p < 256 + 2 * bw; p += 256) {
    const int g = i0 - bw + p;
    xs[p] = (g >= 0 && g < N) ? x[g] : 0.0;
  }
  __syncthreads();
  const int i = i0 + tid;
  // ab: the row's share of the normwise backward error's denominator, (|K| |x| + |rhs|)_i <=
  // ||K|| max |x| + max |rhs| -- a backward-stable solve only guarantees |r| <~ eps |K| |x|, which
  // against max |rhs| alone is eps cond(K) (pgf_api.hip, residual_rel)
  double ar = 0.0, ab = 0.0;
  if (i < N) {
    double acc = rhs0[i];
    ab = fabs(acc);
    for (int d = 0; d <= bw && d <= i; ++d) {
      acc = fma(-bs[tid * ldb + d], xs[bw + tid - d], acc);
      ab += fabs(bs[tid * ldb + d] * xs[bw + tid - d]);
    }
    for (int d = 1; d <= bw && i + d < N; ++d) {
      acc = fma(-bs[(tid + d) * ldb + d], xs[bw + tid + d], acc);
      ab += fabs(bs[(tid + d) * ldb + d] * xs[bw + tid + d]);
    }
    r[i] = acc;
    ar = (acc == acc) ? fabs(acc) : __builtin_huge_val();
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    ar = fmax(ar, __shfl_down(ar, off));
    ab = fmax(ab, __shfl_down(ab, off));
  }
  if ((threadIdx.x & 63) == 0) {
    pr[threadIdx.x >> 6] = ar;
    pb[threadIdx.x >> 6] = ab;
  }
  __syncthreads();
  // one pair per workgroup, reduced on the host after the step's synchronisation (586 atomics on
  // two words cost 14 us: same-address atomics serialise in L2)
  if (threadIdx.x == 0) {
    rsmax[2 * blockIdx.x] = fmax(fmax(pr[0], pr[1]), fmax(pr[2], pr[3]));
    rsmax[2 * blockIdx.x + 1] = fmax(fmax(pb[0], pb[1]), fmax(pb[2], pb[3]));
  }
}

// ---------------------------------------------------------------- the step finished on the device
// What band_batch_sync (pgf_api_band_batch.hip) does on the host after a step's synchronisation, for
// the device-resident controller, which has no synchronisation to do it behind.  ONE wavefront per
// instance (the caller picks the instance from its wavefront's index); stat: the instance's status
// block as b_band_residual and b_band_step_update left it.
//   *diff_out   sqrt of the sum of the step update's partial sums, taken by lane 0 in index order --
//               the order of band_batch_sync, so the bits agree (nred = ceil(N / 256) adds); 0 after
//               a bad pivot, when no step was taken
//   flags_out   [0] bit 0: zero or non-finite pivot; bit 2: the guard's measure (band_residual_rel_of:
//               max |r| / max (|K| |x| + |rhs|) over the pairs, +inf for a NaN or overflowed numerator,
//               denominator 1 when it is 0; a max is order-free, so lane strides and shuffles) misses
//               tol -- only when guard_on, and only behind a clean pivot, as on the host;
//               [1] negative pivots; [2] |I|
//   rejects     [0] += bit 0, [1] += bit 2: the instance's own words, no atomics
// The host repairs an instance above its tolerance on its handle.  Here the step counts as failed:
// kb_dctl_mid / kb_dctl_end reject it with 2 lambda and kb_advance puts the instance back on its
// outer point, over the inaccurate point the step update swapped in -- the reference's own recovery,
// a larger lambda makes K quasi-definite again (step_control.py:80-107).
// rw != nullptr (PGF_BATCH_CTL_REFINE, behind the refinement rounds): the instance's refinement words,
// and bit 2 is band_refine's verdict instead -- the step missed tol as it came out of the solve
// (rw[2], b_band_refine_decide) and the measure is above fail now.
__device__ __forceinline__ void b_band_step_final(const double *__restrict__ stat, int nred, int n_inner,
                                                  bool guard_on, double tol, double *__restrict__ diff_out,
                                                  int *__restrict__ flags_out, int *__restrict__ rejects,
                                                  const int *__restrict__ rw = nullptr, double fail = 0.0) {
  const int lane = threadIdx.x & 63;
  double r = 0.0, den = 0.0;
  int broken = 0;
  for (int k = lane; k < nred; k += 64) {
    const double rk = stat[2 * k];
    if (!(rk == rk) || !(rk <= 1.79e308))
      broken = 1;
    else
      r = fmax(r, rk);
    den = fmax(den, stat[2 * k + 1]);  // (fmax drops a NaN, as std::max(den, NaN) does)
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    r = fmax(r, __shfl_xor(r, off));
    den = fmax(den, __shfl_xor(den, off));
    broken |= __shfl_xor(broken, off);
  }
  if (lane != 0) return;
  const double rel = broken ? __builtin_huge_val() : r / (den > 0.0 ? den : 1.0);
  const int bad = stat[3 * nred] != 0.0 ? 1 : 0;
  double sum = 0.0;
  for (int k = 0; k < nred; ++k) sum += stat[2 * nred + k];
  const bool above = rw ? (rw[2] != 0 && !(rel <= fail)) : !(rel <= tol);
  const int miss = (!bad && guard_on && above) ? 4 : 0;
  *diff_out = bad ? 0.0 : sqrt(sum);
  flags_out[0] = bad | miss;
  flags_out[1] = (int)stat[3 * nred + 1];
  flags_out[2] = n_inner;
  if (bad) ++rejects[0];
  if (miss) ++rejects[1];
}

// ---------------------------------------------------------------- refinement inside the loop
// band_refine's rule (pgf_api_band.hip) for one instance and one round, ONE wavefront per instance;
// stat as above.  The measure is band_residual_rel_of of the pairs as they stand: the step's in
// round 0, the last round's behind it.  w: the instance's refinement words, which the round's
// launches read as their ctl -- [0] stays 0 (no assembly, kept factors, no write of ctl[1]), [1] a
// round ran, [2] the step missed tol as it came out of the solve (for b_band_step_final), [3] sits
// this round out.  A round runs for an instance that is live, has a clean pivot and the guard on,
// while tol < rel < 1; a second one only behind a first that made the measure fall (*prev).
// cnt: [0] steps refined, [1] rounds run -- the instance's own words, no atomics.
__device__ __forceinline__ void b_band_refine_decide(const double *__restrict__ stat, int nred, bool frozen,
                                                     bool guard_on, double tol, int round,
                                                     int *__restrict__ w, double *__restrict__ prev,
                                                     int *__restrict__ cnt) {
  const int lane = threadIdx.x & 63;
  double r = 0.0, den = 0.0;
  int broken = 0;
  for (int k = lane; k < nred; k += 64) {
    const double rk = stat[2 * k];
    if (!(rk == rk) || !(rk <= 1.79e308))
      broken = 1;
    else
      r = fmax(r, rk);
    den = fmax(den, stat[2 * k + 1]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    r = fmax(r, __shfl_xor(r, off));
    den = fmax(den, __shfl_xor(den, off));
    broken |= __shfl_xor(broken, off);
  }
  if (lane != 0) return;
  const double rel = broken ? __builtin_huge_val() : r / (den > 0.0 ? den : 1.0);
  const bool live = !frozen && guard_on && stat[3 * nred] == 0.0;
  bool go;
  if (round == 0) {
    const bool missed = live && !(rel <= tol);
    w[2] = missed ? 1 : 0;
    go = missed && rel > tol && rel < 1.0;
    if (go) ++cnt[0];
  } else {
    go = live && w[1] != 0 && rel < *prev && rel > tol && rel < 1.0;
  }
  w[0] = 0;
  w[1] = go ? 1 : 0;
  w[3] = go ? 0 : 1;
  if (go) {
    *prev = rel;
    ++cnt[1];
  }
}
