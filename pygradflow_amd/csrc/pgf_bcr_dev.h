// Device helpers of the 8 x 8 block cyclic reductions (pgf_sparse.hip: one right-hand side;
// pgf_border.hip: a panel of right-hand sides): the reciprocal, the in-place block inverse and the
// block product, one wavefront per block, lane <-> (row, col).
#pragma once

#include <hip/hip_runtime.h>

__device__ __forceinline__ double recip2(double d) {
  double r = __builtin_amdgcn_rcp(d);
  double e = fma(-d, r, 1.0);
  r = fma(r, e, r);
  e = fma(-d, r, 1.0);
  return fma(r, e, r);
}

// in-place Gauss-Jordan inverse of the 8 x 8 block in LDS (one wavefront, lane = (r, c));
// returns the number of negative pivots, sets *bad on a zero / non-finite pivot
__device__ __forceinline__ int gj_inverse8(double *M, int lane, int *bad) {
  const int r = lane >> 3, c = lane & 7;
  int neg = 0;
  double mrc = M[lane];  // own entry: stays in a register between the steps
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const double p = M[k * 8 + k];
    const bool isbad = (p == 0.0) || !(fabs(p) <= 1.79e308);
    *bad |= isbad ? 1 : 0;
    neg += (p < 0.0) ? 1 : 0;
    // v_rcp_f64 + two Newton steps (full precision) instead of the ~30-instruction IEEE
    // division: eight of them sat on every block operation's dependent chain
    const double d = isbad ? 0.0 : recip2(p);
    const double mrk = M[r * 8 + k], mkc = M[k * 8 + c];
    double v;
    if (r == k && c == k)
      v = d;
    else if (r == k)
      v = mkc * d;
    else if (c == k)
      v = -mrk * d;
    else
      v = fma(-mrk * d, mkc, mrc);
    M[lane] = v;  // all lanes have read before any lane writes (one wavefront, lockstep)
    mrc = v;
  }
  return neg;
}

// 8 x 8 product helper: out[r][c] = sum_k A[r][k] B[k][c], operands in LDS
__device__ __forceinline__ double mm8(const double *A, const double *B, int r, int c) {
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < 8; ++k) acc = fma(A[r * 8 + k], B[k * 8 + c], acc);
  return acc;
}
