// Device-side bodies of the bordered band's kernels: shared by the kernels of one handle
// (pgf_border.hip, which describes the block elimination and the storage) and their batched twins
// (the same file: instance = blockIdx.y, pointers from the instance's BandInst, the sizes
// from BandShape).  Every body takes the arguments its kernel took, in the same order, and reads its
// place from blockIdx.x / threadIdx.x; both callers pass the same arguments, so an instance of a
// batch computes the bits the single handle computes -- which keeps the deterministic, atomics-free
// summation of b_border_gram and the Dot2 accumulation of b_border_ctv as they are.  Both files are
// compiled with -ffp-contract=off (explicit fma() only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgf_bcr_dev.h"
#include "pgf_sparse.h"

// ---------------------------------------------------------------- assembly
// diagonal of the band and of D: lamb (inactive variable), 1 (active variable), -delta (constraint),
// 1 (padding of D)
__device__ __forceinline__ void b_border_set_diag(int n, int m, const int *__restrict__ pos,
                                                  const uint8_t *__restrict__ mask, double lamb, double delta,
                                                  double *__restrict__ band, int ldb, int Nb,
                                                  double *__restrict__ Dd, int k, int kp) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int N = n + m;
  if (i >= N + kp - k) return;
  if (i >= N) {
    const int j = k + i - N;
    Dd[(int64_t)j * kp + j] = 1.0;
    return;
  }
  double v;
  if (i < n)
    v = mask[i] ? 1.0 : lamb;
  else
    v = -delta;
  const int p = pos[i];
  if (p < Nb)
    band[(int64_t)p * ldb] = v;
  else
    Dd[(int64_t)(p - Nb) * kp + (p - Nb)] = v;
}

// ---------------------------------------------------------------- Y = inv(B) C, 8 x 8 blocks
// (the recurrences and the panel's layout: pgf_border.hip)
#define MB_MAXQ 8  // panel columns per lane: R / 8 <= 8

// 64 threads, block blockIdx.x
__device__ __forceinline__ void b_mbcr_extract(const double *__restrict__ band, int ldb, int bw,
                                               const double *__restrict__ C, int R, int N, int nb,
                                               double *__restrict__ D, double *__restrict__ L,
                                               double *__restrict__ U, double *__restrict__ P) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const int r = lane >> 3, c = lane & 7;
  const int gr = i * 8 + r, gc = i * 8 + c;
  double d = (r == c) ? 1.0 : 0.0;  // identity padding of the last block
  if (gr < N && gc < N) {
    const int hi = max(gr, gc), lo = min(gr, gc);
    d = (hi - lo <= bw) ? band[(int64_t)hi * ldb + (hi - lo)] : 0.0;
  }
  D[(int64_t)i * 64 + lane] = d;
  double l = 0.0;  // L_i[r][c] = K[8i + r][8(i-1) + c]
  if (i > 0 && gr < N) {
    const int dist = gr - ((i - 1) * 8 + c);
    if (dist <= bw) l = band[(int64_t)gr * ldb + dist];
  }
  L[(int64_t)i * 64 + lane] = l;
  double u = 0.0;  // U_i[r][c] = K[8(i+1) + c][8i + r]
  if (i + 1 < nb && gr < N) {
    const int rr = (i + 1) * 8 + c;
    const int dist = rr - gr;
    if (rr < N && dist <= bw) u = band[(int64_t)rr * ldb + dist];
  }
  U[(int64_t)i * 64 + lane] = u;
  for (int cc = c; cc < R; cc += 8) P[(int64_t)gr * R + cc] = (gr < N) ? C[(int64_t)gr * R + cc] : 0.0;
}

// kept block i = 2 s j: inverts its eliminated neighbours i - s and i + s itself (the inverse of
// i + s is stored for the back-substitution) and reduces D, L, U and the panel
__device__ __forceinline__ void b_mbcr_level(double *D, double *L, double *U, double *__restrict__ Dinv,
                                             double *P, int R, int nb, int s) {
  __shared__ double A[64], Bm[64], T[64], pn[8 * 64];
  const int i = (int)blockIdx.x * 2 * s;
  if (i >= nb) return;
  const int lane = threadIdx.x, r = lane >> 3, c = lane & 7;
  double dv = D[(int64_t)i * 64 + lane];
  double lnew = 0.0, unew = 0.0;
  double fv[MB_MAXQ];
#pragma unroll
  for (int q = 0; q < MB_MAXQ; ++q) {
    const int cc = c + 8 * q;
    fv[q] = (cc < R) ? P[((int64_t)i * 8 + r) * R + cc] : 0.0;
  }
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const int nbr = side ? i + s : i - s;
    if (nbr < 0 || nbr >= nb) continue;  // (uniform over the workgroup)
    const double *Mi = side ? U : L;     // coupling of i to the neighbour
    const double *Mn1 = side ? L : U;    // the neighbour's coupling back to i
    const double *Mn2 = side ? U : L;    // the neighbour's coupling onwards
    __syncthreads();
    A[lane] = Mi[(int64_t)i * 64 + lane];
    Bm[lane] = D[(int64_t)nbr * 64 + lane];
    __syncthreads();
    int bad = 0;
    (void)gj_inverse8(Bm, lane, &bad);  // (the solve phase's own reduction reports the pivots of B)
    __syncthreads();
    if (side) Dinv[(int64_t)nbr * 64 + lane] = Bm[lane];
    const double al = mm8(A, Bm, r, c);  // alpha = L_i inv(D_left)  /  gamma = U_i inv(D_right)
    T[lane] = al;
    __syncthreads();
    Bm[lane] = Mn1[(int64_t)nbr * 64 + lane];
    for (int idx = lane; idx < 8 * R; idx += 64) pn[idx] = P[(int64_t)nbr * 8 * R + idx];
    __syncthreads();
    dv -= mm8(T, Bm, r, c);
#pragma unroll
    for (int q = 0; q < MB_MAXQ; ++q) {
      const int cc = c + 8 * q;
      if (cc < R) {
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc = fma(T[r * 8 + k], pn[k * R + cc], acc);
        fv[q] -= acc;
      }
    }
    __syncthreads();
    Bm[lane] = Mn2[(int64_t)nbr * 64 + lane];
    __syncthreads();
    const double nw = -mm8(T, Bm, r, c);  // couples i to i -+ 2 s
    if (side)
      unew = nw;
    else
      lnew = nw;
  }
  D[(int64_t)i * 64 + lane] = dv;
  L[(int64_t)i * 64 + lane] = lnew;
  U[(int64_t)i * 64 + lane] = unew;
#pragma unroll
  for (int q = 0; q < MB_MAXQ; ++q) {
    const int cc = c + 8 * q;
    if (cc < R) P[((int64_t)i * 8 + r) * R + cc] = fv[q];
  }
}

// X_i = inv(D_i) (F_i - L_i X_{i-s} - U_i X_{i+s}) for the blocks eliminated at stride s
// (i = s, 3 s, ...); s == 0: the last remaining block 0, whose inverse is formed here.  X replaces F.
__device__ __forceinline__ void b_mbcr_back(const double *__restrict__ D, double *__restrict__ Dinv,
                                            const double *__restrict__ L, const double *__restrict__ U,
                                            double *__restrict__ P, int R, int nb, int s) {
  __shared__ double Lm[64], Um[64], Im[64], xl[8 * 64], xr[8 * 64], tt[8 * 64];
  const int i = s + (int)blockIdx.x * 2 * s;
  if (i >= nb) return;
  const int lane = threadIdx.x, r = lane >> 3, c = lane & 7;
  const int le = i - s, ri = i + s;
  const bool hl = s > 0 && le >= 0, hr = s > 0 && ri < nb;
  if (s == 0) {
    Im[lane] = D[lane];
    __syncthreads();
    int bad = 0;
    (void)gj_inverse8(Im, lane, &bad);
    __syncthreads();
    Dinv[lane] = Im[lane];
  } else {
    Im[lane] = Dinv[(int64_t)i * 64 + lane];
  }
  Lm[lane] = L[(int64_t)i * 64 + lane];
  Um[lane] = U[(int64_t)i * 64 + lane];
  for (int idx = lane; idx < 8 * R; idx += 64) {
    xl[idx] = hl ? P[(int64_t)le * 8 * R + idx] : 0.0;
    xr[idx] = hr ? P[(int64_t)ri * 8 * R + idx] : 0.0;
  }
  __syncthreads();
  for (int cc = c; cc < R; cc += 8) {
    double acc = P[((int64_t)i * 8 + r) * R + cc];
    if (hl)
#pragma unroll
      for (int k = 0; k < 8; ++k) acc = fma(-Lm[r * 8 + k], xl[k * R + cc], acc);
    if (hr)
#pragma unroll
      for (int k = 0; k < 8; ++k) acc = fma(-Um[r * 8 + k], xr[k * R + cc], acc);
    tt[r * R + cc] = acc;
  }
  __syncthreads();
  for (int cc = c; cc < R; cc += 8) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) acc = fma(Im[r * 8 + k], tt[k * R + cc], acc);
    P[((int64_t)i * 8 + r) * R + cc] = acc;
  }
}

// ---------------------------------------------------------------- tall-skinny products
// part[chunk] = C[rows]' Y[rows] (kp x kp) over a fixed chunk of SP_BORDER_CHUNK rows; the chunks are
// summed in index order by b_border_factor_S: deterministic, no same-address atomics.  Plain FMA:
// per row 2 kp^2 flops against 16 kp bytes, kp / 8 <= 8 flops per byte -- below the FP64 ridge of
// the device, the launch is bound by reading C and Y once.  256 threads, chunk blockIdx.x.
__device__ __forceinline__ void b_border_gram(const double *__restrict__ C, const double *__restrict__ Y,
                                              int Nb, int kp, double *__restrict__ part) {
  __shared__ double cs[16 * 64], ys[16 * 64];
  const int t = threadIdx.x;
  const int i0 = (int)blockIdx.x * SP_BORDER_CHUNK, i1 = min(Nb, i0 + SP_BORDER_CHUNK);
  const int ne = kp * kp / 256;  // outputs per thread: 1, 4, 9, 16
  double acc[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.0;
  for (int base = i0; base < i1; base += 16) {
    const int rows = min(16, i1 - base);
    for (int idx = t; idx < 16 * kp; idx += 256) {
      const bool in = idx / kp < rows;
      cs[idx] = in ? C[(int64_t)base * kp + idx] : 0.0;
      ys[idx] = in ? Y[(int64_t)base * kp + idx] : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (e < ne) {
        const int idx = t + 256 * e, a = idx / kp, b = idx % kp;
#pragma unroll
        for (int rr = 0; rr < 16; ++rr) acc[e] = fma(cs[rr * kp + a], ys[rr * kp + b], acc[e]);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < 16; ++e)
    if (e < ne) part[(int64_t)blockIdx.x * kp * kp + t + 256 * e] = acc[e];
}

// s + e = a + b exactly (Knuth's TwoSum; the callers are compiled without contraction)
__device__ __forceinline__ void two_sum(double a, double b, double &s, double &e) {
  s = a + b;
  const double bb = s - a;
  e = (a - (s - bb)) + (b - bb);
}

// partv[chunk] = (C[rows]' v[rows], |C[rows]|' |v[rows]|, tail), 3 kp doubles per chunk.  The dot
// product is accumulated with error-free products and sums (Ogita, Rump, Oishi: Dot2) and leaves
// as head + tail: in the border rows of the residual the terms of a dense row cancel, its partial
// sums are far larger than the result, and a plain float64 sum carries rounding of the size of the
// residual it is to measure.  256 threads, chunk blockIdx.x.
__device__ __forceinline__ void b_border_ctv(const double *__restrict__ C, const double *__restrict__ v,
                                             int Nb, int kp, double *__restrict__ partv) {
  __shared__ double red[256], redc[256], reda[256];
  const int t = threadIdx.x, j = t % kp, rg = t / kp, nrg = 256 / kp;
  const int i0 = (int)blockIdx.x * SP_BORDER_CHUNK, i1 = min(Nb, i0 + SP_BORDER_CHUNK);
  double acc = 0.0, comp = 0.0, aa = 0.0;
  if (rg < nrg)
    for (int i = i0 + rg; i < i1; i += nrg) {
      const double cv = C[(int64_t)i * kp + j], x = v[i];
      const double p = cv * x, pe = fma(cv, x, -p);
      double e;
      two_sum(acc, p, acc, e);
      comp += e + pe;
      aa += fabs(p);
    }
  red[t] = acc;
  redc[t] = comp;
  reda[t] = aa;
  __syncthreads();
  if (t < kp) {
    double sv = 0.0, sc = 0.0, sa = 0.0;
    for (int g = 0; g < nrg; ++g) {
      double e;
      two_sum(sv, red[g * kp + t], sv, e);
      sc += e + redc[g * kp + t];
      sa += reda[g * kp + t];
    }
    partv[(int64_t)blockIdx.x * 3 * kp + t] = sv;
    partv[(int64_t)blockIdx.x * 3 * kp + kp + t] = sa;
    partv[(int64_t)blockIdx.x * 3 * kp + 2 * kp + t] = sc;
  }
}

// ---------------------------------------------------------------- S = D - C' Y and its L D L'
// One workgroup of 256 threads, S in LDS (kp <= 64: 32 KB); lower triangle only (D is stored that
// way, and of the computed C' Y, symmetric up to rounding, the lower half is taken).  Right-looking,
// no pivoting; out: L strictly below the diagonal, 1 / d on it; sflags[0] zero / non-finite pivot,
// [1] negative pivots.
__device__ __forceinline__ void b_border_factor_S(const double *__restrict__ Dd, const double *__restrict__ part,
                                                  int nchunk, int kp, double *__restrict__ Sfac,
                                                  int *__restrict__ sflags) {
  __shared__ double S[64 * 64];
  __shared__ double w[64];
  const int t = threadIdx.x;
  for (int idx = t; idx < kp * kp; idx += 256) {
    const int a = idx / kp, b = idx % kp;
    double v = 0.0;
    if (a >= b) {
      v = Dd[idx];
      for (int c = 0; c < nchunk; ++c) v -= part[(int64_t)c * kp * kp + idx];
    }
    S[idx] = v;
  }
  int neg = 0, bad = 0;
  for (int j = 0; j < kp; ++j) {
    __syncthreads();
    const double d = S[j * kp + j];
    const bool isbad = (d == 0.0) || !(fabs(d) <= 1.79e308);
    const double dinv = isbad ? 0.0 : recip2(d);
    bad |= isbad ? 1 : 0;
    neg += (d < 0.0) ? 1 : 0;
    if (t > j && t < kp) w[t] = S[t * kp + j];
    __syncthreads();
    if (t > j && t < kp) S[t * kp + j] = w[t] * dinv;
    if (t == j) S[j * kp + j] = dinv;
    const int rem = kp - 1 - j;
    for (int idx = t; idx < rem * rem; idx += 256) {
      const int i = j + 1 + idx / rem, c = j + 1 + idx % rem;
      if (c <= i) S[i * kp + c] = fma(-(w[i] * dinv), w[c], S[i * kp + c]);
    }
  }
  __syncthreads();
  for (int idx = t; idx < kp * kp; idx += 256) Sfac[idx] = S[idx];
  if (t == 0) {
    sflags[0] = bad;
    sflags[1] = neg;
  }
}

// z = inv(S) (rb - sum of the chunks' C' v); z also into x[Nb, Nb + k); the pivot flags of S merge
// into those the reduction of B has just written (flags[0] zero pivot, flags[1] negative pivots).
// One wavefront.
__device__ __forceinline__ void b_border_small_solve(const double *__restrict__ Sfac, int k, int kp,
                                                     const double *__restrict__ rb,
                                                     const double *__restrict__ partv, int nchunk,
                                                     const int *__restrict__ sflags, double *__restrict__ z,
                                                     double *__restrict__ xb, int *__restrict__ flags) {
  __shared__ double Ls[64 * 64];
  __shared__ double tv[64];
  const int t = threadIdx.x;
  for (int idx = t; idx < kp * kp; idx += 64) Ls[idx] = Sfac[idx];
  if (t < kp) {
    double v = rb[t];
    for (int c = 0; c < nchunk; ++c) v -= partv[(int64_t)c * 3 * kp + t] + partv[(int64_t)c * 3 * kp + 2 * kp + t];
    tv[t] = v;
  }
  __syncthreads();
  for (int j = 0; j < kp; ++j) {  // L w = t
    const double wj = tv[j];
    __syncthreads();
    if (t > j && t < kp) tv[t] = fma(-Ls[t * kp + j], wj, tv[t]);
    __syncthreads();
  }
  if (t < kp) tv[t] *= Ls[t * kp + t];
  __syncthreads();
  for (int j = kp - 1; j >= 0; --j) {  // L' z = w
    const double xj = tv[j];
    __syncthreads();
    if (t < j) tv[t] = fma(-Ls[j * kp + t], xj, tv[t]);
    __syncthreads();
  }
  if (t < kp) z[t] = tv[t];
  if (t < k) xb[t] = tv[t];
  if (t == 0) {
    flags[0] |= sflags[0];
    flags[1] += sflags[1];
  }
}

// xa = v - Y z; 256 threads
__device__ __forceinline__ void b_border_update(int Nb, int k, int kp, const double *__restrict__ Y,
                                                const double *__restrict__ z, double *__restrict__ x) {
  __shared__ double zs[64];
  if (threadIdx.x < kp) zs[threadIdx.x] = z[threadIdx.x];
  __syncthreads();
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= Nb) return;
  double acc = x[i];
  for (int j = 0; j < k; ++j) acc = fma(-Y[(int64_t)i * kp + j], zs[j], acc);
  x[i] = acc;
}

// ---------------------------------------------------------------- accuracy guard
// r = rhs0 - K x over all Nb + k rows and the pairs (max |r|, max (|K| |x| + |rhs0|)) that
// b_band_residual writes, so that the host side of the guard (sparse_residual_rel, sparse_refine)
// serves the bordered route as it is.  Workgroup b < ceil(Nb / 256): 256 band rows, B x_a + C z;
// the next one: the border rows, C' x_a (from the chunk sums of b_border_ctv) + D z; any further
// pair is zero.  The pivot flags ride along behind the pairs as in b_band_residual.
__device__ __forceinline__ void b_border_residual(
    const double *__restrict__ band, int ldb, int bw, int Nb, int k, int kp, const double *__restrict__ C,
    const double *__restrict__ Dd, const double *__restrict__ partv, int nchunk,
    const double *__restrict__ x, const double *__restrict__ rhs0, double *__restrict__ r,
    double *__restrict__ rsmax, const int *__restrict__ flags, int nred) {
  if (blockIdx.x == 0 && threadIdx.x < 4) rsmax[3 * nred + threadIdx.x] = (double)flags[threadIdx.x];
  __shared__ double zs[64];
  __shared__ double pr[4], pb[4];
  const int t = threadIdx.x;
  if (t < 64) zs[t] = (t < k) ? x[Nb + t] : 0.0;
  __syncthreads();
  const int nbB = (Nb + 255) / 256;
  double ar = 0.0, ab = 0.0;
  if ((int)blockIdx.x < nbB) {
    const int i = blockIdx.x * 256 + t;
    if (i < Nb) {
      double acc = rhs0[i];
      ab = fabs(acc);
      const double *row = band + (int64_t)i * ldb;
      for (int d = 0; d <= bw && d <= i; ++d) {
        acc = fma(-row[d], x[i - d], acc);
        ab += fabs(row[d] * x[i - d]);
      }
      for (int d = 1; d <= bw && i + d < Nb; ++d) {
        const double kv = band[(int64_t)(i + d) * ldb + d];
        acc = fma(-kv, x[i + d], acc);
        ab += fabs(kv * x[i + d]);
      }
      for (int j = 0; j < k; ++j) {
        const double cv = C[(int64_t)i * kp + j];
        acc = fma(-cv, zs[j], acc);
        ab += fabs(cv * zs[j]);
      }
      r[i] = acc;
      ar = (acc == acc) ? fabs(acc) : __builtin_huge_val();
    }
  } else if ((int)blockIdx.x == nbB) {
    if (t < k) {
      double acc = rhs0[Nb + t];
      ab = fabs(acc);
      // head + tail of rhs - C' x_a - D z, every sum and product error-free
      double comp = 0.0, e;
      for (int c = 0; c < nchunk; ++c) {
        two_sum(acc, -partv[(int64_t)c * 3 * kp + t], acc, e);
        comp += e - partv[(int64_t)c * 3 * kp + 2 * kp + t];
        ab += partv[(int64_t)c * 3 * kp + kp + t];
      }
      for (int l = 0; l < k; ++l) {
        const double dv = Dd[(int64_t)max(t, l) * kp + min(t, l)];
        const double p = dv * zs[l], pe = fma(dv, zs[l], -p);
        two_sum(acc, -p, acc, e);
        comp += e - pe;
        ab += fabs(p);
      }
      acc += comp;
      r[Nb + t] = acc;
      ar = (acc == acc) ? fabs(acc) : __builtin_huge_val();
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    ar = fmax(ar, __shfl_down(ar, off));
    ab = fmax(ab, __shfl_down(ab, off));
  }
  if ((t & 63) == 0) {
    pr[t >> 6] = ar;
    pb[t >> 6] = ab;
  }
  __syncthreads();
  if (t == 0) {
    rsmax[2 * blockIdx.x] = fmax(fmax(pr[0], pr[1]), fmax(pr[2], pr[3]));
    rsmax[2 * blockIdx.x + 1] = fmax(fmax(pb[0], pb[1]), fmax(pb[2], pb[3]));
  }
}
