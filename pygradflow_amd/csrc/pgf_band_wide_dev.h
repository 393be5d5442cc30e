// Device-side bodies of the wide block cyclic reduction (B x B blocks, B in {16, 32, 64}): shared by
// the kernels of one handle (pgf_band_wide.hip, which describes the algorithm and the storage) and
// their batched twins (the same file: instance = blockIdx.y, pointers from the instance's
// BandInst).  Each body takes its block index, its pointers and its LDS scratch as arguments; both
// callers pass the same arguments in the same order, so an instance of a batch computes the bits the
// single handle computes.  Both files are compiled with the same contraction rules (no
// -ffp-contract=off).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

typedef double bw_double4 __attribute__((ext_vector_type(4)));

#define BW_THREADS 256

__device__ __forceinline__ double bw_recip(double d) {
  double r = __builtin_amdgcn_rcp(d);
  double e = fma(-d, r, 1.0);
  r = fma(r, e, r);
  e = fma(-d, r, 1.0);
  return fma(r, e, r);
}

// block extraction from the band (+ identity padding of the last block), matrix part: D, L, U of
// block i; block 0 also clears the pivot flags
template <int B>
__device__ __forceinline__ void bw_extract_matrix(const double *__restrict__ band, int ldb, int bw, int N,
                                                  int nb, double *__restrict__ D, double *__restrict__ L,
                                                  double *__restrict__ U, int *__restrict__ flags, int i) {
  const int tid = threadIdx.x;
  if (i == 0 && tid < 4) flags[tid] = 0;  // (every kernel that sets them runs after this one)
  const int64_t base = (int64_t)i * B * B;
  for (int p = tid; p < B * B; p += BW_THREADS) {
    const int r = p / B, c = p % B;
    const int gr = i * B + r, gc = i * B + c;
    double d = (r == c) ? 1.0 : 0.0;
    if (gr < N && gc < N) {
      const int hi = max(gr, gc), lo = min(gr, gc);
      d = (hi - lo <= bw) ? band[(int64_t)hi * ldb + (hi - lo)] : 0.0;
    }
    D[base + p] = d;
    // L_i[r][c] = K[B i + r][B (i-1) + c]
    double l = 0.0;
    if (i > 0 && gr < N) {
      const int dist = gr - ((i - 1) * B + c);
      if (dist <= bw) l = band[(int64_t)gr * ldb + dist];
    }
    L[base + p] = l;
    // U_i[r][c] = K[B i + r][B (i+1) + c] = K[B (i+1) + c][B i + r]
    double u = 0.0;
    if (i + 1 < nb && gr < N) {
      const int rr = (i + 1) * B + c;
      const int dist = rr - gr;
      if (rr < N && dist <= bw) u = band[(int64_t)rr * ldb + dist];
    }
    U[base + p] = u;
  }
}

// right-hand side part: block i of rhs is copied to F and, for the guard, to rhs0
template <int B>
__device__ __forceinline__ void bw_extract_rhs(const double *__restrict__ rhs, int N, double *__restrict__ F,
                                               double *__restrict__ rhs0, int i) {
  const int tid = threadIdx.x;
  if (tid < B) {
    const int g = i * B + tid;
    const double v = (g < N) ? rhs[g] : 0.0;
    F[(int64_t)i * B + tid] = v;
    if (rhs0 && g < N) rhs0[g] = v;
  }
}

// In-place Gauss-Jordan inverse of the B x B block M (LDS, row stride B + 1) by the whole
// workgroup, no pivoting.  Returns (in thread 0) the number of negative pivots; sets *bad on a
// zero or non-finite pivot.
template <int B>
__device__ __forceinline__ int bw_gj_inverse(double *M, int tid, int *bad) {
  constexpr int LD = B + 1, E = B * B / BW_THREADS > 0 ? B * B / BW_THREADS : 1;
  int neg = 0;
  double own[E];
#pragma unroll
  for (int e = 0; e < E; ++e) {
    const int p = tid + e * BW_THREADS;
    own[e] = (p < B * B) ? M[(p / B) * LD + p % B] : 0.0;
  }
  for (int k = 0; k < B; ++k) {
    const double piv = M[k * LD + k];
    const bool isbad = (piv == 0.0) || !(fabs(piv) <= 1.79e308);
    *bad |= isbad ? 1 : 0;
    neg += (piv < 0.0) ? 1 : 0;
    const double d = isbad ? 0.0 : bw_recip(piv);
    double v[E];
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int p = tid + e * BW_THREADS;
      const int r = p / B, c = p % B;
      const double mrk = M[r * LD + k], mkc = M[k * LD + c];
      if (r == k && c == k)
        v[e] = d;
      else if (r == k)
        v[e] = mkc * d;
      else if (c == k)
        v[e] = -mrk * d;
      else
        v[e] = fma(-mrk * d, mkc, own[e]);
    }
    __syncthreads();  // every thread has read row / column k
#pragma unroll
    for (int e = 0; e < E; ++e) {
      const int p = tid + e * BW_THREADS;
      if (p < B * B) {
        M[(p / B) * LD + p % B] = v[e];
        own[e] = v[e];
      }
    }
    __syncthreads();
  }
  return neg;
}

template <int B>
__device__ __forceinline__ void bw_invert_block(const double *__restrict__ D,
                                                double *__restrict__ Dinv, int i, double *M,
                                                int *__restrict__ flags,
                                                int *__restrict__ negcnt) {
  constexpr int LD = B + 1;
  const int tid = threadIdx.x;
  const int64_t base = (int64_t)i * B * B;
  for (int p = tid; p < B * B; p += BW_THREADS) M[(p / B) * LD + p % B] = D[base + p];
  __syncthreads();
  int bad = 0;
  const int neg = bw_gj_inverse<B>(M, tid, &bad);
  for (int p = tid; p < B * B; p += BW_THREADS) Dinv[base + p] = M[(p / B) * LD + p % B];
  // (the pivots are the same in every thread: thread 0 reports)
  if (tid == 0) {
    if (bad) atomicOr(&flags[0], 1);
    negcnt[i] = neg;
  }
}

// One 16 x 16 tile of acc += A[r0.., :] Bm[:, c0..] (K = B) on v_mfma_f64_16x16x4_f64.
// Operand layout: A: lane l holds A[l & 15][l >> 4], B: B[l >> 4][l & 15];
// C/D: row (l >> 4) + 4 reg, column l & 15 (pgf_factor2.hip, tile_msub).
// neg: accumulate -A Bm instead.
template <int B>
__device__ __forceinline__ bw_double4 bw_tile(const double *A, int lda, const double *Bm, int ldbm,
                                              int r0, int c0, bw_double4 acc, int lane, bool neg) {
  const int l15 = lane & 15, l4 = lane >> 4;
  const double *pa = A + (int64_t)(r0 + l15) * lda + l4;
  const double *pb = Bm + (int64_t)l4 * ldbm + c0 + l15;
#pragma unroll
  for (int k0 = 0; k0 < B; k0 += 4) {
    const double a = pa[k0];
    const double b = pb[(int64_t)k0 * ldbm];
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(neg ? -a : a, b, acc, 0, 0, 0);
  }
  return acc;
}

// (T f_e)[row] for the row of T (LDS) at Trow: the forward update f_i -= T f_e of k_bw_reduce and
// of k_bw_fwd -- one function, one operation order, the same bits
template <int B>
__device__ __forceinline__ double bw_f_dot(const double *Trow, const double *__restrict__ fe) {
  double acc = 0.0;
#pragma unroll 8
  for (int k = 0; k < B; ++k) acc = fma(Trow[k], fe[k], acc);
  return acc;
}

// Reduce the kept blocks of this level: i = 0, 2s, 4s, ...  The eliminated neighbours are not
// written at this level, every kept block only writes its own D, L, U, F: no races.
// KEEP: also store the multipliers T (Mr[i - s], Ml[i + s]: each belongs to one eliminated block and
// one kept block, so nobody else writes them).  RHS false: no right-hand side is carried (F unused).
// T: B x (B + 1) doubles of LDS (alpha, then gamma); i: the kept block.
template <int B, bool KEEP, bool RHS>
__device__ __forceinline__ void bw_reduce_block(double *__restrict__ D, double *__restrict__ L,
                                                double *__restrict__ U, double *__restrict__ F,
                                                const double *__restrict__ Dinv, double *__restrict__ Mr,
                                                double *__restrict__ Ml, int nb, int s, int i, double *T) {
  constexpr int LD = B + 1, NT = (B / 16) * (B / 16);  // 16 x 16 tiles of a block
  constexpr int TPW = NT >= 4 ? NT / 4 : 1;            // tiles per wavefront
  constexpr int BB = B * B;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int le = i - s, ri = i + s;
  const int64_t bi = (int64_t)i * BB;
  const int l4 = lane >> 4, l15 = lane & 15;
  auto tile_rc = [&](int t, int &r0, int &c0) {
    const int tt = wave + 4 * t;
    r0 = (tt / (B / 16)) * 16;
    c0 = (tt % (B / 16)) * 16;
  };
  const bool busy = wave < NT;  // B = 16: one tile, wavefront 0
  // D_i into the accumulators
  bw_double4 dacc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    int r0, c0;
    tile_rc(t, r0, c0);
#pragma unroll
    for (int g = 0; g < 4; ++g)
      dacc[t][g] = busy ? D[bi + (int64_t)(r0 + l4 + 4 * g) * B + c0 + l15] : 0.0;
  }
  double fv = (RHS && tid < B) ? F[(int64_t)i * B + tid] : 0.0;
  // two sides: (coupling of i, eliminated neighbour, its coupling further out, output)
  for (int side = 0; side < 2; ++side) {
    const int e = side == 0 ? le : ri;
    double *Ci = side == 0 ? L : U;        // L_i or U_i
    const double *Ce = side == 0 ? U : L;  // block of e that couples back to i
    const double *Co = side == 0 ? L : U;  // block of e that couples further out
    if (e < 0 || e >= nb) {
      // no neighbour on this side: the coupling stays zero
      for (int p = tid; p < BB; p += BW_THREADS) Ci[bi + p] = 0.0;
      continue;
    }
    const int64_t be = (int64_t)e * BB;
    // T = C_i inv(D_e)
    if (busy) {
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        int r0, c0;
        tile_rc(t, r0, c0);
        bw_double4 acc = {0.0, 0.0, 0.0, 0.0};
        acc = bw_tile<B>(Ci + bi, B, Dinv + be, B, r0, c0, acc, lane, false);
#pragma unroll
        for (int g = 0; g < 4; ++g) T[(r0 + l4 + 4 * g) * LD + c0 + l15] = acc[g];
      }
    }
    __syncthreads();  // T complete; C_i has been read by everyone
    if (busy) {
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        int r0, c0;
        tile_rc(t, r0, c0);
        // D_i -= T (coupling of e back to i)
        dacc[t] = bw_tile<B>(T, LD, Ce + be, B, r0, c0, dacc[t], lane, true);
        // new coupling of i (two blocks out): -T (coupling of e further out)
        bw_double4 acc = {0.0, 0.0, 0.0, 0.0};
        acc = bw_tile<B>(T, LD, Co + be, B, r0, c0, acc, lane, true);
#pragma unroll
        for (int g = 0; g < 4; ++g) Ci[bi + (int64_t)(r0 + l4 + 4 * g) * B + c0 + l15] = acc[g];
      }
    }
    if (RHS && tid < B) fv -= bw_f_dot<B>(T + tid * LD, F + (int64_t)e * B);  // f_i -= T f_e
    if (KEEP) {
      double *M = (side == 0 ? Mr : Ml) + be;
      for (int p = tid; p < BB; p += BW_THREADS) M[p] = T[(p / B) * LD + p % B];
    }
    __syncthreads();  // T is read by everyone before the other side overwrites it
  }
  if (busy) {
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
      int r0, c0;
      tile_rc(t, r0, c0);
#pragma unroll
      for (int g = 0; g < 4; ++g) D[bi + (int64_t)(r0 + l4 + 4 * g) * B + c0 + l15] = dacc[t][g];
    }
  }
  if (RHS && tid < B) F[(int64_t)i * B + tid] = fv;
}

// y = M v (B x B row-major in global memory, v in LDS), the rows split over 256 / B threads
// each; the result is valid in the first thread of each row's group
template <int B>
__device__ __forceinline__ double bw_matvec(const double *__restrict__ M, const double *v, int tid) {
  constexpr int P = BW_THREADS / B;  // threads per row (16, 8, 4): inside one wavefront
  const int r = tid / P, part = tid % P;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < B / P; ++j) acc = fma(M[(int64_t)r * B + part + j * P], v[part + j * P], acc);
#pragma unroll
  for (int off = P / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
  return acc;
}

// x_i = inv(D_i) (f_i - L_i x_{i-s} - U_i x_{i+s}) for the blocks eliminated at stride s
template <int B>
__device__ __forceinline__ void bw_back_block(const double *__restrict__ Dinv,
                                              const double *__restrict__ L,
                                              const double *__restrict__ U,
                                              const double *__restrict__ F,
                                              double *__restrict__ X, int nb, int s, int i,
                                              double *xl, double *xr, double *t) {
  constexpr int P = BW_THREADS / B;
  const int tid = threadIdx.x;
  const int le = i - s, ri = i + s;
  const bool hl = (s > 0) && le >= 0, hr = (s > 0) && ri < nb;
  if (tid < B) {
    xl[tid] = hl ? X[(int64_t)le * B + tid] : 0.0;
    xr[tid] = hr ? X[(int64_t)ri * B + tid] : 0.0;
  }
  __syncthreads();
  const int64_t bi = (int64_t)i * B * B;
  double a = hl ? bw_matvec<B>(L + bi, xl, tid) : 0.0;
  double b = hr ? bw_matvec<B>(U + bi, xr, tid) : 0.0;
  if (tid % P == 0) t[tid / P] = F[(int64_t)i * B + tid / P] - a - b;
  __syncthreads();
  const double x = bw_matvec<B>(Dinv + bi, t, tid);
  if (tid % P == 0) X[(int64_t)i * B + tid / P] = x;
}

// the last block left (block 0): invert, solve, and sum the per-block negative pivots.
// M: B x (B + 1) doubles, t: B doubles, part: BW_THREADS / 64 ints of LDS
template <int B>
__device__ __forceinline__ void bw_last_block(const double *__restrict__ D, double *__restrict__ Dinv,
                                              const double *__restrict__ F, double *__restrict__ X, int nb,
                                              int *__restrict__ flags, int *__restrict__ negcnt, double *M,
                                              double *t, int *part) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  bw_invert_block<B>(D, Dinv, 0, M, flags, negcnt);
  // x_0 = inv(D_0) f_0 with the inverse still in LDS (block 0 has no neighbours left)
  if (tid < B) t[tid] = F[tid];
  __syncthreads();
  {
    constexpr int P = BW_THREADS / B;
    const int r = tid / P, pt = tid % P;
    double acc = 0.0;
#pragma unroll
    for (int j = 0; j < B / P; ++j) acc = fma(M[r * (B + 1) + pt + j * P], t[pt + j * P], acc);
#pragma unroll
    for (int off = P / 2; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (pt == 0) X[r] = acc;
  }
  // inertia: every block has been inverted exactly once by now
  int cnt = 0;
  for (int i = tid; i < nb; i += BW_THREADS) cnt += negcnt[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_down(cnt, off);
  if (lane == 0) part[wave] = cnt;
  __syncthreads();
  if (tid == 0) {
    int tot = 0;
    for (int w = 0; w < BW_THREADS / 64; ++w) tot += part[w];
    flags[1] = tot;
  }
}

// right-hand side in whole blocks for the solve phase (zero padding), rhs0 <- its copy for the guard
__device__ __forceinline__ void bw_load_row(const double *__restrict__ rhs, int N, int nrows,
                                            double *__restrict__ F, double *__restrict__ rhs0, int g) {
  if (g >= nrows) return;
  const double v = (g < N) ? rhs[g] : 0.0;
  F[g] = v;
  if (rhs0 && g < N) rhs0[g] = v;
}

// forward step of one level for the kept blocks i = 0, 2s, ...: f_i -= Mr[i-s] f_{i-s} + Ml[i+s] f_{i+s}
// (a neighbour that does not exist contributes nothing).  The multiplier is staged in LDS with the
// row stride of k_bw_reduce's T and applied by the same bw_f_dot, left side first.  A kept block
// writes its own f only and reads those of blocks eliminated at this level: no races.
// T: B x (B + 1) doubles of LDS; i: the kept block.
template <int B>
__device__ __forceinline__ void bw_fwd_block(const double *__restrict__ Mr, const double *__restrict__ Ml,
                                             double *__restrict__ F, int nb, int s, int i, double *T) {
  constexpr int LD = B + 1, BB = B * B;
  const int tid = threadIdx.x;
  double fv = (tid < B) ? F[(int64_t)i * B + tid] : 0.0;
  for (int side = 0; side < 2; ++side) {
    const int e = side == 0 ? i - s : i + s;
    if (e < 0 || e >= nb) continue;
    const double *M = (side == 0 ? Mr : Ml) + (int64_t)e * BB;
    for (int p = tid; p < BB; p += BW_THREADS) T[(p / B) * LD + p % B] = M[p];
    __syncthreads();
    if (tid < B) fv -= bw_f_dot<B>(T + tid * LD, F + (int64_t)e * B);
    __syncthreads();  // T is read by everyone before the other side overwrites it
  }
  if (tid < B) F[(int64_t)i * B + tid] = fv;
}

// x_0 = inv(D_0) f_0 (the operation order of bw_last_block's product); t: B doubles of LDS
template <int B>
__device__ __forceinline__ void bw_x0_block(const double *__restrict__ Dinv, const double *__restrict__ F,
                                            double *__restrict__ X, double *t) {
  constexpr int P = BW_THREADS / B;
  const int tid = threadIdx.x;
  if (tid < B) t[tid] = F[tid];
  __syncthreads();
  const double x = bw_matvec<B>(Dinv, t, tid);
  if (tid % P == 0) X[tid / P] = x;
}

// ---- solve phase against the kept factors, a panel of kp right-hand sides (row-major, row stride
// ld >= kp; kp a multiple of 16, at most 64: a wider panel is solved as 64-column slices, P
// pointing at the slice's first column), in place, on
// v_mfma_f64_16x16x4_f64: (B / 16) (kp / 16) <= 16 output tiles, at most four per wavefront.
// Forward step of one level for the kept block i: P_i -= Mr[i-s] P_{i-s} + Ml[i+s] P_{i+s}.
template <int B>
__device__ __forceinline__ void bw_fwd_panel_block(const double *__restrict__ Mr,
                                                   const double *__restrict__ Ml, double *__restrict__ P,
                                                   int ld, int kp, int nb, int s, int i) {
  constexpr int BB = B * B;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l4 = lane >> 4, l15 = lane & 15;
  const int le = i - s, ri = i + s;
  const int tc = kp / 16, nt = (B / 16) * tc;
  double *Pi = P + (int64_t)i * B * ld;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int tt = wave + 4 * t;
    if (tt >= nt) break;  // (uniform over the wavefront)
    const int r0 = (tt / tc) * 16, c0 = (tt % tc) * 16;
    bw_double4 acc;
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = Pi[(int64_t)(r0 + l4 + 4 * g) * ld + c0 + l15];
    if (le >= 0)
      acc = bw_tile<B>(Mr + (int64_t)le * BB, B, P + (int64_t)le * B * ld, ld, r0, c0, acc, lane, true);
    if (ri < nb)
      acc = bw_tile<B>(Ml + (int64_t)ri * BB, B, P + (int64_t)ri * B * ld, ld, r0, c0, acc, lane, true);
#pragma unroll
    for (int g = 0; g < 4; ++g) Pi[(int64_t)(r0 + l4 + 4 * g) * ld + c0 + l15] = acc[g];
  }
}

// X_e = inv(D_e) (F_e - L_e X_{e-s} - U_e X_{e+s}) for the eliminated block e; s == 0: the last
// block, no neighbours.  T = F_e - ... in LDS (B x 65 doubles, row stride kp + 1), then the product.
template <int B>
__device__ __forceinline__ void bw_back_panel_block(const double *__restrict__ Dinv,
                                                    const double *__restrict__ L,
                                                    const double *__restrict__ U, double *__restrict__ P,
                                                    int ld, int kp, int nb, int s, int e, double *T) {
  constexpr int BB = B * B;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l4 = lane >> 4, l15 = lane & 15;
  const int le = e - s, ri = e + s, ldt = kp + 1;
  const bool hl = s > 0 && le >= 0, hr = s > 0 && ri < nb;
  const int tc = kp / 16, nt = (B / 16) * tc;
  const int64_t be = (int64_t)e * BB;
  double *Pe = P + (int64_t)e * B * ld;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int tt = wave + 4 * t;
    if (tt >= nt) break;
    const int r0 = (tt / tc) * 16, c0 = (tt % tc) * 16;
    bw_double4 acc;
#pragma unroll
    for (int g = 0; g < 4; ++g) acc[g] = Pe[(int64_t)(r0 + l4 + 4 * g) * ld + c0 + l15];
    if (hl) acc = bw_tile<B>(L + be, B, P + (int64_t)le * B * ld, ld, r0, c0, acc, lane, true);
    if (hr) acc = bw_tile<B>(U + be, B, P + (int64_t)ri * B * ld, ld, r0, c0, acc, lane, true);
#pragma unroll
    for (int g = 0; g < 4; ++g) T[(r0 + l4 + 4 * g) * ldt + c0 + l15] = acc[g];
  }
  __syncthreads();  // T complete (every tile of X_e reads all its rows)
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int tt = wave + 4 * t;
    if (tt >= nt) break;
    const int r0 = (tt / tc) * 16, c0 = (tt % tc) * 16;
    bw_double4 acc = {0.0, 0.0, 0.0, 0.0};
    acc = bw_tile<B>(Dinv + be, B, T, ldt, r0, c0, acc, lane, false);
#pragma unroll
    for (int g = 0; g < 4; ++g) Pe[(int64_t)(r0 + l4 + 4 * g) * ld + c0 + l15] = acc[g];
  }
}

// Accuracy guard for bw <= 64: the same (max |r|, max (|K| |x| + |rhs0|)) pair per 256 rows as
// k_band_residual (pgf_sparse.hip), which stages its rows in LDS for bw <= 10; here a row reads
// its band entries straight from memory (up to 2 x 65 of them, L2-resident neighbours).
// blk: which 256 rows; pr, pb: 4 doubles of LDS each.
__device__ __forceinline__ void bw_residual_rows(const double *__restrict__ band, int ldb, int bw, int N,
                                                 const double *__restrict__ x,
                                                 const double *__restrict__ rhs0, double *__restrict__ r,
                                                 double *__restrict__ rsmax, const int *__restrict__ flags,
                                                 int nred, int blk, double *pr, double *pb) {
  if (blk == 0 && threadIdx.x < 4) rsmax[3 * nred + threadIdx.x] = (double)flags[threadIdx.x];
  const int i = blk * 256 + threadIdx.x;
  double ar = 0.0, ab = 0.0;
  if (i < N) {
    double acc = rhs0[i];
    ab = fabs(acc);
    const double *row = band + (int64_t)i * ldb;
    for (int d = 0; d <= bw && d <= i; ++d) {
      const double kx = row[d] * x[i - d];
      acc = fma(-row[d], x[i - d], acc);
      ab += fabs(kx);
    }
    for (int d = 1; d <= bw && i + d < N; ++d) {
      const double kv = band[(int64_t)(i + d) * ldb + d];
      acc = fma(-kv, x[i + d], acc);
      ab += fabs(kv * x[i + d]);
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
  if (threadIdx.x == 0) {
    rsmax[2 * blk] = fmax(fmax(pr[0], pr[1]), fmax(pr[2], pr[3]));
    rsmax[2 * blk + 1] = fmax(fmax(pb[0], pb[1]), fmax(pb[2], pb[3]));
  }
}
