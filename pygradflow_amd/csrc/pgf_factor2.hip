// Look-ahead schedule of the dense LDL^T factorisation of the reduced KKT matrix (replaces
// SuperLU gstrf reached through scipy.sparse.linalg.splu at reference
// pygradflow/linear_solver/lu_solver.py:14): unpivoted right-looking LDL^T in the natural order,
// inertia = number of negative pivots; handle and solves in pgf_ldlt.hip.  Per outer block k of
// LDLT_OB = 256 columns:
//
//   k_update_diag  (k-1 -> k)   the 256 x 256 DIAGONAL block of block k receives block k-1's
//                               update first (36 tiles of 32 x 32, one workgroup each)
//   k_chain_update              ONE launch with three kinds of workgroups:
//     workgroup 0     D(k)      the chain: 16 wavefronts factorise that diagonal block -- four
//                               64-column sub-panels; per sub-panel the 64 x 64 tile is
//                               eliminated by wavefront 0 (every row of 16 lanes holds the 16 x 16
//                               pivot tile, multipliers as DPP row broadcasts),
//                               the block's rows below ride one 16-column step behind on
//                               wavefronts 1-3, MFMA updates on all 16.  This is the
//                               factorisation's critical chain of N sequential pivots -- and
//                               nothing else is.
//     workgroups 8, 16          its helpers on the same XCD (stamps in global memory): the part
//                               of the in-block update the chain does not need for its next
//                               sub-panel, and the inverses of the unit-lower diagonal tiles
//                               (the solves and k_trsm_block multiply with them)
//     all others                one 128 x 128 tile each of trailing-update work from the lazy
//                               plan (plan_updates): column blocks are kept complete only when
//                               the chain is about to need them, the rest on a budget that
//                               hides behind the chain; W = L D formed from L and D on the fly
//   k_chain_head                the FIRST chain's launch of a dense Newton step: the same roles, the
//                               other workgroups write the part of K and of the panel V that D(0)
//                               does not read (LdltHead) instead of update tiles
//   k_trsm_block   T(k)         all rows below the block: X = T inv(L_kk)^T blocked by 64
//                               (MFMA, B operands straight from L2 into registers); writes
//                               W = X = L D (operand of k_update_diag) and L = X D^-1.
//
// The chain and the update tiles touch disjoint cache lines and hand nothing to each other, so
// the launch is correct whatever order its workgroups run in: look-ahead inside one queue,
// without a second stream (hipExtAnyOrderLaunch starts kernels early but does not run them
// side by side on this stack).  The round-1 schedule ran 80 panel launches of 22-33 us one
// after the other with the bulk updates between them (2.3 ms of 4.0 ms per step at N = 5120);
// here the serial part is D(k), ~66 us per 256 columns, and the update hides behind it.
// Batched mode (kb_*): the same chain / T(k) / update-diag device code with a batch dimension.
// The device code of D(k) and its helpers: pgf_chain_dev.h; the lazy plan and the tile numbering
// of its job tables: pgf_update_plan.h, pgf_update_plan.hip (host only).
#include <hip/hip_ext.h>

#include "pgf_batch.h"
#include "pgf_chain_dev.h"
#include "pgf_env.h"
#include "pgf_head_dev.h"
#include "pgf_kernels.h"
#include "pgf_ldlt.h"
#include "pgf_ldlt_dev.h"
#include "pgf_update_plan.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

// ------------------------------------------------------------------ TS x TS tile product
// One 16 x 16 MFMA tile per wavefront of a (TS / 16)^2-wavefront workgroup:
//   acc -= sum_{k < kd} A[i0 + i][k] * B[j0 + j][k]
// A and B are row-major in global memory (k contiguous, first column already applied to the
// pointers), staged through LDS in 64-deep chunks with the next chunk's loads in flight behind
// the current chunk's MFMAs.  v_mfma_f64_16x16x4_f64 operand layout: A: lane l holds
// A[l & 15][l >> 4], B: B[l >> 4][l & 15], C/D: row (l >> 4) + 4 reg, col l & 15.
template <int TS>
__device__ __forceinline__ void tile_msub(double4_t &acc, double (*As)[C_LD], double (*Bs)[C_LD],
                                          const double *A, int64_t lda, int i0, int ilim,
                                          const double *B, int64_t ldb, int j0, int jlim, int kd) {
  constexpr int WPR = TS / 16, NT = 64 * WPR * WPR, NQ = TS * 32 / NT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave / WPR, wc = wave % WPR, l15 = lane & 15, l4 = lane >> 4;
  double2_t va[NQ], vb[NQ];
  auto fetch = [&](int kk) {  // chunk [kk, kk + 64) -> registers
    const int kc = min(64, kd - kk);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int p = q * NT + tid;
      const int row = p >> 5, c2 = (p & 31) * 2;
      double2_t a = (double2_t){0.0, 0.0}, b = (double2_t){0.0, 0.0};
      if (i0 + row < ilim) {
        const double *src = A + (int64_t)(i0 + row) * lda + kk + c2;
        if (c2 + 1 < kc) a = *reinterpret_cast<const double2_t *>(src);
        else if (c2 < kc) a.x = *src;
      }
      if (j0 + row < jlim) {
        const double *src = B + (int64_t)(j0 + row) * ldb + kk + c2;
        if (c2 + 1 < kc) b = *reinterpret_cast<const double2_t *>(src);
        else if (c2 < kc) b.x = *src;
      }
      va[q] = a;
      vb[q] = b;
    }
  };
  if (kd > 0) fetch(0);
  for (int kk = 0; kk < kd; kk += 64) {
    const int kc = min(64, kd - kk);
    __syncthreads();  // the previous chunk's fragment reads are done
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int p = q * NT + tid;
      const int row = p >> 5, c2 = (p & 31) * 2;
      *reinterpret_cast<double2_t *>(&As[row][c2]) = -va[q];
      *reinterpret_cast<double2_t *>(&Bs[row][c2]) = vb[q];
    }
    __syncthreads();
    if (kk + 64 < kd) fetch(kk + 64);  // in flight during this chunk's MFMAs
    const int kr = (kc + 3) & ~3;
#pragma unroll 4
    for (int ks = 0; ks < kr; ks += 4) {
      const double a = As[16 * wr + l15][ks + l4];
      const double b = Bs[16 * wc + l15][ks + l4];
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
  }
}

// ------------------------------------------------------------------ U_diag
// Diagonal block of the NEXT outer block (rows / columns [c1, c1 + nb1)) -= W L^T of the
// current one (K-depth kd, L in columns [kc0, kc0 + kd) of K, W block-relative).  One
// workgroup per TS x TS tile of the lower triangle; TS = 32: 36 workgroups of 4 wavefronts
// (a tile is 2 TS^2 kd flops on ONE CU's matrix pipes: 6.8 us at TS = 64, 1.7 us at 32).
template <int TS>
__device__ __forceinline__ void update_diag_tile(unsigned char *smem, int t, double *K, int64_t ldk,
                                                 const double *W, int64_t ldw, int kc0, int kd,
                                                 int c1, int nb1) {
  constexpr int WPR = TS / 16;
  double(*As)[C_LD] = reinterpret_cast<double(*)[C_LD]>(smem);
  double(*Bs)[C_LD] = reinterpret_cast<double(*)[C_LD]>(smem + TS * C_LD * 8);
  int I = 0;
  while (t > I) {
    t -= I + 1;
    ++I;
  }
  const int J = t;  // J <= I
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wr = wave / WPR, wc = wave % WPR, l15 = lane & 15, l4 = lane >> 4;
  const int lim = c1 + nb1;
  const int i0 = c1 + TS * I, j0 = c1 + TS * J;
  double4_t acc;
  const int j = j0 + 16 * wc + l15;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + 16 * wr + l4 + 4 * r;
    acc[r] = (i < lim && j < lim && j <= i) ? K[(int64_t)i * ldk + j] : 0.0;
  }
  tile_msub<TS>(acc, As, Bs, W, ldw, i0, lim, K + kc0, ldk, j0, lim, kd);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + 16 * wr + l4 + 4 * r;
    if (i < lim && j < lim && j <= i) K[(int64_t)i * ldk + j] = acc[r];
  }
}

template <int TS>
__global__ __launch_bounds__(4 * TS * TS / 16) void k_update_diag(double *K, int64_t ldk,
                                                                  const double *W, int64_t ldw,
                                                                  int kc0, int kd, int c1, int nb1) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * TS * C_LD * 8];
  update_diag_tile<TS>(smem, (int)blockIdx.x, K, ldk, W, ldw, kc0, kd, c1, nb1);
}

// batched: the 36 tiles of every instance's next diagonal block (block [c1 - 256, c1) applied)
__global__ __launch_bounds__(256) void kb_update_diag(const BInst *__restrict__ tab, int B, int m,
                                                      int wbuf, int c1) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 32 * C_LD * 8];
  int inst, t;
  if (!batch_decode(B, 36, inst, t)) return;
  const BInst &I = tab[inst];
  if (I.ctl[0] == 0) return;
  const int N = I.counts[0] + m;
  if (c1 >= N) return;
  update_diag_tile<32>(smem, t, I.K, I.ldk, I.W + (int64_t)wbuf * I.wstride, 256, c1 - 256, 256, c1,
                       min(256, N - c1));
}

// ------------------------------------------------------------------ T(k)
// Rows below outer block [c0, c0 + nb): workgroup g owns the 16 rows r0 = c0 + nb + 16 g ...
// (row N, a carried right-hand side, included), wavefront wc the columns 16 wc ... of every
// 64-column sub-panel.  Per sub-panel s, left-looking:
//   T_s = K[rows, sub-panel s] - sum_{t < s} X_t L_st^T ;  X_s = T_s inv(L_ss)^T
//   W[rows, 64 s ..] = X_s (= L D) ;  K[rows, sub-panel s] = X_s D^-1 (= L)
// The workgroup's 16 x 256 strip starts in registers (one 16 x 16 accumulator per wavefront and
// sub-panel); the X_t it produces stay in LDS as the A operands of the later sub-panels.
// The B operands (L_10, inv_1, L_20, L_21, inv_2, ...: ten 64 x 64 tiles of the L2-resident
// diagonal block) are NOT staged through LDS: with 16 rows per workgroup every B element
// feeds exactly one wavefront, so each wavefront loads its own 16-row slice straight into MFMA
// operand registers, three tiles ahead of their use, and the six update steps need no barrier
// at all -- only the four solves exchange T_s / X_s through LDS.  (Staged through LDS with two
// barriers per tile the kernel took 20 us, 1.0-1.6 us per step against 0.5 us of MFMA work: one
// wavefront per SIMD has nothing to hide an LDS round trip behind.  Now 17-19 us: an update
// step takes 0.5-0.6 us when its B slice has arrived, but 300 workgroups pulling the same
// 320 KB each out of L2 -- ~100 MB per launch -- make the loads, not the MFMAs, the limit;
// in-kernel stamps: 3.5 us of cold strip loads, ~11 us of steps.)
// The k index of an MFMA step is free as long as A and B agree: step q of lane group l4 takes
// k = 8 (q / 2) + 2 l4 + (q & 1), so that both operands come as aligned 16-byte pairs.
// 16 rows per workgroup because the MFMA work of a workgroup runs on ONE CU's matrix pipes
// (0.3 TFLOP/s): 64 rows took 34 us.
// POST (k_trsm_ud): after the stores of sub-panel s have reached L2 the workgroup posts
// post[s] = postval -- the update of the next diagonal block runs in the same launch and takes
// the rows sub-panel by sub-panel.
// RT: 16-row tiles per workgroup.  1 where the launch is bound by the latency of one row group
// (single instance: ~250 row groups, one per CU); the batched launches -- thousands of row
// groups, three resident per CU, each pulling its own copy of the B slices through the CU's
// texture path -- take 2: every B register feeds two MFMAs (kb_trsm_block, 32 instances:
// 100 -> ... us).
template <bool POST = false, int RT = 1>
__device__ __forceinline__ void trsm_block_body(double (*Xs)[16 * RT][C_LD], double *ds, int wg, double *K,
                                                int64_t ldk, double *W, int64_t ldw, int nrows,
                                                int c0, int nb, const double *__restrict__ dinv,
                                                const double *__restrict__ Linv, int *post = nullptr,
                                                int postval = 0) {
  const int tid = threadIdx.x, lane = tid & 63, wc = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  const int bend = c0 + nb;
  const int r0 = bend + 16 * RT * wg;
  const int ns = (nb + 63) / 64;
  constexpr int DEPTH = 3;
  double2_t bq[DEPTH][8];
  auto fetch_b = [&](double2_t (&dst)[8], int idx) {
    // idx -> tile (s_, t_), s_ (s_ + 1) / 2 + t_ = idx; t_ < s_: L_st, t_ == s_: inv(L_ss)
    const int s_ = (idx >= 6) ? 3 : (idx >= 3) ? 2 : (idx >= 1) ? 1 : 0;
    const int t_ = idx - s_ * (s_ + 1) / 2;
    if (idx >= 10 || s_ >= ns) return;
    const int cb = c0 + 64 * s_;
    const int row = 16 * wc + l15;
    const bool ok = (t_ == s_) || row < min(64, bend - cb);
    const double *src = (t_ == s_) ? Linv + (size_t)(cb / 64) * 4096 + row * 64
                                   : K + (int64_t)(cb + row) * ldk + c0 + 64 * t_;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      dst[j] = ok ? *reinterpret_cast<const double2_t *>(src + 8 * j + 2 * l4) : (double2_t){0.0, 0.0};
  };
#pragma unroll
  for (int d = 0; d < DEPTH; ++d) fetch_b(bq[d], d);
  double4_t acc[RT][4];
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int j = c0 + 64 * s + 16 * wc + l15;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = r0 + 16 * rt + l4 + 4 * r;
        acc[rt][s][r] = (i < nrows && j < bend) ? K[(int64_t)i * ldk + j] : 0.0;
      }
    }
  ds[tid] = (tid < nb) ? dinv[c0 + tid] : 0.0;
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    if (s < ns) {
      const int cb = c0 + 64 * s;
      const int ncol = min(64, bend - cb);
#pragma unroll
      for (int t = 0; t < s; ++t) {
        const int idx = s * (s + 1) / 2 + t;  // compile-time after unrolling
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          double4_t a4 = acc[rt][s];
          double2_t av[8];
#pragma unroll
          for (int j = 0; j < 8; ++j)
            av[j] = *reinterpret_cast<const double2_t *>(&Xs[t][16 * rt + l15][8 * j + 2 * l4]);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            a4 = __builtin_amdgcn_mfma_f64_16x16x4f64(-av[j].x, bq[idx % DEPTH][j].x, a4, 0, 0, 0);
            a4 = __builtin_amdgcn_mfma_f64_16x16x4f64(-av[j].y, bq[idx % DEPTH][j].y, a4, 0, 0, 0);
          }
          acc[rt][s] = a4;
        }
        fetch_b(bq[idx % DEPTH], idx + DEPTH);  // the slot just emptied
      }
      {
        // X[i][j] = sum_k T[i][k] inv[j][k]: T_s goes through LDS (every wavefront needs the
        // whole 64-column row), X_s replaces it there
        const int idx = s * (s + 1) / 2 + s;
        double(*St)[C_LD] = Xs[s];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) St[16 * rt + l4 + 4 * r][16 * wc + l15] = acc[rt][s][r];
        __syncthreads();
        double4_t x[RT];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          x[rt] = (double4_t){0.0, 0.0, 0.0, 0.0};
          double2_t av[8];
#pragma unroll
          for (int j = 0; j < 8; ++j)
            av[j] = *reinterpret_cast<const double2_t *>(&St[16 * rt + l15][8 * j + 2 * l4]);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            x[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[j].x, bq[idx % DEPTH][j].x, x[rt], 0, 0, 0);
            x[rt] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[j].y, bq[idx % DEPTH][j].y, x[rt], 0, 0, 0);
          }
        }
        fetch_b(bq[idx % DEPTH], idx + DEPTH);
        __syncthreads();  // all reads of T done: X replaces it
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
          for (int r = 0; r < 4; ++r) St[16 * rt + l4 + 4 * r][16 * wc + l15] = x[rt][r];
        __syncthreads();
        for (int p = tid; p < 16 * RT * 32; p += 256) {
          const int row = p >> 5, c2 = (p & 31) * 2;
          const int r = r0 + row;
          if (r >= nrows || c2 >= ncol) continue;
          const double2_t w = *reinterpret_cast<const double2_t *>(&St[row][c2]);
          double2_t l;
          l.x = w.x * ds[64 * s + c2];
          l.y = w.y * ds[64 * s + c2 + 1];
          double *wp = W + (int64_t)r * ldw + 64 * s + c2;
          double *kp = K + (int64_t)r * ldk + cb + c2;
          if (c2 + 1 < ncol) {
            *reinterpret_cast<double2_t *>(wp) = w;
            *reinterpret_cast<double2_t *>(kp) = l;
          } else {
            wp[0] = w.x;
            kp[0] = l.x;
          }
        }
        if (POST) {
          // every thread's stores are in L2 (the L1 is write-through) before the stamp is
          asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
          __syncthreads();
          if (tid == 0) post[s] = postval;
        }
      }
    } else if (POST) {
      if (tid == 0) post[s] = postval;  // no such sub-panel (ragged last block): nothing to wait for
    }
  }
}

__global__ __launch_bounds__(256) void k_trsm_block(double *K, int64_t ldk, double *W, int64_t ldw,
                                                    int nrows, int c0, int nb,
                                                    const double *__restrict__ dinv,
                                                    const double *__restrict__ Linv) {
  __shared__ __attribute__((aligned(16))) double Xs[4][16][C_LD];
  __shared__ double ds[256];
  trsm_block_body(Xs, ds, (int)blockIdx.x, K, ldk, W, ldw, nrows, c0, nb, dinv, Linv);
}

// batched: instance = tab[..] (its own N, known on the device), workgroup wg of `per` (32 rows each)
#define KB_TRSM_RT 2
__global__ __launch_bounds__(256) void kb_trsm_block(const BInst *__restrict__ tab, int B, int per,
                                                     int m, int wbuf, int c0) {
  __shared__ __attribute__((aligned(16))) double Xs[4][16 * KB_TRSM_RT][C_LD];
  __shared__ double ds[256];
  int inst, wg;
  if (!batch_decode(B, per, inst, wg)) return;
  const BInst &I = tab[inst];
  if (I.ctl[0] == 0) return;
  const int N = I.counts[0] + m, nrows = N + 1;
  if (c0 >= N) return;
  const int nb = min(256, N - c0);
  if (c0 + nb + 16 * KB_TRSM_RT * wg >= nrows) return;
  trsm_block_body<false, KB_TRSM_RT>(Xs, ds, wg, I.K, I.ldk, I.W + (int64_t)wbuf * I.wstride, 256, nrows, c0,
                                     nb, I.dinv, I.Linv);
}

// ------------------------------------------------------------------ T(k) + U_diag in ONE launch
// k_update_diag (k -> k + 1) only needs the rows of the NEXT diagonal block from T(k): the (at
// most) 16 row groups right below block k.  As its own launch it cost 7.9 us per outer block on
// the factorisation's critical path.  Here those row groups and the 36 diagonal tiles are
// workgroups of one launch on ONE XCD (ids that are multiples of 8, checked through
// HW_REG_XCC_ID like the chain's helpers): a row group posts a stamp per 64-column sub-panel once
// the sub-panel's W / L entries are in that XCD's L2, a diagonal tile takes its K-depth-256
// product sub-panel by sub-panel behind the stamps of the four row groups it reads (operands
// with L1-bypassing loads) and is done about 2 us after the last one -- inside the time the
// other ~290 row groups of T(k) take anyway.  Workgroups only wait for workgroups with smaller
// ids; polls are bounded; a failed placement check or a timed-out wait sets flags[2] and the
// host repeats the factorisation with separate launches (as for the chain's helpers).
#define TUD_BASE 32  // hctl words [32, 96): stamp of (row group g < 16, sub-panel s < 4) at 4 g + s

// wait until the four row groups (g0, g0 + 1, g1, g1 + 1) have posted sub-panel s
__device__ __forceinline__ void tud_wait(const int *st, int g0, int g1, int s, int val, int ngroups,
                                         int *flags) {
  const int lane = threadIdx.x & 63;
  int g = (lane < 2) ? g0 + lane : g1 + (lane - 2);
  const bool mine = lane < 4 && g < ngroups;
  for (int it = 0; it < HELP_SPIN_LIMIT; ++it) {
    int v = val;
    if (mine) v = __hip_atomic_load(st + 4 * g + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool same_epoch = (v >> 4) == (val >> 4);
    if (!__builtin_amdgcn_ballot_w64(!same_epoch)) {
      if (__builtin_amdgcn_ballot_w64(v != val)) atomicOr(&flags[2], 1);  // another XCD
      return;
    }
    __builtin_amdgcn_s_sleep(1);
  }
  atomicOr(&flags[2], 2);
}

// update_diag_tile<32> behind the stamps: chunk kk = sub-panel kk / 64
__device__ __forceinline__ void update_diag_tile_live(unsigned char *smem, int t, double *K, int64_t ldk,
                                                      const double *W, int64_t ldw, int kc0, int kd,
                                                      int c1, int nb1, const int *st, int val,
                                                      int ngroups, int *flags) {
  constexpr int TS = 32, WPR = 2, NT = 256, NQ = 4;
  double(*As)[C_LD] = reinterpret_cast<double(*)[C_LD]>(smem);
  double(*Bs)[C_LD] = reinterpret_cast<double(*)[C_LD]>(smem + TS * C_LD * 8);
  int I = 0;
  while (t > I) {
    t -= I + 1;
    ++I;
  }
  const int J = t;  // J <= I
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave / WPR, wc = wave % WPR, l15 = lane & 15, l4 = lane >> 4;
  const int lim = c1 + nb1;
  const int i0 = c1 + TS * I, j0 = c1 + TS * J;
  double4_t acc;
  const int j = j0 + 16 * wc + l15;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + 16 * wr + l4 + 4 * r;
    acc[r] = (i < lim && j < lim && j <= i) ? K[(int64_t)i * ldk + j] : 0.0;
  }
  const double *B = K + kc0;
  for (int kk = 0; kk < kd; kk += 64) {
    const int kc = min(64, kd - kk);
    tud_wait(st, 2 * I, 2 * J, kk >> 6, val, ngroups, flags);
    double2_t va[NQ], vb[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int p = q * NT + tid;
      const int row = p >> 5, c2 = (p & 31) * 2;
      double2_t a = (double2_t){0.0, 0.0}, b = (double2_t){0.0, 0.0};
      if (i0 + row < lim) {
        const double *src = W + (int64_t)(i0 + row) * ldw + kk + c2;
        if (c2 < kc) a.x = ld_agent(src);
        if (c2 + 1 < kc) a.y = ld_agent(src + 1);
      }
      if (j0 + row < lim) {
        const double *src = B + (int64_t)(j0 + row) * ldk + kk + c2;
        if (c2 < kc) b.x = ld_agent(src);
        if (c2 + 1 < kc) b.y = ld_agent(src + 1);
      }
      va[q] = a;
      vb[q] = b;
    }
    __syncthreads();  // the previous chunk's fragment reads are done
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int p = q * NT + tid;
      const int row = p >> 5, c2 = (p & 31) * 2;
      *reinterpret_cast<double2_t *>(&As[row][c2]) = -va[q];
      *reinterpret_cast<double2_t *>(&Bs[row][c2]) = vb[q];
    }
    __syncthreads();
    const int kr = (kc + 3) & ~3;
#pragma unroll 4
    for (int ks = 0; ks < kr; ks += 4) {
      const double a = As[16 * wr + l15][ks + l4];
      const double b = Bs[16 * wc + l15][ks + l4];
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + 16 * wr + l4 + 4 * r;
    if (i < lim && j < lim && j <= i) K[(int64_t)i * ldk + j] = acc[r];
  }
}

// grid: tud_grid() workgroups.  nA = row groups of the next diagonal block, nU = its tiles,
// S = nA + nU special workgroups at the ids 8 q; every other id takes one of the other row groups.
__global__ __launch_bounds__(256) void k_trsm_ud(double *K, int64_t ldk, double *W, int64_t ldw,
                                                 int nrows, int c0, int nb,
                                                 const double *__restrict__ dinv,
                                                 const double *__restrict__ Linv, int N, int *hctl,
                                                 int epoch, int *flags) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * 16 * C_LD * 8 + 256 * 8];
  double(*Xs)[16][C_LD] = reinterpret_cast<double(*)[16][C_LD]>(smem);
  double *ds = reinterpret_cast<double *>(smem + 4 * 16 * C_LD * 8);
  const int c1 = c0 + nb, nb1 = min(256, N - c1);
  const int nT = (nrows - c1 + 15) / 16;
  const int nA = min(nT, (nb1 + 15) / 16);
  const int nt = (nb1 + 31) / 32, nU = nt * (nt + 1) / 2;
  const int S = nA + nU;
  const int id = (int)blockIdx.x;
  int *st = hctl + TUD_BASE;
  const int val = ((epoch & 0x7ffffff) << 4) | (int)(__builtin_amdgcn_s_getreg(6164) & 15);
  if (id < 8 * S && (id & 7) == 0) {
    const int q = id >> 3;
    if (q < nA) {
      trsm_block_body<true>(Xs, ds, q, K, ldk, W, ldw, nrows, c0, nb, dinv, Linv, st + 4 * q, val);
    } else {
      update_diag_tile_live(smem, q - nA, K, ldk, W, ldw, c0, nb, c1, nb1, st, val, nA, flags);
    }
    return;
  }
  const int r = id < 8 * S ? id - (id >> 3) - 1 : id - S;
  if (nA + r >= nT) return;
  trsm_block_body<false>(Xs, ds, nA + r, K, ldk, W, ldw, nrows, c0, nb, dinv, Linv);
}

// workgroup 0: the chain; with HELP (grid of 17) workgroups 8 and 16 are its helpers, the
// others leave at once
template <bool HELP>
__global__ __launch_bounds__(64 * CH_WAVES) void k_diag_chain(double *K, int64_t ldk, int c0, int nb,
                                                           double *__restrict__ dvec,
                                                           double *__restrict__ dinv,
                                                           int *__restrict__ flags,
                                                           double *__restrict__ Linv,
                                                           double *__restrict__ LinvT,
                                                           long long *__restrict__ dbg, int *hc,
                                                           int epoch, int tail) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[CH_SMEM];
  if (blockIdx.x == 0) {
    chain_body<HELP>(smem, K, ldk, c0, nb, dvec, dinv, flags, Linv, LinvT, dbg, hc, epoch, tail);
  } else if (HELP && blockIdx.x == 8) {
    helper_tiles(smem, K, ldk, c0, nb, dvec, hc, epoch, flags);
  } else if (HELP && blockIdx.x == 16) {
    helper_inverses(smem, K, ldk, c0, nb, hc, epoch, flags, Linv, LinvT, tail, dbg);
  }
}

// ------------------------------------------------------------------ D(k + 1) beside update tiles
// ONE launch: workgroup 0 is the chain D(k + 1) of the next outer block (workgroups 8 and 16
// its helpers); every other workgroup applies pending blocks to one 128 x 128 tile of the
// trailing matrix below the next diagonal block, as the launch's job table says (update_tile of
// pgf_ldlt_dev.h with the A operand scaled by D while it is staged).  The two roles touch
// disjoint cache lines and hand nothing to each other, so the launch is correct whatever order
// the workgroups run in; dispatched first, the chain has its CU from the start.
// (The job table UpdJobs and the tile numbering upd_tile: pgf_update_plan.h.)

// tile t of a launch's job table.  ONE 128 x 128 tile per workgroup, 16 wavefronts as 4 x 4 with
// 2 x 2 MFMA tiles each and two LDS stages of K-depth 32: the chain's LDS footprint allows one
// workgroup per CU, so the 16 wavefronts share one staged panel pair.
__device__ __forceinline__ void update_job_tile(unsigned char *smem, int t, double *K, int64_t ldk,
                                                const double *__restrict__ dvec, int N, int nrows,
                                                const UpdJobs &jobs, const UpdVirt &uv) {
  // (past the end: upd_tile says so too, for the host's walk; left to it alone, the compiler
  // carries its answer as a value through the tile loop instead of branching on the comparison)
  if (t >= jobs.tile_begin[jobs.njobs]) return;
  int q, i0, j0;
  upd_tile(jobs, t, N, nrows, q, i0, j0);
  const int kc0 = jobs.kc0[q], KBr = jobs.KB[q], kc0v = jobs.kc0v[q], KBv = jobs.KBv[q];
  if (KBv > 0)
    update_tile<UPD_TM, 128, 32, 4, 4, 1, true>(smem, threadIdx.x, i0, j0, K, ldk, uv.V + kc0v, uv.ldv, N,
                                                nrows, N, kc0, KBv + KBr, uv.vd + kc0v, KBv, K + kc0, ldk,
                                                dvec + kc0);
  else
    update_tile<UPD_TM, 128, 32, 4, 4, 1, true>(smem, threadIdx.x, i0, j0, K, ldk, K + kc0, ldk, N, nrows, N,
                                                kc0, KBr, dvec + kc0);
}

// The update role, persistent: a workgroup takes tile after tile of the launch's job table from an
// atomic counter (zeroed with the factorisation's flags) until the table is exhausted -- deepest
// jobs first, so the long tiles start early and the short ones fill the gaps (round 2: one tile
// per workgroup; ~260 tiles over 253 CUs ran as two rounds, the second nearly empty).
__device__ __forceinline__ void update_worker(unsigned char *smem, double *K, int64_t ldk,
                                              const double *__restrict__ dvec, int N, int nrows,
                                              const UpdJobs &jobs, const UpdVirt &uv, int *ctr) {
  __shared__ int s_next;
  const int total = jobs.tile_begin[jobs.njobs];
  for (;;) {
    if (threadIdx.x == 0) s_next = atomicAdd(ctr, 1);
    __syncthreads();
    const int t = s_next;
    __syncthreads();  // (s_next is rewritten next round; the previous tile's LDS reads are done)
    if (t >= total) return;
    update_job_tile(smem, t, K, ldk, dvec, N, nrows, jobs, uv);
  }
}

template <bool HELP>
__global__ __launch_bounds__(1024) void k_chain_update(double *K, int64_t ldk, int c0, int nb,
                                                       double *__restrict__ dvec,
                                                       double *__restrict__ dinv,
                                                       int *__restrict__ flags,
                                                       double *__restrict__ Linv,
                                                       double *__restrict__ LinvT, int *hc,
                                                       int epoch, int N, int nrows,
                                                       const UpdJobs jobs, const UpdVirt uv, int *ctr,
                                                       int tail) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[CH_SMEM];
  const int b = (int)blockIdx.x;
  if (b == 0) {
    chain_body<HELP>(smem, K, ldk, c0, nb, dvec, dinv, flags, Linv, LinvT, nullptr, hc, epoch, tail);
    return;
  }
  if (HELP && b == 8) {
    helper_tiles(smem, K, ldk, c0, nb, dvec, hc, epoch, flags);
    return;
  }
  if (HELP && b == 16) {
    helper_inverses(smem, K, ldk, c0, nb, hc, epoch, flags, Linv, LinvT, tail);
    return;
  }
  update_worker(smem, K, ldk, dvec, N, nrows, jobs, uv, ctr);
}

// ------------------------------------------------------------------ D(0) beside the step's head
// The first chain's launch of a step (LdltHead, pgf_ldlt.h): the same grid and roles as
// k_chain_update, but the workgroups beside the chain and its helpers write what the step has
// not assembled yet -- K's rows below the first diagonal block and the panel V -- instead of
// update tiles: D(0) reads K[0:256, 0:256] alone, which the launch in front (k_assemble_kkt_head)
// has written.  Nobody waits for anybody: the roles write disjoint cache lines, and the first
// reader of the workers' entries is a later launch.  A kernel of its own: k_diag_chain and
// k_chain_update keep their code.
static_assert(ASM_ROWS == HEAD_ASM_ROWS, "head_unit's row groups are b_assemble_kkt's");
// Worker w of W: the four 256-lane quarters of the workgroup take units 4 w + q, 4 (w + W) + q, ...
// of head_unit's list, one each per round.  The panel's tiles go through the kernel's LDS buffer
// (two sets of four tiles, by the round's parity: ONE barrier per round keeps a tile's readers
// ahead of its next writers); every quarter runs every round, so all reach the barriers together.
__device__ __forceinline__ void head_worker(unsigned char *smem, double *K, int64_t ldk, const LdltHead &hw,
                                            int w, int W) {
  CondTile *tiles = reinterpret_cast<CondTile *>(smem);
  static_assert(8 * sizeof(CondTile) <= CH_SMEM, "two sets of four tiles");
  const int q = threadIdx.x >> 8, t = threadIdx.x & 255;
  const int N = hw.nI + hw.m, mp = hw.V ? hw.mp : 0;
  const int nasm = head_asm_units(N), total = nasm + head_panel_units(hw.nI, mp);
  const double ginv = 1.0 / hw.delta;
  int par = 0;
  for (int base = 4 * w; base < total; base += 4 * W, par ^= 4) {
    const HeadUnit hu = head_unit(base + q < total ? base + q : -1, N, hw.nI, mp);
    if (hu.kind == 0) {
      if (hw.G)
        b_assemble_kkt<ASM_ROWS, true>(hu.a, hu.b, t, K, ldk, hw.H, hw.ldh, hw.J, hw.ldj, hw.idxI, hw.nI, hw.m,
                                       hw.lamb, hw.delta, hw.G, hw.ldg, ginv);
      else
        b_assemble_kkt<ASM_ROWS, false>(hu.a, hu.b, t, K, ldk, hw.H, hw.ldh, hw.J, hw.ldj, hw.idxI, hw.nI, hw.m,
                                        hw.lamb, hw.delta);
    }
    if (base + 3 < nasm) continue;  // (the whole workgroup: a round without a tile needs no barrier)
    if (hu.kind == 1)
      b_cond_panel_load(tiles[par + q], hu.a, hu.b, t, hw.V, hw.ldv, mp, hw.J, hw.ldj, hw.idxI, hw.nI, hw.pm,
                        hw.vd, hw.rhs_y, hw.delta);
    __syncthreads();
    if (hu.kind == 1) b_cond_panel_store(tiles[par + q], hu.a, hu.b, t, hw.V, hw.ldv, mp, hw.nI);
  }
}

template <bool HELP>
__global__ __launch_bounds__(1024) void k_chain_head(double *K, int64_t ldk, int nb,
                                                     double *__restrict__ dvec,
                                                     double *__restrict__ dinv,
                                                     int *__restrict__ flags,
                                                     double *__restrict__ Linv,
                                                     double *__restrict__ LinvT,
                                                     long long *__restrict__ dbg, int *hc, int epoch,
                                                     const LdltHead hw, int tail) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[CH_SMEM];
  const int b = (int)blockIdx.x;
  if (b == 0) {
    chain_body<HELP>(smem, K, ldk, 0, nb, dvec, dinv, flags, Linv, LinvT, dbg, hc, epoch, tail);
    return;
  }
  if (HELP && b == 8) {
    helper_tiles(smem, K, ldk, 0, nb, dvec, hc, epoch, flags);
    return;
  }
  if (HELP && b == 16) {
    helper_inverses(smem, K, ldk, 0, nb, hc, epoch, flags, Linv, LinvT, tail, dbg);
    return;
  }
  if (HELP)
    head_worker(smem, K, ldk, hw, b - 1 - (b > 8) - (b > 16), (int)gridDim.x - 3);
  else
    head_worker(smem, K, ldk, hw, b - 1, (int)gridDim.x - 1);
}

// the update role alone (per-kernel profiling, PGF_FUSED=0): same tiles, same job table
__global__ __launch_bounds__(1024) void k_update_jobs(double *K, int64_t ldk,
                                                      const double *__restrict__ dvec, int N,
                                                      int nrows, const UpdJobs jobs, const UpdVirt uv,
                                                      int *ctr) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * 256 * 34 * 8];
  update_worker(smem, K, ldk, dvec, N, nrows, jobs, uv, ctr);
}

// The pre-eliminated block's update of ONE diagonal block, C -= V diag(vd) V^T on rows and columns
// [c0, c0 + nb): the only piece of it the first chain waits for.  Latency, not throughput (a
// 128 x 128 job tile of depth 1024 would take ~85 us): one 16 x 16 tile of the lower triangle per
// workgroup, its four wavefronts taking the 16-column chunks of the depth in turn (c = w, w + 4,
// ...; two chunks in flight per wavefront: the operands come straight from L2, ~1 us per dependent
// round trip) and summed through LDS in a fixed order.  Lane (l15, l4) reads four consecutive
// doubles of its row per chunk and feeds component t to MFMA t: the sum over k does not care
// which lane group carries which k as long as A and B agree.
__device__ __forceinline__ void virtual_diag_body(double (*part)[4][64], int t, double *K, int64_t ldk, int c0,
                                                  int nb, const double *__restrict__ V, int64_t ldv,
                                                  const double *__restrict__ vd, int depth, int vrows) {
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  const int tj = t - ti * (ti + 1) / 2;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, l4 = lane >> 4;
  const int i0 = 16 * ti, j0 = 16 * tj;
  const double *pa = V + (int64_t)min(c0 + i0 + l15, vrows - 1) * ldv + 4 * l4;
  const double *pb = V + (int64_t)min(c0 + j0 + l15, vrows - 1) * ldv + 4 * l4;
  const double *pd = vd + 4 * l4;
  double4_t acc = {0.0, 0.0, 0.0, 0.0};
  const int nc = depth / 16;
  for (int c = wave; c < nc; c += 8) {
    const int k0 = 16 * c;
    const bool two = c + 4 < nc;
    const int k1 = two ? k0 + 64 : k0;
    const double2_t a0 = *reinterpret_cast<const double2_t *>(pa + k0), a1 = *reinterpret_cast<const double2_t *>(pa + k0 + 2);
    const double2_t b0 = *reinterpret_cast<const double2_t *>(pb + k0), b1 = *reinterpret_cast<const double2_t *>(pb + k0 + 2);
    const double2_t d0 = *reinterpret_cast<const double2_t *>(pd + k0), d1 = *reinterpret_cast<const double2_t *>(pd + k0 + 2);
    const double2_t e0 = *reinterpret_cast<const double2_t *>(pa + k1), e1 = *reinterpret_cast<const double2_t *>(pa + k1 + 2);
    const double2_t f0 = *reinterpret_cast<const double2_t *>(pb + k1), f1 = *reinterpret_cast<const double2_t *>(pb + k1 + 2);
    const double2_t g0 = *reinterpret_cast<const double2_t *>(pd + k1), g1 = *reinterpret_cast<const double2_t *>(pd + k1 + 2);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a0[0] * d0[0], b0[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a0[1] * d0[1], b0[1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a1[0] * d1[0], b1[0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a1[1] * d1[1], b1[1], acc, 0, 0, 0);
    if (two) {
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-e0[0] * g0[0], f0[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-e0[1] * g0[1], f0[1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-e1[0] * g1[0], f1[0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-e1[1] * g1[1], f1[1], acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) part[wave][r][lane] = acc[r];
  __syncthreads();
  if (wave != 0) return;
  const int j = j0 + l15;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + l4 + 4 * r;
    if (i < nb && j <= i) {
      double *p = K + (int64_t)(c0 + i) * ldk + c0 + j;
      *p = *p + (((part[0][r][lane] + part[1][r][lane]) + part[2][r][lane]) + part[3][r][lane]);
    }
  }
}
__global__ __launch_bounds__(256) void k_virtual_diag(double *K, int64_t ldk, int c0, int nb,
                                                      const double *__restrict__ V, int64_t ldv,
                                                      const double *__restrict__ vd, int depth, int vrows) {
  __shared__ double part[4][4][64];
  virtual_diag_body(part, (int)blockIdx.x, K, ldk, c0, nb, V, ldv, vd, depth, vrows);
}
// batched: the first diagonal block of every instance that factorises (blockIdx.z = instance).
// Throughput, not the latency of one tile: a wavefront takes one 16 x 16 tile over the whole
// depth, four chunks (64 columns) in flight -- 34 workgroups per instance, all of a small batch
// resident at once (the split-depth version above: 4352 workgroups for 32 instances, 42 us).
__global__ __launch_bounds__(256) void kb_virtual_diag(const BInst *__restrict__ tab, int depth) {
  const BInst &I = tab[blockIdx.z];
  if (I.ctl[0] == 0) return;
  const int N = I.counts[0];
  if (N <= 0) return;
  const int nb = min(256, N), nt = (nb + 15) / 16;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, l4 = lane >> 4;
  const int t = 4 * (int)blockIdx.x + wave;
  if (t >= nt * (nt + 1) / 2) return;
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
  const int tj = t - ti * (ti + 1) / 2;
  const int i0 = 16 * ti, j0 = 16 * tj;
  const double *pa = I.V + (int64_t)min(i0 + l15, N) * I.ldv + 4 * l4;
  const double *pb = I.V + (int64_t)min(j0 + l15, N) * I.ldv + 4 * l4;
  const double *pd = I.vd + 4 * l4;
  double4_t acc;
  const int j = j0 + l15;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + l4 + 4 * r;
    acc[r] = (i < nb && j <= i) ? I.K[(int64_t)i * I.ldk + j] : 0.0;
  }
  for (int k0 = 0; k0 < depth; k0 += 64) {
    double2_t a[4][2], b[4][2], d[4][2];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = min(k0 + 16 * c, depth - 16);  // (a clamped chunk is skipped below)
      a[c][0] = *reinterpret_cast<const double2_t *>(pa + k);
      a[c][1] = *reinterpret_cast<const double2_t *>(pa + k + 2);
      b[c][0] = *reinterpret_cast<const double2_t *>(pb + k);
      b[c][1] = *reinterpret_cast<const double2_t *>(pb + k + 2);
      d[c][0] = *reinterpret_cast<const double2_t *>(pd + k);
      d[c][1] = *reinterpret_cast<const double2_t *>(pd + k + 2);
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (k0 + 16 * c >= depth) break;
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[c][0][0] * d[c][0][0], b[c][0][0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[c][0][1] * d[c][0][1], b[c][0][1], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[c][1][0] * d[c][1][0], b[c][1][0], acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-a[c][1][1] * d[c][1][1], b[c][1][1], acc, 0, 0, 0);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int i = i0 + l4 + 4 * r;
    if (i < nb && j <= i) I.K[(int64_t)i * I.ldk + j] = acc[r];
  }
}

// ------------------------------------------------------------------ batched wrappers
// The same chain and T(k) kernels with a batch dimension: instance = workgroup (chain) or
// batch_decode (T); every instance has its own N on the device, workgroups beyond it return.
// The chain runs WITHOUT helper workgroups here: with hundreds of instances there is one
// chain per CU and a spinning helper could wait for a CU its own chain occupies.
template <bool HELP>
__global__ __launch_bounds__(1024) void kb_diag_chain(const BInst *__restrict__ tab, int B, int Bp, int m,
                                                      int c0, int epoch, int tail) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[CH_SMEM];
  // roles: [0, Bp) chains, [Bp, 2 Bp) helpers T, [2 Bp, 3 Bp) helpers I; Bp = B rounded up to 8,
  // so that the three workgroups of an instance land on one XCD (ids equal modulo 8)
  const int id = (int)blockIdx.x, role = id / Bp, inst = id - role * Bp;
  if (inst >= B) return;
  const BInst &I = tab[inst];
  if (I.ctl[0] == 0) return;
  const int N = I.counts[0] + m;
  if (c0 >= N) return;
  const int nb = min(256, N - c0);
  if (role == 0)
    chain_body<HELP>(smem, I.K, I.ldk, c0, nb, I.dvec, I.dinv, I.flags, I.Linv, I.LinvT, nullptr,
                     I.hctl, epoch, tail);
  else if (HELP && role == 1)
    helper_tiles(smem, I.K, I.ldk, c0, nb, I.dvec, I.hctl, epoch, I.flags);
  else if (HELP && role == 2)
    helper_inverses(smem, I.K, I.ldk, c0, nb, I.hctl, epoch, I.flags, I.Linv, I.LinvT, tail);
}

// chains of the outer block at c1 beside the previous block's trailing update (everything below
// the diagonal block at c1), all instances in ONE launch: workgroups [0, Bp) are the chains
// (Bp = B rounded up to 8, so that the tiles behind them keep the instance -> XCD pinning),
// the rest one 128 x 128 update tile each.  Small batches only: with a chain per CU the tiles
// would queue behind them.
template <bool HELP>
__global__ __launch_bounds__(1024) void kb_chain_update(const BInst *__restrict__ tab, int B, int Bp,
                                                        int per, int m, int wbuf, int c1, int epoch,
                                                        int vdepth, int tail) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[CH_SMEM];
  const int id = (int)blockIdx.x;
  constexpr int NR = HELP ? 3 : 1;  // roles of the chain: chain, helper T, helper I
  if (id < NR * Bp) {
    const int role = id / Bp, ci = id - role * Bp;
    if (ci >= B) return;
    const BInst &I = tab[ci];
    if (I.ctl[0] == 0) return;
    const int N = I.counts[0] + m;
    if (c1 >= N) return;
    const int nb = min(256, N - c1);
    if (role == 0)
      chain_body<HELP>(smem, I.K, I.ldk, c1, nb, I.dvec, I.dinv, I.flags, I.Linv, I.LinvT, nullptr,
                       I.hctl, epoch, tail);
    else if (role == 1)
      helper_tiles(smem, I.K, I.ldk, c1, nb, I.dvec, I.hctl, epoch, I.flags);
    else
      helper_inverses(smem, I.K, I.ldk, c1, nb, I.hctl, epoch, I.flags, I.Linv, I.LinvT, tail);
    return;
  }
  int inst, t;
  if (!batch_decode_id(id - NR * Bp, B, per, inst, t)) return;
  const BInst &I = tab[inst];
  if (I.ctl[0] == 0) return;
  const int N = I.counts[0] + m, nrows = N + 1;
  if (c1 >= N) return;
  const int row0 = c1 + min(256, N - c1);
  if (row0 >= nrows) return;
  const int tr = (nrows - row0 + 127) / 128, tc = (N - c1 + 127) / 128;
  int by = 0;
  while (by < tr) {
    const int nc = min(tc, (row0 + 128 * by + 127 - c1) / 128 + 1);
    if (t < nc) break;
    t -= nc;
    ++by;
  }
  if (by >= tr) return;
  if (vdepth > 0)
    // c1 = 0, condensed order: the "previous block" is the pre-eliminated constraint block -- its
    // panel V with the scaling -1 / delta, everything but the first diagonal block (kb_virtual_diag)
    update_tile<128, 128, 32, 4, 4, 1, true>(smem, threadIdx.x, row0 + 128 * by, c1 + 128 * t, I.K, I.ldk, I.V,
                                             I.ldv, N, nrows, N, 0, vdepth, I.vd);
  else
    update_tile<128, 128, 32, 4, 4, 1>(smem, threadIdx.x, row0 + 128 * by, c1 + 128 * t, I.K, I.ldk,
                                       I.W + (int64_t)wbuf * I.wstride, 256, N, nrows, N, c1 - 256, 256);
}

void ldlt_batch_launch_update_diag(hipStream_t s, const BInst *tab, int B, int m, int wbuf, int c1) {
  hipLaunchKernelGGL(kb_update_diag, dim3(batch_grid(B, 36)), dim3(256), 0, s, tab, B, m, wbuf, c1);
}
// per: tiles of the largest possible instance (Nmax) in this launch
// Epochs of the chain <-> helper stamps: ONE counter for the process, single-instance and
// batched launches alike.  A handle's stamp words outlive the launches that wrote them (handles
// are pooled and move in and out of batches): with a counter per handle or per mode an old
// stamp could equal a new launch's epoch and release a helper before its chain had produced
// anything (seen once in ~10 runs of the test suite as a wrong inertia in a batched test that
// followed single-instance tests on the same pooled handles).
static std::atomic<int> g_help_epoch{0};
static int next_help_epoch() {
  int e = ++g_help_epoch;
  if (e <= 0 || e == 0x7fffffff) {  // wrapped: start over (2^31 launches)
    g_help_epoch = 1;
    e = 1;
  }
  return e;
}
static bool chain_helpers();  // (below: PGF_CHAIN_HELP and the process-wide switch-off)
static int chain_tail();      // (below: PGF_CHAIN_TAIL)
// compute units of the current device, asked once per process (256 if it cannot be asked)
static int device_cus() {
  static const int ncu = []() {
    int dev = 0, n = 256;
    hipDeviceProp_t pr;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&pr, dev) == hipSuccess && pr.multiProcessorCount > 0)
      n = pr.multiProcessorCount;
    return n;
  }();
  return ncu;
}
void ldlt_batch_launch_chain_update(hipStream_t s, const BInst *tab, int B, int Nmax, int m, int wbuf,
                                    int c1, bool helpers, int vdepth) {
  const int nrows = Nmax + 1, row0 = std::min(c1 + 256, Nmax);
  int per = 0;
  if (row0 < nrows) {
    const int tr = (nrows - row0 + 127) / 128, tc = (Nmax - c1 + 127) / 128;
    for (int by = 0; by < tr; ++by) per += std::min(tc, (row0 + 128 * by + 127 - c1) / 128 + 1);
  }
  const int Bp = 8 * ((B + 7) / 8);
  const int tiles = per ? batch_grid(B, per) : 0;
  // The helper workgroups (two per instance, a CU each for the length of the chain) shorten the
  // chain from ~86 to ~70 us -- which only pays while the launch is bound by its chains: with more
  // than ~1.5 tiles per CU (a 128 x 128 x 256 tile: ~40 us) the update tiles are the longer role
  // and want those CUs (32 instances, N = 1280: the first two of four launches)
  const int ncu = device_cus();
  if (helpers && 2 * B * per > 3 * std::max(1, ncu - B)) helpers = false;
  if (helpers && chain_helpers())
    hipLaunchKernelGGL(kb_chain_update<true>, dim3(3 * Bp + tiles), dim3(1024), 0, s, tab, B, Bp,
                       std::max(per, 1), m, wbuf, c1, next_help_epoch(), vdepth, chain_tail());
  else
    hipLaunchKernelGGL(kb_chain_update<false>, dim3(Bp + tiles), dim3(1024), 0, s, tab, B, Bp,
                       std::max(per, 1), m, wbuf, c1, 0, vdepth, 0);
}
void ldlt_batch_launch_virtual_diag(hipStream_t s, const BInst *tab, int B, int vdepth) {
  hipLaunchKernelGGL(kb_virtual_diag, dim3(34, 1, B), dim3(256), 0, s, tab, vdepth);
}
void ldlt_batch_launch_chain(hipStream_t s, const BInst *tab, int B, int m, int c0, bool helpers) {
  const int Bp = 8 * ((B + 7) / 8);
  if (helpers && chain_helpers())
    hipLaunchKernelGGL(kb_diag_chain<true>, dim3(3 * Bp), dim3(1024), 0, s, tab, B, Bp, m, c0,
                       next_help_epoch(), chain_tail());
  else
    hipLaunchKernelGGL(kb_diag_chain<false>, dim3(Bp), dim3(1024), 0, s, tab, B, Bp, m, c0, 0, 0);
}
// per: 16-row groups of the largest possible instance below the block
void ldlt_batch_launch_trsm(hipStream_t s, const BInst *tab, int B, int per, int m, int wbuf, int c0) {
  const int wgs = (per + KB_TRSM_RT - 1) / KB_TRSM_RT;
  hipLaunchKernelGGL(kb_trsm_block, dim3(batch_grid(B, wgs)), dim3(256), 0, s, tab, B, wgs, m, wbuf, c0);
}

// ------------------------------------------------------------------ host schedule
// helper workgroups of the diagonal chain (PGF_CHAIN_HELP=0: the chain does everything itself);
// switched off for the process after a failed placement check or a timed-out hand-over
static bool g_help_off = false;
static bool g_fused_ud_off = false;
static bool chain_helpers() {
  static const bool on = env_on("PGF_CHAIN_HELP");
  return on && !g_help_off;
}
void ldlt_chain_helpers_off() {
  // (flags[2] does not say which of the in-launch hand-overs failed: both kinds go)
  g_help_off = true;
  g_fused_ud_off = true;
}
bool ldlt_chain_helpers_enabled() { return chain_helpers(); }
// the chain inverts its block's last full diagonal tile itself, straight from its LDS
// (PGF_CHAIN_TAIL=0: helper I does, behind the chain's last stamp)
static int chain_tail() {
  static const bool on = env_on("PGF_CHAIN_TAIL");
  return on ? 1 : 0;
}
void ldlt_chain_helpers_set(bool on) {
  g_help_off = !on;
  g_fused_ud_off = !on;
}

// test hook (pgf_debug_fail_next_helper): make the factorisation just enqueued look like one
// whose helpers failed their checks
__global__ void k_helper_inject(int *__restrict__ flags) { atomicOr(&flags[2], 1); }
void ldlt_inject_helper_failure(hipStream_t s, int *flags) {
  hipLaunchKernelGGL(k_helper_inject, dim3(1), dim3(1), 0, s, flags);
}

// T(k) and the next diagonal block's update in one launch (k_trsm_ud); PGF_FUSED_UD=0 or a failed
// placement check: two launches
static bool fused_ud() {
  static const bool on = env_on("PGF_FUSED_UD");
  return on && !g_fused_ud_off;
}

static bool fused() {
  static const bool on = env_on("PGF_FUSED");
  return on;
}

// the step's head beside the first chain (k_chain_head); PGF_HEAD_FUSED=0: the assembly and the
// panel as launches of their own in front of a plain first chain
static bool head_fused() {
  static const bool on = env_on("PGF_HEAD_FUSED");
  return on;
}
bool ldlt_head_wanted(const DenseLdlt &f, int N) {
  const bool per_kernel = f.prof && f.prof->enabled && f.prof->mode != 2;
  return head_fused() && fused() && !per_kernel && N > LDLT_OB && f.vdepth == 0;
}

// PGF_CHAIN_TIMING=k (diagnostic): the chain of outer block k - 1 of every factorisation (k = 1:
// the first block; later blocks only where the chain is a launch of its own, PGF_FUSED=0) stamps
// its phases into this buffer, helper I its own behind them (CH_DBG_CHAIN);
// ldlt_chain_timing_dump prints the last set
static long long *g_chain_dbg = nullptr;
static int chain_dbg_block() {
  static const int blk = []() {
    const char *v = getenv("PGF_CHAIN_TIMING");
    return v ? std::max(0, atoi(v) - 1) : -1;
  }();
  return blk;
}
static long long *chain_dbg_buffer() {
  if (chain_dbg_block() < 0) return nullptr;
  if (!g_chain_dbg) {
    if (hipMalloc((void **)&g_chain_dbg, CH_DBG_WORDS * sizeof(long long)) != hipSuccess) return nullptr;
    (void)hipMemset(g_chain_dbg, 0, CH_DBG_WORDS * sizeof(long long));
  }
  return g_chain_dbg;
}
void ldlt_chain_timing_dump() {
  if (!g_chain_dbg) return;
  long long h[CH_DBG_WORDS];
  if (hipMemcpy(h, g_chain_dbg, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess) return;
  if (!h[0]) return;  // (no stamped chain since the last dump)
  fprintf(stderr, "k_diag_chain phase stamps (us since kernel start):");
  for (int i = 1; i < CH_DBG_CHAIN && h[i]; ++i) fprintf(stderr, " %.2f", (double)(h[i] - h[0]) * 0.01);
  fprintf(stderr, "\nhelper I (released, tile in LDS, inverse stored) per sub-panel:");
  for (int i = CH_DBG_CHAIN; i < CH_DBG_WORDS; ++i)
    if (h[i]) fprintf(stderr, " %.2f", (double)(h[i] - h[0]) * 0.01);
    else fprintf(stderr, " -");
  fprintf(stderr, "\n");
  (void)hipMemset(g_chain_dbg, 0, sizeof(h));
}

hipError_t ldlt_factor_async(DenseLdlt &f, int N, int nrows, const LdltHead *head) {
  if (head && (!ldlt_head_wanted(f, N) || head->nI + head->m != N)) return hipErrorInvalidValue;
  f.N = N;
  f.factored = false;
  hipStream_t s = f.stream;
  // flags [0, 4) and the update launches' tile counters behind them
  hipError_t e = hipSuccess;
  // (with a head its first launch zeroes them, flags_zeroed or not)
  if (!f.flags_zeroed && !head) e = hipMemsetAsync(f.flags, 0, (4 + LDLT_UPD_COUNTERS) * sizeof(int), s);
  f.flags_zeroed = false;
  if (e != hipSuccess) return e;
  const int ncu = device_cus();
  PgfProfile *p = (f.prof && f.prof->enabled) ? f.prof : nullptr;
  if (p) {
    p->factor_spans.emplace_back(prof_event(p), prof_event(p));
    (void)hipEventRecord(p->factor_spans.back().first, s);
  }
  constexpr int OB = LDLT_OB;
  const int64_t ldw = OB;
  auto span_begin = [&](std::vector<std::pair<hipEvent_t, hipEvent_t>> &v) {
    if (!p) return;
    v.emplace_back(prof_event(p), prof_event(p));
    (void)hipEventRecord(v.back().first, s);
  };
  auto span_end = [&](std::vector<std::pair<hipEvent_t, hipEvent_t>> &v) {
    if (p) (void)hipEventRecord(v.back().second, s);
  };
  PgfProfile dummy;
  PgfProfile &pr = p ? *p : dummy;
  const bool help = chain_helpers();
  const int vdepth = f.vdepth;
  const UpdVirt uv{f.V, f.ldv, f.vd};
  auto launch_d = [&](int c0) {
    span_begin(pr.chain_spans);
    long long *dbg = (c0 == OB * chain_dbg_block()) ? chain_dbg_buffer() : nullptr;
    const int nb = std::min(OB, N - c0);
    const int ep = next_help_epoch();
    if (help)
      hipLaunchKernelGGL(k_diag_chain<true>, dim3(17), dim3(1024), 0, s, f.K, f.ldk, c0, nb, f.dvec,
                         f.dinv, f.flags, f.Linv, f.LinvT, dbg, f.hctl, ep, chain_tail());
    else
      hipLaunchKernelGGL(k_diag_chain<false>, dim3(1), dim3(1024), 0, s, f.K, f.ldk, c0, nb, f.dvec,
                         f.dinv, f.flags, f.Linv, f.LinvT, dbg, f.hctl, ep, chain_tail());
    span_end(pr.chain_spans);
  };
  // T(c0) -- with the update of the next diagonal block in the same launch (k_trsm_ud) unless
  // per-kernel events are wanted or there is no next block
  const bool prod = p && p->mode == 2;  // production launches, one span each
  const bool fud = fused_ud() && (!p || prod);
  auto launch_t = [&](int c0, double *Wb) {
    const int nb = std::min(OB, N - c0);
    const int below = nrows - (c0 + nb);
    if (below <= 0) return;
    if (fud && c0 + nb < N) {
      const int c1 = c0 + nb, nb1 = std::min(OB, N - c1);
      const int nT = (below + 15) / 16, nA = std::min(nT, (nb1 + 15) / 16);
      const int nt = (nb1 + 31) / 32, S = nA + nt * (nt + 1) / 2;
      const int rest = nT - nA;  // row groups at the ordinary ids
      const int last = rest > 0 ? (rest - 1 < 7 * S ? (rest - 1) + (rest - 1) / 7 + 1 : rest - 1 + S) : 0;
      const int grid = std::max(8 * (S - 1) + 1, last + 1);
      if (prod) span_begin(pr.trsmud_spans);
      hipLaunchKernelGGL(k_trsm_ud, dim3(grid), dim3(256), 0, s, f.K, f.ldk, Wb, ldw, nrows, c0, nb,
                         f.dinv, f.Linv, N, f.hctl, next_help_epoch(), f.flags);
      if (prod) span_end(pr.trsmud_spans);
      return;
    }
    span_begin(pr.trsm_spans);
    hipLaunchKernelGGL(k_trsm_block, dim3((below + 15) / 16), dim3(256), 0, s, f.K, f.ldk, Wb, ldw,
                       nrows, c0, nb, f.dinv, f.Linv);
    span_end(pr.trsm_spans);
  };
  // Lazy trailing update (production; the plan: pgf_update_plan.hip).  PGF_LAZY_BUDGET fixes the
  // budget (0 = no limit = the eager schedule: every launch applies its block everywhere).
  const bool lazy = fused() && (!p || prod);  // one launch for chain + update; else two, same jobs
  const int nblk = (N + OB - 1) / OB;
  static const UpdPlan no_plan{};  // (a single block without virtual ones: no update launch)
  const UpdPlan &plan = (nblk > 1 || vdepth > 0) ? update_plan_for(N, nrows, vdepth) : no_plan;
  // algorithmic work of a launch's update jobs: entries (i, j), j <= i, of every job's region, 2 KB
  // flops each; bytes: every such entry read and written once, the L rows of the region's rows
  // and of its columns once per job
  auto job_work = [&](const UpdJobs &js, double &fl, double &by) {
    fl = by = 0.0;
    for (int q = 0; q < js.njobs; ++q) {
      const int col0 = js.col0[q], colEnd = std::min(N, col0 + 128 * js.ntc[q]);
      const int rs = std::max(js.rowstart[q], col0);
      double cnt = 0.0;
      for (int i = rs; i < nrows; ++i) cnt += std::min(colEnd, i + 1) - col0;
      const double kd = js.KB[q] + js.KBv[q];
      fl += 2.0 * cnt * kd;
      by += 16.0 * cnt + 8.0 * kd * ((double)(nrows - rs) + (double)(colEnd - col0));
    }
  };
  // chain of column block [c1, c1 + nb1) beside the update jobs js, one launch
  auto launch_fused = [&](int c1, int nb1, const UpdJobs &js, int *ctr) {
    const int ntiles = js.tile_begin[js.njobs];
    const int ep = next_help_epoch();
    if (prod) {
      span_begin(pr.fused_spans);
      double fl, by;
      job_work(js, fl, by);
      p->fused_flops.push_back(fl);
      p->fused_bytes.push_back(by);
    }
    const int workers = std::min(ntiles, ncu - 3);  // one workgroup per CU: persistent tile loops
    if (help)
      hipLaunchKernelGGL(k_chain_update<true>, dim3(std::max(17, workers + 3)), dim3(1024), 0, s, f.K, f.ldk,
                         c1, nb1, f.dvec, f.dinv, f.flags, f.Linv, f.LinvT, f.hctl, ep, N, nrows, js, uv, ctr,
                         chain_tail());
    else
      hipLaunchKernelGGL(k_chain_update<false>, dim3(1 + workers), dim3(1024), 0, s, f.K, f.ldk, c1, nb1,
                         f.dvec, f.dinv, f.flags, f.Linv, f.LinvT, f.hctl, ep, N, nrows, js, uv, ctr, 0);
    if (prod) span_end(pr.fused_spans);
  };
  // update jobs alone
  auto launch_jobs = [&](const UpdJobs &js, int *ctr) {
    const int ntiles = js.tile_begin[js.njobs];
    if (ntiles <= 0) return;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (p && !prod) {
      e0 = prof_event(p);
      e1 = prof_event(p);
      (void)hipEventRecord(e0, s);
    }
    hipLaunchKernelGGL(k_update_jobs, dim3(std::min(ntiles, ncu)), dim3(1024), 0, s, f.K, f.ldk, f.dvec, N,
                       nrows, js, uv, ctr);
    if (p && !prod) {
      (void)hipEventRecord(e1, s);
      p->update_spans.emplace_back(e0, e1);
      double fl, by;
      job_work(js, fl, by);
      p->update_flops.push_back(fl);
      p->update_bytes.push_back(by);
    }
  };
  int buf = 0;
  if (N > 0) {
    // a pre-eliminated block: its update of the first diagonal block first (nothing hides it), the
    // rest of column block 0, column block 1 -- and whatever the plan adds -- beside the first chain
    if (vdepth > 0) {
      const int nb0 = std::min(OB, N), nt = (nb0 + 15) / 16;
      hipLaunchKernelGGL(k_virtual_diag, dim3(nt * (nt + 1) / 2), dim3(256), 0, s, f.K, f.ldk, 0, nb0, f.V,
                         f.ldv, f.vd, vdepth, nrows);
    }
    if (head) {
      // the first diagonal block's rows and the zeroing, then D(0) with the rest of the head's
      // units on the other CUs; row nI of K needs the whole of V: a launch of its own behind them
      launch_assemble_kkt_head(s, f.K, f.ldk, *head, f.flags, 4 + LDLT_UPD_COUNTERS);
      const int units = head_asm_units(N) + head_panel_units(head->nI, head->V ? head->mp : 0);
      const int workers = std::min((units + 3) / 4, ncu - 3);
      const int ep = next_help_epoch();
      long long *head_dbg = chain_dbg_block() == 0 ? chain_dbg_buffer() : nullptr;
      span_begin(pr.chain_spans);
      if (help)
        hipLaunchKernelGGL(k_chain_head<true>, dim3(std::max(17, workers + 3)), dim3(1024), 0, s, f.K, f.ldk,
                           OB, f.dvec, f.dinv, f.flags, f.Linv, f.LinvT, head_dbg, f.hctl, ep, *head, chain_tail());
      else
        hipLaunchKernelGGL(k_chain_head<false>, dim3(1 + workers), dim3(1024), 0, s, f.K, f.ldk, OB, f.dvec,
                           f.dinv, f.flags, f.Linv, f.LinvT, head_dbg, f.hctl, ep, *head, 0);
      span_end(pr.chain_spans);
      if (head->crhs)
        launch_cond_rhs(s, head->nI, head->pm, head->V, head->ldv, head->crhs, head->delta, head->crhs_out);
    } else if (vdepth > 0 && lazy && plan.first.njobs > 0) {
      launch_fused(0, std::min(OB, N), plan.first, f.flags + 4);
    } else {
      launch_d(0);
      if (vdepth > 0) launch_jobs(plan.first, f.flags + 4);
    }
    launch_t(0, f.W);
  }
  for (int c0 = 0; c0 + OB < N; c0 += OB, buf ^= 1) {
    const int c1 = c0 + OB, nb1 = std::min(OB, N - c1);
    const double *Wb = f.W + (size_t)buf * f.wstride;
    const int nt = (nb1 + 31) / 32;
    if (!fud) {
      span_begin(pr.udiag_spans);
      hipLaunchKernelGGL(k_update_diag<32>, dim3(nt * (nt + 1) / 2), dim3(256), 0, s, f.K, f.ldk, Wb,
                         ldw, c0, OB, c1, nb1);
      span_end(pr.udiag_spans);
    }
    // D(k + 1) beside trailing-update work, in one launch; while profiling (per-kernel events)
    // and on request (PGF_FUSED=0) D(k + 1) and the whole of U(k) as two launches
    int *ctr = f.flags + 4 + ((c0 / OB + 1) % (LDLT_UPD_COUNTERS - 1));
    if (lazy) {
      launch_fused(c1, nb1, plan.launch[c0 / OB], ctr);
    } else {
      launch_d(c1);
      launch_jobs(plan.launch[c0 / OB], ctr);
    }
    launch_t(c1, f.W + (size_t)(buf ^ 1) * f.wstride);
  }
  if (p) (void)hipEventRecord(p->factor_spans.back().second, s);
  if (f.inject_helper_failure) {
    f.inject_helper_failure = 0;
    ldlt_inject_helper_failure(s, f.flags);
  }
  if (f.defer_status) {
    f.status_words |= 1;
  } else {
    e = hipMemcpyAsync(f.h_flags, f.flags, 4 * sizeof(int), hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return e;
  }
  return hipGetLastError();
}

// G <- V V^T, lower triangle (declared in pgf_ldlt.h): the update role alone (k_update_jobs)
// with one job over every 128-wide tile column, its K-range the panel V only (KB = 0: no column of
// G itself is read as an operand).  With vd = -1 the tile's C -= V diag(vd) V^T adds V V^T to the
// zeroed G.  n^2 depth flops once per derivative upload (pgf_api_factor.hip, gram_prepare).
hipError_t ldlt_gram_async(hipStream_t s, double *G, int64_t ldg, int n, const double *V, int64_t ldv,
                           const double *vd, int depth, int *ctr) {
  if (n <= 0 || depth <= 0 || depth % 32) return hipErrorInvalidValue;
  hipError_t e;
  if ((e = hipMemsetAsync(G, 0, (size_t)n * ldg * sizeof(double), s)) != hipSuccess) return e;
  if ((e = hipMemsetAsync(ctr, 0, sizeof(int), s)) != hipSuccess) return e;
  const int ncu = device_cus();
  UpdJobs js;
  memset(&js, 0, sizeof js);
  js.njobs = 1;
  js.col0[0] = 0;
  js.rowstart[0] = 0;
  js.kc0[0] = 0;
  js.KB[0] = 0;
  js.kc0v[0] = 0;
  js.KBv[0] = depth;
  js.ntc[0] = (n + 127) / 128;
  int ntiles = 0;  // as update_job_tile walks them: tile column c holds rows [128 c, n) in UPD_TM-row tiles
  for (int c = 0; c < js.ntc[0]; ++c) ntiles += (n - 128 * c + UPD_TM - 1) / UPD_TM;
  js.tile_begin[0] = 0;
  js.tile_begin[1] = ntiles;
  const UpdVirt uv{V, ldv, vd};
  // (dvec belongs to the K-range's second segment, which is empty here: G stands in, never read)
  hipLaunchKernelGGL(k_update_jobs, dim3(std::min(ntiles, ncu)), dim3(1024), 0, s, G, ldg, G, n, n, js, uv, ctr);
  return hipGetLastError();
}
