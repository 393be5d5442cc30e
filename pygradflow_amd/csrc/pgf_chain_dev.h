// Device code of the diagonal chain D(k) of the dense LDL^T look-ahead schedule and of its two
// helper workgroups: the DPP elimination of a 64-column sub-panel, the chain <-> helper stamp
// protocol, the inverses of the unit-lower diagonal tiles, and chain_body / helper_tiles /
// helper_inverses, the three roles a chain launch hands to workgroups.  Included by
// pgf_factor2.hip only, whose kernels wrap the roles; the schedule is described there.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgf_ldlt_dev.h"

#define C_LD 66    // LDS row stride of 64-column tiles: conflict-free MFMA fragment reads
#define C_WLD 18
#define CH_ROWS 256
#define CH_WAVES 16  // wavefronts of the chain workgroup (128 registers per lane, a few spilled)
// M[256][66] | Wt[2][64][18] | D[64] | 1/D[64] | flag (16 bytes) | 1/D of the sub-panel just
// factored [64]
#define CH_SMEM (CH_ROWS * C_LD * 8 + 2 * 64 * C_WLD * 8 + 3 * 64 * 8 + 16)

// ------------------------------------------------------------------ D(k)
// The elimination with DPP row broadcasts.  gfx950 has 64-bit DPP operands for
// row_newbcast ("DP ALU DPP"): v_fmac_f64_dpp acc, src row_newbcast:k, mult adds (lane k's src of
// the own row of 16 lanes) * mult -- ONE instruction per entry of a rank-1 update instead of two
// v_readlane + FMA, issued every 4 cycles (tools/chain_dpp_test.hip: a 16 x 16 tile in 0.83 us
// against 1.45, with 64 rows riding along 1.06 against 1.65).  Every row of 16 lanes therefore
// holds the whole pivot tile (lane r <-> pivot row r, all four rows of lanes the same), and each
// lane one more row that rides along: its row of the 64 x 64 diagonal tile (chain_a_plus) or of
// the rows below (chain_b_own).
template <int L>
__device__ __forceinline__ double dpp_bcast(double v) {
  return __builtin_amdgcn_update_dpp(0.0, v, 0x150 + L, 0xf, 0xf, false);
}
// acc += (lane L's src) * mult.  FRESH: two wait states first -- a DPP operand written by the
// instruction right before is read stale otherwise (inline assembly is invisible to the
// compiler's hazard recogniser).
template <int L, bool FRESH = false>
__device__ __forceinline__ void dpp_fmac(double &acc, double src, double mult) {
  if (FRESH)
    asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(acc)
                 : "v"(src), "v"(mult), "n"(L));
  else
    asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf"
                 : "+v"(acc)
                 : "v"(src), "v"(mult), "n"(L));
}

// column C of chain_a_plus: a[] = the lane's pivot row (entries <= row valid), b[] = its riding
// row; r = 1 / a[C] of the own lane (meaningful in lane C), npc = -a[C] * a[C + 1][C].  The
// riding row's L entry and W entry of column C go to LDS at once (mrow / wrow: byte addresses of
// M[row][cb] and Wt[row][0]): the stores drain beside the arithmetic.
// The serial chain of the whole factorisation runs through here: pivot -> reciprocal (seed + ONE
// Newton step: v_rcp_f64 delivers > 26 bits, the pivots only enter through products) -> the ONE
// entry the next pivot needs -> next pivot.  Written software-pipelined, with a scheduling
// barrier per column: left alone, the compiler's list scheduler turns the right-looking updates
// into a lazy (left-looking) order in which column j waits for a chain of j dependent FMAs right
// before its pivot.
template <int C>
__device__ __forceinline__ void chain_a_col(double (&a)[16], double (&b)[16], double &r, double &npc,
                                            double &dmine, int prow, double *mrow, double *wrow) {
  constexpr int C1 = (C + 1) & 15, C2 = (C + 2) & 15;
  double rn = 0.0, npn = 0.0;
  if (C + 1 < 16) {
    // the pivot chain: next pivot's column first, its reciprocal in flight behind the rest
    dpp_fmac<C, true>(a[C1], r, npc);
    rn = __builtin_amdgcn_rcp(a[C1]);
  }
  const double rb = dpp_bcast<C>(r);
  const double l = -a[C] * rb;   // -L[pivot row][C] (junk on and above the diagonal: never used)
  const double mr = -b[C] * rb;  // -L[riding row][C]
  if (C + 2 < 16) npn = -a[C1] * dpp_bcast<C2>(a[C1]);
  mrow[C] = -mr;
  wrow[C] = b[C];
#define CH_UA(K) \
  if (K > C + 1) dpp_fmac<K>(a[K], a[C], l);
  CH_UA(2) CH_UA(3) CH_UA(4) CH_UA(5) CH_UA(6) CH_UA(7) CH_UA(8) CH_UA(9) CH_UA(10) CH_UA(11)
  CH_UA(12) CH_UA(13) CH_UA(14) CH_UA(15)
#undef CH_UA
#define CH_UB(K) \
  if (K > C) dpp_fmac<K>(b[K], a[C], mr);
  CH_UB(1) CH_UB(2) CH_UB(3) CH_UB(4) CH_UB(5) CH_UB(6) CH_UB(7) CH_UB(8) CH_UB(9) CH_UB(10)
  CH_UB(11) CH_UB(12) CH_UB(13) CH_UB(14) CH_UB(15)
#undef CH_UB
  dmine = (prow == C) ? a[C] : dmine;
  if (C + 1 < 16) {
    rn = fma(rn, fma(-a[C1], rn, 1.0), rn);
    r = rn;
    npc = npn;
  }
  __builtin_amdgcn_sched_barrier(0);
}

// wavefront 0: right-looking elimination of the 16 columns of sub-block sb of the 64 x 64
// diagonal tile; emits L into M (rows of the tile at and below the sub-block), W = L D of the
// rows below the 16 x 16 pivot tile into Wt, D and 1 / D.  (Rows ABOVE the sub-block ride along
// with zeros, and the pivot rows ride along as copies of themselves: what they store above the
// diagonal of the tile is never read.)
__device__ __forceinline__ void chain_a_plus(double (*M)[C_LD], double (*Wt)[C_WLD], double *dD,
                                             double *dI, int &s_bad, int lane, int sb, int ncol) {
  const int cb = sb * 16, prow = lane & 15;
  double a[16], b[16];
#pragma unroll
  for (int k = 0; k < 16; k += 2) {
    const double2_t v = *reinterpret_cast<const double2_t *>(&M[cb + prow][cb + k]);
    const double2_t u = *reinterpret_cast<const double2_t *>(&M[lane][cb + k]);
    a[k] = v.x;
    a[k + 1] = v.y;
    b[k] = u.x;
    b[k + 1] = u.y;
  }
  double r = __builtin_amdgcn_rcp(a[0]);
  r = fma(r, fma(-a[0], r, 1.0), r);
  double npc = -a[0] * dpp_bcast<1>(a[0]);
  double dmine = 1.0;
  double *mrow = &M[lane][cb], *wrow = &Wt[lane][0];
  chain_a_col<0>(a, b, r, npc, dmine, prow, mrow, wrow);
  chain_a_col<1>(a, b, r, npc, dmine, prow, mrow, wrow);
  chain_a_col<2>(a, b, r, npc, dmine, prow, mrow, wrow);
  chain_a_col<3>(a, b, r, npc, dmine, prow, mrow, wrow);
  chain_a_col<4>(a, b, r, npc, dmine, prow, mrow, wrow);
  chain_a_col<5>(a, b, r, npc, dmine, prow, mrow, wrow);
  chain_a_col<6>(a, b, r, npc, dmine, prow, mrow, wrow);
  chain_a_col<7>(a, b, r, npc, dmine, prow, mrow, wrow);
  chain_a_col<8>(a, b, r, npc, dmine, prow, mrow, wrow);
  chain_a_col<9>(a, b, r, npc, dmine, prow, mrow, wrow);
  chain_a_col<10>(a, b, r, npc, dmine, prow, mrow, wrow);
  chain_a_col<11>(a, b, r, npc, dmine, prow, mrow, wrow);
  chain_a_col<12>(a, b, r, npc, dmine, prow, mrow, wrow);
  chain_a_col<13>(a, b, r, npc, dmine, prow, mrow, wrow);
  chain_a_col<14>(a, b, r, npc, dmine, prow, mrow, wrow);
  chain_a_col<15>(a, b, r, npc, dmine, prow, mrow, wrow);
  const int tr = lane - cb;  // row inside the 16 x 16 pivot tile
  const bool piv = tr >= 0 && tr < 16;
  // classes flagged bad: sNaN, qNaN, -inf, -0, +0, +inf
  const bool isbad = __builtin_amdgcn_class(dmine, 0x1 | 0x2 | 0x4 | 0x20 | 0x40 | 0x200);
  const bool bad_any = __ballot(piv && isbad && lane < ncol) != 0ull;
  if (piv) {
    M[lane][lane] = dmine;  // (behind the riding copy's store of a 1 at this place)
    dD[lane] = dmine;
    dI[lane] = isbad ? 0.0 : fast_recip(dmine);
    if (tr == 0 && bad_any) s_bad = 1;
  }
}

// one lane per stack row below the diagonal tile: x L_bb^T = a_row for sub-block sbp; X (= L D)
// replaces the row's entries in place.  The lane holds pivot row (lane & 15) of W = L D of the
// factored tile (from M and D: chain_a_plus left L below the tile's diagonal), the multipliers
// come as DPP broadcasts: x[K] -= (x[C] / d_C) * W[K][C].
template <int C>
__device__ __forceinline__ void chain_b_col(double (&x)[16], const double (&w)[16], double di) {
  const double m = -x[C] * dpp_bcast<C>(di);
#define CH_UX(K) \
  if (K > C) dpp_fmac<K>(x[K], w[C], m);
  CH_UX(1) CH_UX(2) CH_UX(3) CH_UX(4) CH_UX(5) CH_UX(6) CH_UX(7) CH_UX(8) CH_UX(9) CH_UX(10)
  CH_UX(11) CH_UX(12) CH_UX(13) CH_UX(14) CH_UX(15)
#undef CH_UX
  __builtin_amdgcn_sched_barrier(0);  // eager (right-looking) order, see chain_a_plus
}
__device__ __forceinline__ void chain_b_own(double (*M)[C_LD], int row, int sbp, int lane,
                                            const double *dD, const double *dI) {
  const int cb = sbp * 16, prow = lane & 15;
  double x[16], w[16];
#pragma unroll
  for (int k = 0; k < 16; k += 2) {
    const double2_t v = *reinterpret_cast<const double2_t *>(&M[row][cb + k]);
    const double2_t l = *reinterpret_cast<const double2_t *>(&M[cb + prow][cb + k]);
    const double2_t d = *reinterpret_cast<const double2_t *>(&dD[cb + k]);
    x[k] = v.x;
    x[k + 1] = v.y;
    w[k] = l.x * d.x;  // (entries on and above the diagonal: D itself or junk, never broadcast)
    w[k + 1] = l.y * d.y;
  }
  const double di = dI[cb + prow];
  chain_b_col<0>(x, w, di);
  chain_b_col<1>(x, w, di);
  chain_b_col<2>(x, w, di);
  chain_b_col<3>(x, w, di);
  chain_b_col<4>(x, w, di);
  chain_b_col<5>(x, w, di);
  chain_b_col<6>(x, w, di);
  chain_b_col<7>(x, w, di);
  chain_b_col<8>(x, w, di);
  chain_b_col<9>(x, w, di);
  chain_b_col<10>(x, w, di);
  chain_b_col<11>(x, w, di);
  chain_b_col<12>(x, w, di);
  chain_b_col<13>(x, w, di);
  chain_b_col<14>(x, w, di);
#pragma unroll
  for (int k = 0; k < 16; k += 2) {
    double2_t wv;
    wv.x = x[k];
    wv.y = x[k + 1];
    *reinterpret_cast<double2_t *>(&M[row][cb + k]) = wv;
  }
}

// C (16 x 16 at M[ci][cj]) -= A B^T over 16 k: A rows at (ar, ak) of Am (stride lda doubles),
// B rows at M[br][bk]
template <int LDA>
__device__ __forceinline__ void chain_tile16(double (*M)[C_LD], int ci, int cj,
                                             const double (*Am)[LDA], int ar, int ak, int br,
                                             int bk, int l15, int l4) {
  double4_t acc;
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = M[ci + l4 + 4 * r][cj + l15];
#pragma unroll
  for (int ks = 0; ks < 16; ks += 4) {
    const double av = -Am[ar + l15][ak + ks + l4];
    const double bv = M[br + l15][bk + ks + l4];
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) M[ci + l4 + 4 * r][cj + l15] = acc[r];
}

// block column Q of the inverse of a unit-lower 64 x 64 tile whose diagonal 16 x 16 sub-tiles
// already hold their inverses (see the end of k_diag_chain); one wavefront.  Xo[p - Q - 1] =
// block (p, Q), p > Q, in MFMA C layout.
template <int Q>
__device__ __forceinline__ void inv_block_column(const double (*Lg)[C_LD], double4_t (&Xo)[3],
                                                 int l15, int l4) {
  double4_t X[4];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) X[Q][rr] = Lg[16 * Q + 4 * rr + l4][16 * Q + l15];
#pragma unroll
  for (int p = Q + 1; p < 4; ++p) {
    double4_t S = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int r = Q; r < p; ++r)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        S = __builtin_amdgcn_mfma_f64_16x16x4f64(Lg[16 * p + l15][16 * r + 4 * rr + l4], X[r][rr], S,
                                                 0, 0, 0);
    double4_t Xp = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
      Xp = __builtin_amdgcn_mfma_f64_16x16x4f64(-Lg[16 * p + l15][16 * p + 4 * rr + l4], S[rr], Xp, 0,
                                                0, 0);
    X[p] = Xp;
    Xo[p - Q - 1] = Xp;
  }
}

// ---- helper workgroups of the chain (same launch, same XCD: workgroup ids 0, 8 and 16)
// The chain workgroup hands each finished 64-column sub-panel to two helpers through stamps in
// global memory: helper T applies the sub-panel to the part of the diagonal block the chain
// does not need for its NEXT sub-panel, helper I inverts the sub-panel's unit-lower tile.  Both
// used to sit at the end of the chain's own critical path.  Protocol as for the chained solves
// (pgf_ldlt.hip): producer drains its stores (s_waitcnt vmcnt(0)) behind a barrier, then ONE
// lane stores the epoch stamp with an L1-bypassing access; the consumer polls it (bounded) and
// reads the data through its own, freshly invalidated L1 or with L1-bypassing loads; producer
// and consumer share an L2 because ids that are multiples of 8 land on one XCD -- checked at run
// time through HW_REG_XCC_ID.  A failed check or a timed-out wait sets flags[2]; the host then
// repeats the factorisation without helpers.
#define HC_STAMP 0  // [0, 4): sub-panel s written back (chain -> helpers)
#define HC_DONE 4   // [4, 8): deferred tiles of sub-panel s updated (helper T -> chain)
#define HC_XCC 8    // max over the three roles of (epoch << 4 | xcc)
#define HC_WORDS 16
#define HELP_SPIN_LIMIT (1 << 18)

__device__ __forceinline__ void help_wait(const int *stamp, int epoch, int *flags) {
  for (int it = 0; it < HELP_SPIN_LIMIT; ++it) {
    if (__hip_atomic_load(stamp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == epoch) return;
    __builtin_amdgcn_s_sleep(1);
  }
  atomicOr(&flags[2], 2);
}
__device__ __forceinline__ void help_post(int *stamp, int epoch) {
  __hip_atomic_store(stamp, epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void help_check_xcc(int *hc, int epoch, int *flags) {
  const int ep = epoch & 0x7ffffff;
  const int mine = (ep << 4) | (int)(__builtin_amdgcn_s_getreg(6164) & 15);  // XCC_ID[3:0]
  const int old = atomicMax(&hc[HC_XCC], mine);
  if ((old >> 4) == ep && old != mine) atomicOr(&flags[2], 1);
}
__device__ __forceinline__ double ld_agent(const double *p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// inverse of the unit-lower 64 x 64 diagonal tile g of the block (rows / columns from b0), by
// the four wavefronts [4 slot, 4 slot + 4) of the workgroup.  Blocked by 16:
// wavefront v inverts the 16 x 16 diagonal sub-tile v by substitution (lane c <-> column c),
// then wavefront q < 3 builds block column q of the inverse top down,
//   X_pq = -D_p sum_{r = q}^{p-1} L_pr X_rq   (D_p = inv(L_pp), X_qq = D_q),
// with MFMA: a 16 x 16 accumulator (row (l >> 4) + 4 reg, column l & 15) IS the B operand
// of the next four k-steps, so the X_rq stay in registers.  Stored as inv and as its
// transpose, [tile][row][64]: forward and backward solves both read coalesced rows.
// Three pieces: the unit-lower copy Lg in LDS, the inversion in place, the two stores.  (The
// chain's own last tile takes the same sums in another order of time: tail_column_step.)

// Lg <- the tile's unit-lower part from K (zeros above the diagonal, ones on it, identity
// beyond nbw columns); thread t of nt
__device__ __forceinline__ void inv_fill_global(double (*Lg)[C_LD], const double *K, int64_t ldk,
                                                int b0, int nbw, int t, int nt) {
  for (int idx = t; idx < 64 * 32; idx += nt) {
    const int row = idx >> 5, c2 = (idx & 31) * 2;
    double2_t v = (double2_t){0.0, 0.0};
    if (row < nbw) {
      const double *src = K + (int64_t)(b0 + row) * ldk + b0 + c2;
      if (c2 + 1 < row) v = *reinterpret_cast<const double2_t *>(src);
      else if (c2 < row) v.x = *src;
    }
    if (c2 == row) v.x = 1.0;
    if (c2 + 1 == row) v.y = 1.0;
    *reinterpret_cast<double2_t *>(&Lg[row][c2]) = v;
  }
}

// D_t = inverse of the unit-lower 16 x 16 diagonal sub-tile t of the tile in Ls (only its entries
// below the diagonal are read), by substitution: lane c < 16 <-> column c; written to the same
// place of Dd (which may be Ls itself: a row is stored once no later step reads it, see below).
// Fifteen dependent steps of a few FMAs each, each behind the LDS reads of its column: from step
// INV_PF on, column c + 1 is fetched while column c is applied (the kernels have no registers
// for two whole columns beside y in the first steps).  Row c is final after step c - 1 and stored
// at once: no later step reads it.
#define INV_PF 5
__device__ __forceinline__ void inv_diag16(const double (*Ls)[C_LD], double (*Dd)[C_LD], int t, int lane) {
  if (lane < 16) {
    double y[16], cur[16], nxt[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) y[j] = (j == lane) ? 1.0 : 0.0;
#pragma unroll
    for (int c = 0; c < 15; ++c) {
      if (c <= INV_PF) {
#pragma unroll
        for (int j = c + 1; j < 16; ++j) cur[j] = Ls[16 * t + j][16 * t + c];
      }
      if (c >= INV_PF) {
#pragma unroll
        for (int j = c + 2; j < 16; ++j) nxt[j] = Ls[16 * t + j][16 * t + c + 1];
      }
      const double yc = y[c];
      Dd[16 * t + c][16 * t + lane] = yc;
#pragma unroll
      for (int j = c + 1; j < 16; ++j) y[j] = fma(-yc, cur[j], y[j]);
      __builtin_amdgcn_sched_barrier(0);
      if (c >= INV_PF) {
#pragma unroll
        for (int j = c + 2; j < 16; ++j) cur[j] = nxt[j];
      }
    }
    Dd[16 * t + 15][16 * t + lane] = y[15];
  }
}

// Lg (complete, behind a barrier) <- its inverse, in place.  Every thread of the workgroup calls
// this (three barriers, the last one behind the inverse's last LDS store); `live` says whether
// the thread's wavefront is one of the tile's four, v = its number among them.
__device__ __forceinline__ void inv_lds(double (*Lg)[C_LD], bool live, int v, int lane) {
  const int l15 = lane & 15, l4 = lane >> 4;
  if (live) inv_diag16(Lg, Lg, v, lane);
  __syncthreads();
  double4_t Xo[3];
  if (live) {
    if (v == 0) inv_block_column<0>(Lg, Xo, l15, l4);
    else if (v == 1) inv_block_column<1>(Lg, Xo, l15, l4);
    else if (v == 2) inv_block_column<2>(Lg, Xo, l15, l4);
  }
  __syncthreads();  // every wavefront is done reading the L blocks: the X blocks go in place
  if (live && v < 3) {
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      const int pb = v + 1 + t;
      if (pb < 4) {
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) Lg[16 * pb + l4 + 4 * rr][16 * v + l15] = Xo[t][rr];
      }
    }
  }
  __syncthreads();
}

// the inverse in Lg -> Linv and LinvT of tile b0 / 64; thread t of nt
__device__ __forceinline__ void inv_store(const double (*Lg)[C_LD], int b0, double *__restrict__ Linv,
                                          double *__restrict__ LinvT, int t, int nt) {
  double *o = Linv + (size_t)(b0 / 64) * 4096;
  double *ot = LinvT + (size_t)(b0 / 64) * 4096;
  for (int idx = t; idx < 64 * 64; idx += nt) {
    const int row = idx >> 6, col = idx & 63;
    o[idx] = Lg[row][col];
    ot[idx] = Lg[col][row];
  }
}

// ---- the chain's own inverse of its block's LAST tile (chain_body, PGF_CHAIN_TAIL), pipelined
// with the tile's elimination.  Column block t of the factored tile in M[0..63] is final once
// chain_a_plus has eliminated it, so the same sums as above can be taken apart by the column block
// they read: wavefront q + 1 (q < 3; never wavefront 0's SIMD) owns block column q of the inverse
// and, as soon as column block t >= q is final, forms
//   D_t by substitution (each of the three for itself: no hand-over between wavefronts),
//   X_tq = D_q (t == q) or -D_t S_t (S_t is complete: its last term came with column block t - 1),
//   S_p += L_pt X_tq for every p > t       (S_p = sum_{r = q}^{p-1} L_pr X_rq, r ascending)
// -- per entry invert_tile's operations in invert_tile's order.  Between two calls everything
// lives in the wavefront's own 64 rows of M (rows 64 (q + 1) ..: free, nothing lies below a last
// tile), laid out like the tile: D_t at block (t, t), X_tq and the unfinished S_p at block (., q).
// After the call for t = 3 those rows hold block column q of the inverse (and D_3 at (3, 3)).
__device__ __forceinline__ void tail_column_step(double (*M)[C_LD], int t, int q, int lane) {
  if (t < q) return;
  // (laundered here: no address of this function is formed ahead of the call and kept alive
  // across the eliminations of the sub-panels in front, cf. chain_body)
  asm volatile("" : "+v"(lane));
  double(*P)[C_LD] = M + 64 * (q + 1);
  const int l15 = lane & 15, l4 = lane >> 4;
  inv_diag16(M, P, t, lane);
  __builtin_amdgcn_wave_barrier();  // (LDS serves a wavefront's accesses in order)
  double4_t X;
  if (t == q) {
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) X[rr] = P[16 * q + 4 * rr + l4][16 * q + l15];
  } else {
    double4_t S;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) S[rr] = P[16 * t + l4 + 4 * rr][16 * q + l15];
    X = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
      X = __builtin_amdgcn_mfma_f64_16x16x4f64(-P[16 * t + l15][16 * t + 4 * rr + l4], S[rr], X, 0, 0, 0);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) P[16 * t + l4 + 4 * rr][16 * q + l15] = X[rr];
  }
#pragma unroll
  for (int pp = 1; pp < 4; ++pp) {  // (unrolled: the three sums are independent)
    const int p = t + pp;
    if (p >= 4) break;
    double4_t S = (double4_t){0.0, 0.0, 0.0, 0.0};
    if (t > q) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) S[rr] = P[16 * p + l4 + 4 * rr][16 * q + l15];
    }
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)
      S = __builtin_amdgcn_mfma_f64_16x16x4f64(M[16 * p + l15][16 * t + 4 * rr + l4], X[rr], S, 0, 0, 0);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) P[16 * p + l4 + 4 * rr][16 * q + l15] = S[rr];
  }
}
// entry (row, col) of the inverse the three wavefronts have left behind
__device__ __forceinline__ double tail_entry(const double (*M)[C_LD], int row, int col) {
  const int bc = col >> 4;
  return (row >> 4) < bc ? 0.0 : M[64 * (min(bc, 2) + 1) + row][col];
}

// fill from global memory, invert, store: every thread of the workgroup calls this (barriers),
// `live` says whether its wavefront group has a tile.  st (PGF_CHAIN_TIMING, else null): thread 0
// stamps "tile in LDS" into st[1] and "inverse stored" (its own stores drained) into st[2].
__device__ __forceinline__ void invert_tile(unsigned char *smem, const double *K, int64_t ldk,
                                            int b0, int nbw, bool live, double *__restrict__ Linv,
                                            double *__restrict__ LinvT, long long *st = nullptr) {
  // wave: uniform per wavefront -> scalar register, role tests and tile numbers on the SALU
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  double(*Lg)[C_LD] = reinterpret_cast<double(*)[C_LD]>(smem + (size_t)(wave >> 2) * 64 * C_LD * 8);
  if (live) inv_fill_global(Lg, K, ldk, b0, nbw, tid & 255, 256);
  __syncthreads();
  if (st && tid == 0) st[1] = wall_clock64();
  inv_lds(Lg, live, wave & 3, lane);
  if (live) inv_store(Lg, b0, Linv, LinvT, tid & 255, 256);
  if (st && tid == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    st[2] = wall_clock64();
  }
  __syncthreads();  // Lg is refilled by the next pass
}

// 16 x 16 sub-tiles on or below the diagonal of a lower-triangular region of nt 64-row tiles,
// tile (I, J), J <= I, holding 10 (I == J) or 16 of them; (mi, mj) = offsets inside the region
__device__ __forceinline__ void decode_subtile(int e, int &mi, int &mj) {
  int I = 0, J = 0;
  while (true) {
    const int cnt = (I == J) ? 10 : 16;
    if (e < cnt) break;
    e -= cnt;
    if (++J > I) {
      J = 0;
      ++I;
    }
  }
  int ti, tj;
  if (I == J) {
    ti = (e >= 6) ? 3 : (e >= 3) ? 2 : (e >= 1) ? 1 : 0;
    tj = e - ti * (ti + 1) / 2;
  } else {
    ti = e >> 2;
    tj = e & 3;
  }
  mi = 64 * I + 16 * ti;
  mj = 64 * J + 16 * tj;
}

// helper T (workgroup 8): for every sub-panel s with rows beyond the NEXT sub-panel, apply it to
// the lower triangle of those rows / columns [cb + 128, bend): C -= (L D) L^T with L read back
// from global memory (the chain wrote L = X D^-1; X itself stays in its LDS)
__device__ __forceinline__ void helper_tiles(unsigned char *smem, double *K, int64_t ldk, int c0,
                                             int nb, const double *dvec, int *hc, int epoch,
                                             int *flags) {
  constexpr int NT = 64 * CH_WAVES;
  double(*Mh)[C_LD] = reinterpret_cast<double(*)[C_LD]>(smem);
  double *dDs = reinterpret_cast<double *>(smem + 128 * C_LD * 8);
  // wave: uniform per wavefront -> scalar register, role tests and tile numbers on the SALU
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int bend = c0 + nb, ns = (nb + 63) / 64;
  if (tid == 0) help_check_xcc(hc, epoch, flags);
  for (int s = 0; s + 2 < ns; ++s) {
    const int cb = c0 + 64 * s, r0 = cb + 128;
    const int rows = bend - r0, rowsp = (rows + 63) & ~63, nt = rowsp / 64;
    if (tid == 0) help_wait(hc + HC_STAMP + s, epoch, flags);
    __syncthreads();
    for (int p = tid; p < rowsp * 32; p += NT) {
      const int row = p >> 5, c2 = (p & 31) * 2;
      double2_t t = (double2_t){0.0, 0.0};
      if (row < rows) t = *reinterpret_cast<const double2_t *>(K + (int64_t)(r0 + row) * ldk + cb + c2);
      *reinterpret_cast<double2_t *>(&Mh[row][c2]) = t;
    }
    if (tid < 64) dDs[tid] = dvec[cb + tid];
    __syncthreads();
    const int total = nt * (nt + 1) / 2 * 16 - nt * 6;
    for (int e = wave; e < total; e += CH_WAVES) {
      int mi, mj;
      decode_subtile(e, mi, mj);
      const int gi = r0 + mi, gj = r0 + mj, j = gj + l15;
      double4_t c = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = gi + l4 + 4 * r;
        if (i < bend && j < bend && j <= i) c[r] = ld_agent(K + (int64_t)i * ldk + j);
      }
#pragma unroll 4
      for (int ks = 0; ks < 64; ks += 4) {
        const double av = -Mh[mi + l15][ks + l4] * dDs[ks + l4];
        const double bv = Mh[mj + l15][ks + l4];
        c = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, c, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = gi + l4 + 4 * r;
        if (i < bend && j < bend && j <= i) K[(int64_t)i * ldk + j] = c[r];
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) help_post(hc + HC_DONE + s, epoch);
  }
}

// The chain inverts its block's LAST diagonal tile itself (PGF_CHAIN_TAIL, `tail`) when that tile
// is a full one: it still holds the tile in LDS when helper I could only begin to fetch it.  A
// ragged last tile stays with helper I.  Chain and helper decide with this one test.
__device__ __forceinline__ bool chain_takes_last_tile(int tail, int nb) {
  return tail && nb > 0 && (nb & 63) == 0;
}

// PGF_CHAIN_TIMING: helper I's stamps live behind the chain's in the same buffer, three per
// sub-panel: released from help_wait, tile in LDS, inverse stored
#define CH_DBG_CHAIN 32
#define CH_DBG_WORDS (CH_DBG_CHAIN + 12)

// helper I (workgroup 16): the inverse of every sub-panel's diagonal tile as soon as it is final
// (but for the one the chain takes itself)
__device__ __forceinline__ void helper_inverses(unsigned char *smem, const double *K, int64_t ldk,
                                                int c0, int nb, int *hc, int epoch, int *flags,
                                                double *__restrict__ Linv,
                                                double *__restrict__ LinvT, int tail,
                                                long long *__restrict__ dbg = nullptr) {
  const int tid = threadIdx.x, wave = tid >> 6;
  const int bend = c0 + nb, ns = (nb + 63) / 64;
  const int mine = chain_takes_last_tile(tail, nb) ? ns - 1 : ns;
  if (tid == 0) help_check_xcc(hc, epoch, flags);
  for (int s = 0; s < mine; ++s) {
    const int b0 = c0 + 64 * s;
    long long *st = (dbg && s < 4) ? dbg + CH_DBG_CHAIN + 3 * s : nullptr;
    if (tid == 0) {
      help_wait(hc + HC_STAMP + s, epoch, flags);
      if (st) st[0] = wall_clock64();
    }
    __syncthreads();
    invert_tile(smem, K, ldk, b0, min(64, bend - b0), wave < 4, Linv, LinvT, st);
  }
}

template <bool HELP>
__device__ __forceinline__ void chain_body(unsigned char *smem, double *K, int64_t ldk, int c0,
                                           int nb, double *__restrict__ dvec,
                                           double *__restrict__ dinv, int *__restrict__ flags,
                                           double *__restrict__ Linv, double *__restrict__ LinvT,
                                           long long *__restrict__ dbg, int *hc, int epoch,
                                           int tail) {
  double(*M)[C_LD] = reinterpret_cast<double(*)[C_LD]>(smem);
  double(*Wt)[C_WLD] = reinterpret_cast<double(*)[C_WLD]>(smem + CH_ROWS * C_LD * 8);
  double *dD = reinterpret_cast<double *>(smem + CH_ROWS * C_LD * 8 + 2 * 64 * C_WLD * 8);
  double *dI = dD + 64;
  int &s_bad = *reinterpret_cast<int *>(dI + 64);
  constexpr int NT = 64 * CH_WAVES;
  // wave: uniform per wavefront -> scalar register, role tests and tile numbers on the SALU
  const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int bend = c0 + nb;
  const int ns = (nb + 63) / 64;
  const bool own_last = HELP && chain_takes_last_tile(tail, nb);  // (see "the last tile" below)
  // PGF_CHAIN_TIMING: phase stamps of the first sub-panel (100 MHz wall clock), thread 0
  int dbi = 0;
#define CH_STAMP()                                                         \
  do {                                                                     \
    if (dbg && tid == 0 && dbi < CH_DBG_CHAIN) dbg[dbi++] = wall_clock64(); \
  } while (0)
  CH_STAMP();
  if (HELP && tid == 0) help_check_xcc(hc, epoch, flags);

  bool preloaded = false, early0 = false;
  double *dIo = dI + 64 + 2;  // 1/D of the sub-panel just factored (behind the flag word)
  for (int s = 0; s < ns; ++s) {
    // Thread and wavefront indices are laundered once per sub-panel: otherwise every address
    // and role predicate of the loop body is hoisted to the kernel entry and kept alive across
    // the eliminations, where a lane has no register to spare (128 in a 16-wavefront workgroup):
    // 60 spilled registers, and a first scratch access costs microseconds.
    int tl_ = threadIdx.x, wv_ = wave;
    asm volatile("" : "+v"(tl_), "+s"(wv_));
    const int tid = tl_, lane = tid & 63, wave = wv_;
    const int l15 = lane & 15, l4 = lane >> 4;
    const int cb = c0 + 64 * s;
    const int ncol = min(64, bend - cb);
    const int own = max(0, bend - cb - 64);  // block rows below the tile (ncol == 64 if any)
    const int ownp = (own + 63) & ~63;       // padded to whole wavefronts of rows
    if (tid == 0 && !early0) s_bad = 0;
    // ---- load the stack: diagonal tile (identity outside the valid lower triangle) + the
    // block's rows below, all loads of a lane in flight before its first LDS store.  Not for
    // a stack the previous sub-panel's in-block update has left in M already (see there).
    if (!preloaded) {
      constexpr int NQ = 8192 / NT;
      double2_t v[NQ];
      const int np = (64 + ownp) * 32;
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int p = q * NT + tid;
        const int row = p >> 5, c2 = (p & 31) * 2;
        double2_t t = (double2_t){0.0, 0.0};
        if (p < np) {
          if (row < 64) {
            if (row < ncol) {
              const double *src = K + (int64_t)(cb + row) * ldk + cb + c2;
              if (c2 + 1 <= row) t = *reinterpret_cast<const double2_t *>(src);
              else if (c2 <= row) t.x = *src;
            } else {
              if (c2 == row) t.x = 1.0;
              if (c2 + 1 == row) t.y = 1.0;
            }
          } else if (row < 64 + own) {
            t = *reinterpret_cast<const double2_t *>(K + (int64_t)(cb + row) * ldk + cb + c2);
          }
        }
        v[q] = t;
      }
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int p = q * NT + tid;
        if (p < np) *reinterpret_cast<double2_t *>(&M[p >> 5][(p & 31) * 2]) = v[q];
      }
    }
    __syncthreads();
    CH_STAMP();  // stack loaded

    // ---- 64-column panel, four 16-column steps.  Critical path = wavefront 0 (a+); the rows
    // below the tile follow one step behind on wavefronts 1..3 (64 rows each).  The rank-16
    // MFMA updates are split by urgency: what the NEXT phase 1 reads -- column block sb + 1 of
    // the diagonal tile (step sb) and column block sb of the rows below (step sb - 1) -- is
    // updated between the two barriers of the step; every other tile waits for the idle
    // wavefronts 4.. of the following phase 1, in the shadow of (a+).  W = L D of the diagonal
    // rows is double buffered (Wt[sb & 1]) because of that.
    //   update of diagonal tile (ti, tj) by step t: urgent if tj == t + 1 (phase 2 of step t),
    //                                               else phase 1 of step t + 1;
    //   update of lower    tile (ti, tj) by step t: urgent if tj == t + 1 (phase 2 of step t + 1),
    //                                               else phase 1 of step t + 2.
    const int ot = ownp / 16;  // 16-row tiles below the diagonal tile
    auto diag_tile = [&](int t, int ti, int tj) {  // step t applied to diagonal tile (ti, tj)
      chain_tile16<C_WLD>(M, ti * 16, tj * 16, Wt + (t & 1) * 64, ti * 16, 0, tj * 16, t * 16, l15, l4);
    };
    auto own_tile = [&](int t, int ti, int tj) {  // step t applied to lower tile (ti, tj), ti >= 4
      chain_tile16<C_LD>(M, ti * 16, tj * 16, M, ti * 16, t * 16, tj * 16, t * 16, l15, l4);
    };
    for (int sb = 0; sb < 4; ++sb) {
      if (wave == 0) {
        // (step 0 of a stack built in place has been eliminated beside the tail of the
        // previous sub-panel's in-block update already)
        if (!(early0 && sb == 0)) chain_a_plus(M, Wt + (sb & 1) * 64, dD, dI, s_bad, lane, sb, ncol);
      } else if (wave <= 3) {
        if (sb > 0 && 64 * (wave - 1) < own) chain_b_own(M, 64 * wave + lane, sb - 1, lane, dD, dI);
        // the block's last tile: its inverse follows the elimination one step behind
        if (own_last && s == ns - 1 && sb > 0) tail_column_step(M, sb - 1, wave - 1, lane);
      } else {
        // deferred tiles: diagonal (ti, tj), tj in [sb + 1, 3], of step sb - 1; lower (ti, tj),
        // tj in [sb, 3], of step sb - 2
        const int ndd = sb >= 1 ? (3 - sb) * (4 - sb) / 2 : 0;
        const int ndo = sb >= 2 ? ot * (4 - sb) : 0;
        // (wavefronts 4, 8, 12 share wavefront 0's SIMD: they stay out of its way; the other
        // nine of 4..15 take the tiles in turn)
        const int w4 = wave - 4;
        const int rk = (w4 & 3) ? w4 - (w4 >> 2) - 1 : -1;
        for (int e0 = rk; rk >= 0 && e0 < ndd + ndo; e0 += 9) {
          if (e0 < ndd) {
            int e = e0, tj = sb + 1;
            while (e >= 4 - tj) {
              e -= 4 - tj;
              ++tj;
            }
            diag_tile(sb - 1, tj + e, tj);
          } else {
            const int e = e0 - ndd;
            own_tile(sb - 2, 4 + e % ot, sb + e / ot);
          }
        }
        // helper T has had three steps to finish what it was handed one sub-panel ago:
        // everything this sub-panel's in-block update fetches after step 3
        if (HELP && sb == 3 && tid == NT - 64 && s >= 1 && s + 1 < ns)
          help_wait(hc + HC_DONE + s - 1, epoch, flags);
      }
      __syncthreads();
      if (s == 0) CH_STAMP();  // phase 1 of step sb
      // urgent tiles: diagonal (ti, sb + 1), ti in [sb + 1, 3], of step sb; lower (ti, sb) of
      // step sb - 1
      const int nud = 3 - sb;
      const int nuo = sb >= 1 ? ot : 0;
      for (int e0 = wave; e0 < nud + nuo; e0 += CH_WAVES) {
        if (e0 < nud) diag_tile(sb, sb + 1 + e0, sb + 1);
        else own_tile(sb - 1, 4 + (e0 - nud), sb);
      }
      __syncthreads();
    }
    if (s == 0) CH_STAMP();  // four steps done
    // the block's last tile, full, with helpers: written back behind the loop, where its
    // inverse is finished
    if (own_last && s == ns - 1) break;
    // ---- trailing update inside the block (rows / columns below the tile, K-depth 64, A = -X
    // from M, B = X D^-1): the C tiles live in global memory; ALL of a wavefront's tiles are
    // fetched in one burst here, so that their latency (they were last written by another
    // kernel: HBM / Infinity Cache, ~2 us) is paid once and hides behind the write-back.
    // Only 16 x 16 sub-tiles on or below the diagonal are enumerated, dealt round-robin: the
    // phase is bound by the CU's matrix pipes, every wavefront should carry the same number.
    // With helpers only the tiles of the NEXT sub-panel's columns are this workgroup's: tile
    // column 0 of the region, 10 + 16 (nt - 1) sub-tiles; the rest is helper T's.
    constexpr int MT = ((HELP ? 42 : 78) + CH_WAVES - 1) / CH_WAVES;  // sub-tiles per wavefront, at most
    const int nt = ownp / 64;
    const int total = HELP ? (nt ? 10 + 16 * (nt - 1) : 0) : nt * (nt + 1) / 2 * 16 - nt * 6;
    auto decode = [&](int e, int &gi, int &gj, int &mi, int &mj) {
      if (HELP) {
        if (e < 10) {
          const int ti = (e >= 6) ? 3 : (e >= 3) ? 2 : (e >= 1) ? 1 : 0;
          mi = 16 * ti;
          mj = 16 * (e - ti * (ti + 1) / 2);
        } else {
          mi = 64 + 16 * ((e - 10) >> 2);  // tile row 1 + (e - 10) / 16, sub-row ((e - 10) / 4) % 4
          mj = 16 * ((e - 10) & 3);
        }
      } else {
        decode_subtile(e, mi, mj);
      }
      mi += 64;
      mj += 64;
      gi = cb + mi;
      gj = cb + mj;
    };
    // whole 64-row tiles below (no ragged edge): the next stack is built in place
    const bool direct = own > 0 && (own & 63) == 0;
    double4_t ct[MT];
    early0 = false;
    if (HELP && direct) {
      // ---- With helpers and whole tiles the sub-panel boundary is pipelined:
      //  A  wavefronts 1-3 finish the lagging rows (step 3); the others fetch their C sub-tiles
      //     and write the factored tile, D, 1/D and the flags back meanwhile
      //  B  L rows written back; first round of MFMA sub-tiles = the NEXT diagonal tile (plus
      //     six others), which goes straight into M[0..63]; stamp to the helpers
      //  C  wavefront 0 eliminates step 0 of the next sub-panel while the others finish the
      //     remaining sub-tiles (in registers: M's rows 64.. are still their operands)
      //  D  those go into M as the rest of the next stack
      auto eidx = [&](int q) {  // sub-tile of round q: round 0 one per wavefront, then 1..15 only
        if (q == 0) return wave;
        return wave == 0 ? total : CH_WAVES + (wave - 1) + (CH_WAVES - 1) * (q - 1);
      };
      // (the C loads of wavefronts 1-3 are in flight while they finish the lagging rows)
#pragma unroll
      for (int q = 0; q < MT; ++q) {
        const int e = eidx(q);
        ct[q] = (double4_t){0.0, 0.0, 0.0, 0.0};
        if (e < total) {
          int gi, gj, mi, mj;
          decode(e, gi, gj, mi, mj);
          const int j = gj + l15;
#pragma unroll
          for (int r = 0; r < 4; ++r) ct[q][r] = ld_agent(K + (int64_t)(gi + l4 + 4 * r) * ldk + j);
        }
      }
      if (s == 0) CH_STAMP();  // C loads issued
      if (wave >= 1 && wave <= 3 && 64 * (wave - 1) < own) chain_b_own(M, 64 * wave + lane, 3, lane, dD, dI);
      for (int p = tid; p < 64 * 64; p += NT) {
        const int row = p >> 6, c = p & 63;
        if (c <= row) K[(int64_t)(cb + row) * ldk + cb + c] = M[row][c];
      }
      if (s == 0) CH_STAMP();  // tile written back
      if (tid < 64) {
        dvec[cb + tid] = dD[tid];
        dinv[cb + tid] = dI[tid];
        dIo[tid] = dI[tid];
      }
      if (wave == 0) {
        const unsigned long long negs = __ballot(dD[lane] < 0.0);
        if (lane == 0) {
          if (s_bad) atomicOr(&flags[0], 1);
          s_bad = 0;  // for the early step 0 below
          const int neg = __popcll(negs);
          if (neg) atomicAdd(&flags[1], neg);
        }
      }
      if (s == 0) CH_STAMP();  // (wavefront 0) before the barrier
      __syncthreads();  // A -> B
      CH_STAMP();       // panel factored
      for (int p = tid; p < own * 32; p += NT) {
        const int row = 64 + (p >> 5), c2 = (p & 31) * 2;
        double2_t v = *reinterpret_cast<const double2_t *>(&M[row][c2]);
        v.x *= dIo[c2];
        v.y *= dIo[c2 + 1];
        *reinterpret_cast<double2_t *>(K + (int64_t)(cb + row) * ldk + cb + c2) = v;
      }
      auto mfma_sub = [&](int q) {
        const int e = eidx(q);
        if (e < total) {
          int gi, gj, mi, mj;
          decode(e, gi, gj, mi, mj);
          double4_t c = ct[q];
#pragma unroll 4
          for (int ks = 0; ks < 64; ks += 4) {
            const double av = -M[mi + l15][ks + l4];
            const double bv = M[mj + l15][ks + l4] * dIo[ks + l4];
            c = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, c, 0, 0, 0);
          }
          ct[q] = c;
        }
      };
      auto to_stack = [&](int q) {  // sub-tile of round q -> its place in the next stack
        const int e = eidx(q);
        if (e < total) {
          int gi, gj, mi, mj;
          decode(e, gi, gj, mi, mj);
          const int cj = mj - 64 + l15;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int ri = mi - 64 + l4 + 4 * r;
            M[ri][cj] = (cj <= ri) ? ct[q][r] : 0.0;
          }
        }
      };
      if (s == 0) CH_STAMP();  // L rows written back
      mfma_sub(0);
      if (s == 0) CH_STAMP();  // first MFMA round
      // rows 0..63 of M (the old tile) were last read by the write-back before A -> B
      if (wave < 10) to_stack(0);
      for (int p = tid; p < 6 * 256; p += NT) {  // the six sub-tiles above the new diagonal
        const int t6 = p >> 8, rr = (p >> 4) & 15, cc = p & 15;
        const int ti = (t6 >= 5) ? 2 : (t6 >= 3) ? 1 : 0;  // (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
        const int tj = (ti == 0) ? 1 + t6 : (ti == 1) ? t6 - 1 : 3;
        M[16 * ti + rr][16 * tj + cc] = 0.0;
      }
      if (s == 0) CH_STAMP();  // next diagonal tile stored
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // write-backs have left
      if (s == 0) CH_STAMP();  // stores drained
      __syncthreads();  // B -> C
      if (tid == 0) help_post(hc + HC_STAMP + s, epoch);
      CH_STAMP();  // next diagonal tile in place
      // (one barrier, reached on two paths: the branch is uniform per wavefront, and this way
      // no accumulator of the other path is live across the elimination, which has no
      // registers to spare)
      if (wave == 0) {
        chain_a_plus(M, Wt, dD, dI, s_bad, lane, 0, 64);
        __syncthreads();  // C -> D
      } else {
#pragma unroll
        for (int q = 1; q < MT; ++q) mfma_sub(q);
        __syncthreads();  // C -> D: nobody reads the old rows 64.. of M any more
        if (wave >= 10) to_stack(0);
#pragma unroll
        for (int q = 1; q < MT; ++q) to_stack(q);
      }
      preloaded = true;
      early0 = true;
    } else {
      if (wave >= 1 && wave <= 3 && 64 * (wave - 1) < own) chain_b_own(M, 64 * wave + lane, 3, lane, dD, dI);
      __syncthreads();
      CH_STAMP();  // panel factored
#pragma unroll
      for (int q = 0; q < MT; ++q) {
        const int e = wave + q * CH_WAVES;
        ct[q] = (double4_t){0.0, 0.0, 0.0, 0.0};
        if (e < total) {
          int gi, gj, mi, mj;
          decode(e, gi, gj, mi, mj);
          const int j = gj + l15;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int i = gi + l4 + 4 * r;
            if (i < bend && j < bend && j <= i)
              ct[q][r] = HELP ? ld_agent(K + (int64_t)i * ldk + j) : K[(int64_t)i * ldk + j];
          }
        }
      }
      // ---- write back: factored tile, D, 1/D, flags; rows below: L = X D^-1
      for (int p = tid; p < 64 * 64; p += NT) {
        const int row = p >> 6, c = p & 63;
        if (row < ncol && c <= row) K[(int64_t)(cb + row) * ldk + cb + c] = M[row][c];
      }
      if (tid < ncol) {
        dvec[cb + tid] = dD[tid];
        dinv[cb + tid] = dI[tid];
      }
      if (wave == 0) {
        const unsigned long long negs = __ballot(lane < ncol && dD[lane] < 0.0);
        if (lane == 0) {
          if (s_bad) atomicOr(&flags[0], 1);
          const int neg = __popcll(negs);
          if (neg) atomicAdd(&flags[1], neg);
        }
      }
      for (int p = tid; p < own * 32; p += NT) {
        const int row = 64 + (p >> 5), c2 = (p & 31) * 2;
        double2_t v = *reinterpret_cast<const double2_t *>(&M[row][c2]);
        v.x *= dI[c2];
        v.y *= dI[c2 + 1];
        *reinterpret_cast<double2_t *>(K + (int64_t)(cb + row) * ldk + cb + c2) = v;
      }
      if (s == 0) CH_STAMP();  // written back
#pragma unroll
      for (int q = 0; q < MT; ++q) {
        const int e = wave + q * CH_WAVES;
        if (e < total) {
          int gi, gj, mi, mj;
          decode(e, gi, gj, mi, mj);
          {
            double4_t c = ct[q];
#pragma unroll 4
            for (int ks = 0; ks < 64; ks += 4) {
              const double av = -M[mi + l15][ks + l4];
              const double bv = M[mj + l15][ks + l4] * dI[ks + l4];
              c = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, c, 0, 0, 0);
            }
            if (direct && mj < 128) {
              ct[q] = c;  // next sub-panel's stack: stays in registers until M is free
            } else {
              const int j = gj + l15;
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int i = gi + l4 + 4 * r;
                if (i < bend && j < bend && j <= i) K[(int64_t)i * ldk + j] = c[r];
              }
            }
          }
        }
      }
      if (HELP) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // write-backs have left
      __syncthreads();  // M is refilled next; the global tiles written above are read back
      if (HELP && tid == 0) help_post(hc + HC_STAMP + s, epoch);
      preloaded = direct;
      if (direct) {
        // the next sub-panel's stack (columns 64..127 of this one's rows 64..) goes from the
        // accumulators straight into M: no round trip through global memory
#pragma unroll
        for (int q = 0; q < MT; ++q) {
          const int e = wave + q * CH_WAVES;
          if (e < total) {
            int gi, gj, mi, mj;
            decode(e, gi, gj, mi, mj);
            if (mj < 128) {
              const int cj = mj - 64 + l15;
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                const int ri = mi - 64 + l4 + 4 * r;
                M[ri][cj] = (cj <= ri) ? ct[q][r] : 0.0;
              }
            }
          }
        }
        // the six 16 x 16 sub-tiles above the diagonal of the new diagonal tile
        for (int p = tid; p < 6 * 256; p += NT) {
          const int t6 = p >> 8, rr = (p >> 4) & 15, cc = p & 15;
          const int ti = (t6 >= 5) ? 2 : (t6 >= 3) ? 1 : 0;  // (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
          const int tj = (ti == 0) ? 1 + t6 : (ti == 1) ? t6 - 1 : 3;
          M[16 * ti + rr][16 * tj + cc] = 0.0;
        }
      }
    }
    CH_STAMP();  // in-block update done
  }

  // ---- the last tile (own_last): factored in M[0..63]; wavefronts 1-3 have brought their block
  // columns of its inverse as far as column block 2 allows (tail_column_step, rows 64.. of M).
  // They finish them -- D_3 and one product -- while the other thirteen write the tile, D, 1/D
  // and the flags back; then all sixteen store the inverse.  No stamp, no drained stores, no
  // read from global memory: helper I could only begin all of that once this workgroup had
  // ended.  Linv and LinvT are the same bits as invert_tile's.
  if (own_last) {
    int tl_ = threadIdx.x;
    asm volatile("" : "+v"(tl_));
    const int tid = tl_, lane = tid & 63;
    const int cb = c0 + 64 * (ns - 1);
    CH_STAMP();  // panel factored
    if (wave >= 1 && wave <= 3) {
      tail_column_step(M, 3, wave - 1, lane);
    } else {
      for (int p = wave == 0 ? tid : tid - 192; p < 64 * 64; p += NT - 192) {
        const int row = p >> 6, c = p & 63;
        if (c <= row) K[(int64_t)(cb + row) * ldk + cb + c] = M[row][c];
      }
      if (tid < 64) {
        dvec[cb + tid] = dD[tid];
        dinv[cb + tid] = dI[tid];
      }
      if (wave == 0) {
        const unsigned long long negs = __ballot(dD[lane] < 0.0);
        if (lane == 0) {
          if (s_bad) atomicOr(&flags[0], 1);
          const int neg = __popcll(negs);
          if (neg) atomicAdd(&flags[1], neg);
        }
      }
    }
    __syncthreads();
    CH_STAMP();  // inverted
    double *o = Linv + (size_t)(cb / 64) * 4096;
    double *ot = LinvT + (size_t)(cb / 64) * 4096;
    for (int idx = tid; idx < 64 * 64; idx += NT) {
      const int row = idx >> 6, col = idx & 63;
      o[idx] = tail_entry(M, row, col);
      ot[idx] = tail_entry(M, col, row);
    }
    if (dbg && tid == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (as helper I's last stamp)
  }

  // ---- inverses of the block's unit-lower diagonal tiles (invert_tile), four wavefronts per
  // tile; with helpers this is helper I's work (and, for the last tile, the code above)
  if (!HELP) {
    for (int g0 = 0; g0 < ns; g0 += CH_WAVES / 4) {
      const int g = g0 + (wave >> 2);
      const int b0 = c0 + 64 * g;
      invert_tile(smem, K, ldk, b0, min(64, bend - b0), g < ns, Linv, LinvT);
    }
  }
  CH_STAMP();  // inverses done
#undef CH_STAMP
}
