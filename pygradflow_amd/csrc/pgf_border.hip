// Bordered band: K = [[B, C], [C', D]] up to the plan's permutation, B banded (half-bandwidth <= 64,
// the existing cyclic reductions take it), C the Nb x k coupling to a border of k <= 64 KKT nodes
// (dense rows / columns: a budget constraint, a global parameter), D the k x k border block.
// 65 <= k <= 1024 (the large border): pgf_border_large.hip behind the same entry points.
//
// Block elimination of B first:
//   factor, once per assembled matrix:  Y = inv(B) C,  S = D - C' Y,  S = L D L'
//   solve, per right-hand side (ra, rb): v = inv(B) ra,  z = inv(S) (rb - C' v),  xa = v - Y z,  xb = z
// B is a principal submatrix of the symmetric quasi-definite K and S its Schur complement: both are
// quasi-definite again (the argument above k_bcr_extract, pgf_sparse.hip), so neither needs
// pivoting, and the negative eigenvalues of K are those of B plus those of S (Haynsworth).
//
// Storage (sparse.py lays the slots out, the scatter kernels of pgf_sparse.hip fill them): behind
// the (Nb + 1) x ldb band array C, row-major Nb x kp, then the lower triangle of D, kp x kp; kp = k
// rounded up to a multiple of 16, padding columns of C zero, padding of D the identity.  Active
// variables stay identity rows: an active border variable has a zero column in C and a unit row in D.
//
// Compiled with -ffp-contract=off (explicit fma() only), as pgf_sparse.hip.
#include <stdlib.h>

#include "pgf_band_dev.h"
#include "pgf_border_dev.h"
#include "pgf_band_batch.h"
#include "pgf_batch.h"
#include "pgf_env.h"
#include "pgf_sparse.h"

static inline dim3 g1(int n, int b = 256) { return dim3((n + b - 1) / b); }

// the banded solve of B: sp.vec.brhs[0, N) <- inv(B) sp.vec.brhs[0, N) (the solution is written in whole
// blocks: up to 63 entries behind N are overwritten)
static void band_solve(hipStream_t s, const SparseDev &sp, int N, int *flags) {
  if (sp.blk.B > 8)
    sp_launch_bw_solve(s, sp, N, flags, /*guard=*/false);
  else
    sp_launch_bcr_solve(s, sp, N, flags, /*guard=*/false);
}

// ---------------------------------------------------------------- kernels of one handle
// Thin wrappers of the device bodies in pgf_border_dev.h (shared with the batched twins at the
// end of this file).
__global__ void k_border_set_diag(int n, int m, const int *__restrict__ pos,
                                  const uint8_t *__restrict__ mask, double lamb, double delta,
                                  double *__restrict__ band, int ldb, int Nb, double *__restrict__ Dd,
                                  int k, int kp) {
  b_border_set_diag(n, m, pos, mask, lamb, delta, band, ldb, Nb, Dd, k, kp);
}

void sp_border_assemble(hipStream_t s, const SparseDev &sp, int n, int m, const uint8_t *mask,
                        double lamb, double delta) {
  const size_t total = (size_t)(sp.bor.Nb + 1) * sp.pat.ldb + (size_t)sp.bor.Nb * sp.bor.bkp + (size_t)sp.bor.bkp * sp.bor.bkp;
  (void)hipMemsetAsync(sp.pat.band, 0, total * sizeof(double), s);
  hipLaunchKernelGGL(k_border_set_diag, g1(n + m + sp.bor.bkp - sp.bor.bk), dim3(256), 0, s, n, m, sp.pat.pos, mask, lamb,
                     delta, sp.pat.band, sp.pat.ldb, sp.bor.Nb, sp.bor.bDd, sp.bor.bk, sp.bor.bkp);
  sp_launch_scatter(s, sp, mask);
}

// ---------------------------------------------------------------- Y = inv(B) C, 8 x 8 blocks
// The recurrences of k_bcr_level / k_bcr_back (pgf_sparse.hip) with an 8 x R panel per block in place
// of the 8-vector f (R = kp).  The panel has C's own layout -- row-major, R doubles per row -- so
// that the 8 x R rows of a block are one contiguous, coalesced piece of memory; it starts as a copy
// of C and ends as Y.  One level per launch, everything in place: a kept block only reads the two
// blocks eliminated at its level, which no workgroup of that launch writes.  The work arrays (D, L,
// U, inverses) are those of the single-right-hand-side reduction, which runs strictly before or
// after on the same stream.  One wavefront per block, lane <-> (row, col).
__global__ __launch_bounds__(64) void k_mbcr_extract(const double *__restrict__ band, int ldb, int bw,
                                                     const double *__restrict__ C, int R, int N, int nb,
                                                     double *__restrict__ D, double *__restrict__ L,
                                                     double *__restrict__ U, double *__restrict__ P) {
  b_mbcr_extract(band, ldb, bw, C, R, N, nb, D, L, U, P);
}

__global__ __launch_bounds__(64) void k_mbcr_level(double *D, double *L, double *U,
                                                   double *__restrict__ Dinv, double *P, int R, int nb,
                                                   int s) {
  b_mbcr_level(D, L, U, Dinv, P, R, nb, s);
}

__global__ __launch_bounds__(64) void k_mbcr_back(const double *__restrict__ D, double *__restrict__ Dinv,
                                                  const double *__restrict__ L,
                                                  const double *__restrict__ U, double *__restrict__ P,
                                                  int R, int nb, int s) {
  b_mbcr_back(D, Dinv, L, U, P, R, nb, s);
}

static void mbcr_solve(hipStream_t s, const SparseDev &sp) {
  const int N = sp.bor.Nb, R = sp.bor.bkp, nb = (N + 7) / 8;
  hipLaunchKernelGGL(k_mbcr_extract, dim3(nb), dim3(64), 0, s, sp.pat.band, sp.pat.ldb, sp.pat.bw, sp.bor.bC, R, N, nb, sp.blk.bD,
                     sp.blk.bL, sp.blk.bU, sp.bor.bY);
  int st = 1;
  for (; st < nb; st *= 2) {
    const int nk = (nb + 2 * st - 1) / (2 * st);  // kept: 0, 2 st, ...
    hipLaunchKernelGGL(k_mbcr_level, dim3(nk), dim3(64), 0, s, sp.blk.bD, sp.blk.bL, sp.blk.bU, sp.blk.bDinv, sp.bor.bY, R, nb, st);
  }
  hipLaunchKernelGGL(k_mbcr_back, dim3(1), dim3(64), 0, s, sp.blk.bD, sp.blk.bDinv, sp.blk.bL, sp.blk.bU, sp.bor.bY, R, nb, 0);
  for (st /= 2; st >= 1; st /= 2) {
    const int ne = (nb - st + 2 * st - 1) / (2 * st);  // eliminated: st, 3 st, ...
    hipLaunchKernelGGL(k_mbcr_back, dim3(ne), dim3(64), 0, s, sp.blk.bD, sp.blk.bDinv, sp.blk.bL, sp.blk.bU, sp.bor.bY, R, nb, st);
  }
}

// ---------------------------------------------------------------- Y by repeated single solves
// column j of C into the right-hand side / the solution into column j of Y
__global__ void k_border_col(int N, int kp, int j, const double *__restrict__ from, double *__restrict__ to,
                             int put) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  if (put)
    to[(int64_t)i * kp + j] = from[i];
  else
    to[i] = from[(int64_t)i * kp + j];
}

// ---------------------------------------------------------------- tall-skinny products, S, guard
__global__ __launch_bounds__(256) void k_border_gram(const double *__restrict__ C,
                                                     const double *__restrict__ Y, int Nb, int kp,
                                                     double *__restrict__ part) {
  b_border_gram(C, Y, Nb, kp, part);
}

__global__ __launch_bounds__(256) void k_border_ctv(const double *__restrict__ C,
                                                    const double *__restrict__ v, int Nb, int kp,
                                                    double *__restrict__ partv) {
  b_border_ctv(C, v, Nb, kp, partv);
}

__global__ __launch_bounds__(256) void k_border_factor_S(const double *__restrict__ Dd,
                                                         const double *__restrict__ part, int nchunk,
                                                         int kp, double *__restrict__ Sfac,
                                                         int *__restrict__ sflags) {
  b_border_factor_S(Dd, part, nchunk, kp, Sfac, sflags);
}

__global__ __launch_bounds__(64) void k_border_small_solve(const double *__restrict__ Sfac, int k, int kp,
                                                           const double *__restrict__ rb,
                                                           const double *__restrict__ partv, int nchunk,
                                                           const int *__restrict__ sflags,
                                                           double *__restrict__ z, double *__restrict__ xb,
                                                           int *__restrict__ flags) {
  b_border_small_solve(Sfac, k, kp, rb, partv, nchunk, sflags, z, xb, flags);
}

__global__ __launch_bounds__(256) void k_border_update(int Nb, int k, int kp, const double *__restrict__ Y,
                                                       const double *__restrict__ z,
                                                       double *__restrict__ x) {
  b_border_update(Nb, k, kp, Y, z, x);
}

__global__ __launch_bounds__(256) void k_border_residual(
    const double *__restrict__ band, int ldb, int bw, int Nb, int k, int kp, const double *__restrict__ C,
    const double *__restrict__ Dd, const double *__restrict__ partv, int nchunk,
    const double *__restrict__ x, const double *__restrict__ rhs0, double *__restrict__ r,
    double *__restrict__ rsmax, const int *__restrict__ flags, int nred) {
  b_border_residual(band, ldb, bw, Nb, k, kp, C, Dd, partv, nchunk, x, rhs0, r, rsmax, flags, nred);
}

// ---------------------------------------------------------------- phases
// Wide remainder (B = 16, 32, 64) with the factor / solve split on: B is factorised ONCE per
// assembled matrix (the factor-only KEEP reduction of pgf_band_wide.hip), and every solve with B --
// the kp columns of Y as one panel, v of each solve phase -- runs against the kept factors.
static bool wide_kept(const SparseDev &sp) { return sp.blk.B > 8 && sp.blk.split && sp.blk.bMr; }

// The solve phase of the wide band leaves the pivot flags alone, and k_border_small_solve ADDS
// those of S to them: the flags of B are parked in bsflags[2, 4) by the factor phase (save) and
// put back in front of every solve phase (flags[2], flags[3] cleared as the extraction does).
__global__ void k_border_bflags(int *__restrict__ flags, int *__restrict__ sflags, int save) {
  if (threadIdx.x != 0) return;
  if (save) {
    sflags[2] = flags[0];
    sflags[3] = flags[1];
  } else {
    flags[0] = sflags[2];
    flags[1] = sflags[3];
    flags[2] = 0;
    flags[3] = 0;
  }
}

// Wide remainder under wide_kept, first half of the factor phase (both border sizes): the
// factor-only KEEP reduction of B, its flags parked, Y = inv(B) C as one panel (kp <= 64, or 64-column
// slices of the same launches beyond) or, PGF_BORDER_MULTI=0, column by column.
void sp_border_wide_Y(hipStream_t s, const SparseDev &sp, int *flags) {
  static const bool multi = env_on("PGF_BORDER_MULTI");
  const int Nb = sp.bor.Nb, k = sp.bor.bk, kp = sp.bor.bkp;
  sp_launch_bw_factor(s, sp, Nb, flags);  // (reads sp.vec.brhs, writes none of it)
  hipLaunchKernelGGL(k_border_bflags, dim3(1), dim3(64), 0, s, flags, sp.bor.bsflags, 1);
  const int nbB = (Nb + sp.blk.B - 1) / sp.blk.B * sp.blk.B;  // Y in whole B-row blocks, the padding rows zero
  if (multi) {
    (void)hipMemcpyAsync(sp.bor.bY, sp.bor.bC, (size_t)Nb * kp * sizeof(double), hipMemcpyDeviceToDevice, s);
    if (nbB > Nb)
      (void)hipMemsetAsync(sp.bor.bY + (size_t)Nb * kp, 0, (size_t)(nbB - Nb) * kp * sizeof(double), s);
    sp_launch_bw_panel_solve(s, sp, Nb, sp.bor.bY, kp);
  } else {
    (void)hipMemcpyAsync(sp.vec.bres, sp.vec.brhs, (size_t)(Nb + k) * sizeof(double), hipMemcpyDeviceToDevice, s);
    (void)hipMemsetAsync(sp.bor.bY, 0, (size_t)nbB * kp * sizeof(double), s);
    for (int j = 0; j < k; ++j) {
      hipLaunchKernelGGL(k_border_col, g1(Nb), dim3(256), 0, s, Nb, kp, j, sp.bor.bC, sp.vec.brhs, 0);
      sp_launch_bw_backsolve(s, sp, Nb, flags, /*guard=*/false);
      hipLaunchKernelGGL(k_border_col, g1(Nb), dim3(256), 0, s, Nb, kp, j, sp.vec.brhs, sp.bor.bY, 1);
    }
    (void)hipMemcpyAsync(sp.vec.brhs, sp.vec.bres, (size_t)(Nb + k) * sizeof(double), hipMemcpyDeviceToDevice, s);
  }
}

// the small border's Gram launch alone (tools: timed against the MFMA kernel at kp = 64)
void sp_border_gram_fma(hipStream_t s, const SparseDev &sp) {
  hipLaunchKernelGGL(k_border_gram, dim3(sp.bor.bnchunk), dim3(256), 0, s, sp.bor.bC, sp.bor.bY, sp.bor.Nb, sp.bor.bkp, sp.bor.bpart);
}

// ... and of the solve phase: v = inv(B) ra against the kept factors; flags <- pivots of B as kept
void sp_border_wide_v(hipStream_t s, const SparseDev &sp, int *flags) {
  hipLaunchKernelGGL(k_border_bflags, dim3(1), dim3(64), 0, s, flags, sp.bor.bsflags, 0);
  sp_launch_bw_backsolve(s, sp, sp.bor.Nb, flags, /*guard=*/false);
}

void sp_border_factor(hipStream_t s, const SparseDev &sp, int *flags) {
  const int Nb = sp.bor.Nb, k = sp.bor.bk, kp = sp.bor.bkp;
  ++sp.cnt.stat_bfactor;
  if (sp_border_large(sp)) {  // 65 .. 1024 border nodes: pgf_border_large.hip
    sp_borderL_factor(s, sp, flags);
    return;
  }
  // PGF_BORDER_MULTI=0: Y column by column through the single-right-hand-side solves at every B:
  // slower, and an independent check of the panel kernels
  static const bool multi = env_on("PGF_BORDER_MULTI");
  if (sp.blk.B == 8 && multi) {
    mbcr_solve(s, sp);
  } else if (wide_kept(sp)) {
    sp_border_wide_Y(s, sp, flags);
  } else {
    // the band solves work in sp.vec.brhs: whatever right-hand side waits there moves out of the way
    (void)hipMemcpyAsync(sp.vec.bres, sp.vec.brhs, (size_t)(Nb + k) * sizeof(double), hipMemcpyDeviceToDevice, s);
    (void)hipMemsetAsync(sp.bor.bY, 0, (size_t)Nb * kp * sizeof(double), s);
    for (int j = 0; j < k; ++j) {
      hipLaunchKernelGGL(k_border_col, g1(Nb), dim3(256), 0, s, Nb, kp, j, sp.bor.bC, sp.vec.brhs, 0);
      band_solve(s, sp, Nb, flags);
      hipLaunchKernelGGL(k_border_col, g1(Nb), dim3(256), 0, s, Nb, kp, j, sp.vec.brhs, sp.bor.bY, 1);
    }
    (void)hipMemcpyAsync(sp.vec.brhs, sp.vec.bres, (size_t)(Nb + k) * sizeof(double), hipMemcpyDeviceToDevice, s);
  }
  hipLaunchKernelGGL(k_border_gram, dim3(sp.bor.bnchunk), dim3(256), 0, s, sp.bor.bC, sp.bor.bY, Nb, kp, sp.bor.bpart);
  hipLaunchKernelGGL(k_border_factor_S, dim3(1), dim3(256), 0, s, sp.bor.bDd, sp.bor.bpart, sp.bor.bnchunk, kp, sp.bor.bS,
                     sp.bor.bsflags);
}

void sp_border_residual(hipStream_t s, const SparseDev &sp, const int *flags) {
  if (sp_border_large(sp)) {
    sp_borderL_residual(s, sp, flags);
    return;
  }
  hipLaunchKernelGGL(k_border_ctv, dim3(sp.bor.bnchunk), dim3(256), 0, s, sp.bor.bC, sp.vec.brhs, sp.bor.Nb, sp.bor.bkp, sp.bor.bpartv);
  hipLaunchKernelGGL(k_border_residual, dim3(sp.vec.nred), dim3(256), 0, s, sp.pat.band, sp.pat.ldb, sp.pat.bw, sp.bor.Nb, sp.bor.bk,
                     sp.bor.bkp, sp.bor.bC, sp.bor.bDd, sp.bor.bpartv, sp.bor.bnchunk, sp.vec.brhs, sp.vec.brhs0, sp.vec.bres, sp.vec.bred, flags,
                     sp.vec.nred);
}

void sp_border_solve(hipStream_t s, const SparseDev &sp, int *flags, bool guard) {
  const int Nb = sp.bor.Nb, k = sp.bor.bk, kp = sp.bor.bkp;
  ++sp.cnt.stat_bsolve;
  if (sp_border_large(sp)) {
    sp_borderL_solve(s, sp, flags, guard);
    return;
  }
  // (the band solve writes whole blocks: the border entries behind Nb do not survive it)
  (void)hipMemcpyAsync(sp.bor.brb, sp.vec.brhs + Nb, (size_t)k * sizeof(double), hipMemcpyDeviceToDevice, s);
  if (guard)
    (void)hipMemcpyAsync(sp.vec.brhs0, sp.vec.brhs, (size_t)(Nb + k) * sizeof(double), hipMemcpyDeviceToDevice, s);
  if (wide_kept(sp)) {
    sp_border_wide_v(s, sp, flags);
  } else {
    band_solve(s, sp, Nb, flags);  // v = inv(B) ra; flags <- pivots of B
  }
  hipLaunchKernelGGL(k_border_ctv, dim3(sp.bor.bnchunk), dim3(256), 0, s, sp.bor.bC, sp.vec.brhs, Nb, kp, sp.bor.bpartv);
  hipLaunchKernelGGL(k_border_small_solve, dim3(1), dim3(64), 0, s, sp.bor.bS, k, kp, sp.bor.brb, sp.bor.bpartv, sp.bor.bnchunk,
                     sp.bor.bsflags, sp.bor.bz, sp.vec.brhs + Nb, flags);
  hipLaunchKernelGGL(k_border_update, g1(Nb), dim3(256), 0, s, Nb, k, kp, sp.bor.bY, sp.bor.bz, sp.vec.brhs);
  if (guard) sp_border_residual(s, sp, flags);
}

// ================================================================= bordered band in a device batch
// The kernels above with a batch dimension, for the narrow route (block size 8) and, with the band
// part handed to pgf_band_wide.hip, for a wide remainder (block size 16, 32, 64; "wide remainder"
// below).  Every kernel here is the twin of a kernel of one handle: instance = blockIdx.y, its pointers from the BandInst table, the pattern arrays from instance 0 and the sizes
// (bk, bkp, Nb, bnchunk -- equal across the instances by construction) through BandShape, and then
// the SAME device function from pgf_border_dev.h with the same arguments in the same order: the
// batch computes, instance by instance, the bits the single handle computes on its panel route
// (PGF_BORDER_MULTI=0, the column-by-column cross-check, stays a single-handle switch).
//
// Phases per instance, decided on the device.  Factor phase -- clear, diagonal, scatters, the panel
// reduction Y = inv(B) C, C' Y, S and its factor: only where ctl[0] != 0 (kb_mask_adopt: the matrix
// changed, or the last factor phase met a bad pivot), which is where the single handle finds
// !fac.factored.  Solve phase: every instance that is not frozen, every step.  The reduction of B on
// the right-hand side in between is the plain band batch's (bandb_launch_solve over Nb rows).
//
// What the single handle does with memsets and copies is ONE twin kernel each here (B copies would
// be B launches): kbd_border_zero, kbd_border_save.
//
// Wide remainder: the handle's panel route under wide_kept (above).  Factor phase: assembly
// as above, the factor-only KEEP reduction of B (bandb_launch_wide_factor), its pivot flags parked in
// bsflags[2, 4) (kbd_border_bflags_save), Y <- C in whole B-row blocks (kbd_border_ycopy), Y <-
// inv(B) Y as one panel solve against the kept factors (bandb_launch_wide_panel), gram, factor_S:
// 11 + 4 L launches for L = ceil(log2(ceil(Nb / B))) levels.  Solve phase: save with the flags of B
// put back (kbd_border_save_wide), v = inv(B) r_a against the kept factors
// (bandb_launch_wide_kept_solve: load, L forward, x_0, L backward), then ctv, small_solve, update,
// ctv, residual as on the narrow route: 8 + 2 L launches.  The copies and the flag kernels are
// integer or plain moves: the contraction rules of this file do not touch them; everything that
// multiplies on the band lives in pgf_band_wide.hip beside the kernels it mirrors.
//
// Grid shape of the one-workgroup kernels: (1, B).  kbd_border_factor_S holds at most 32.5 KB of LDS
// (kp = 64), kbd_border_small_solve the same: several share a CU.

// factor phase: the instances that assemble this step (a frozen instance has ctl[0] == 0)
#define FINST(I)                        \
  const BandInst &I = tab[blockIdx.y];  \
  if (I.ctl[0] == 0) return
// solve phase: every instance that takes the step
#define SINST(I)                        \
  const BandInst &I = tab[blockIdx.y];  \
  if (I.ctl[3]) return /* frozen: sits this step out */

// ---------------------------------------------------------------- assembly
// band, C and D: (Nb + 1) ldb + Nb kp + kp kp doubles, one array (the single handle's memset)
__global__ void kbd_border_zero(const BandInst *__restrict__ tab, BandShape sh) {
  FINST(I);
  const int64_t total = (int64_t)(sh.Nb + 1) * sh.ldb + (int64_t)sh.Nb * sh.bkp + (int64_t)sh.bkp * sh.bkp;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < total) I.band[p] = 0.0;
}

__global__ void kbd_border_set_diag(const BandInst *__restrict__ tab, BandShape sh) {
  FINST(I);
  b_border_set_diag(sh.n, sh.m, sh.pos, I.mask, I.ps[BPS_LAMB], I.ps[BPS_DELTA], I.band, sh.ldb, sh.Nb, I.bDd,
                    sh.bk, sh.bkp);
}

// (the slots point into the band or into the border store behind it)
__global__ void kbd_border_scatter_H(const BandInst *__restrict__ tab, BandShape sh) {
  FINST(I);
  b_band_scatter_H(sh.nnzH, sh.Hrow, sh.Hcol, I.Hval, sh.Hslot, I.mask, I.band);
}

__global__ void kbd_border_scatter_J(const BandInst *__restrict__ tab, BandShape sh) {
  FINST(I);
  b_band_scatter_J(sh.nnzJ, sh.Jcol, I.Jval, sh.Jslot, I.mask, I.band);
}

// ---------------------------------------------------------------- Y = inv(B) C
// (the work arrays are the first block set of the instance's reduction, as on the handle)
__global__ __launch_bounds__(64) void kbd_mbcr_extract(const BandInst *__restrict__ tab, BandShape sh, int nb) {
  FINST(I);
  b_mbcr_extract(I.band, sh.ldb, sh.bw, I.bC, sh.bkp, sh.Nb, nb, I.bD, I.bL, I.bU, I.bY);
}

__global__ __launch_bounds__(64) void kbd_mbcr_level(const BandInst *__restrict__ tab, BandShape sh, int nb,
                                                     int s) {
  FINST(I);
  b_mbcr_level(I.bD, I.bL, I.bU, I.bDinv, I.bY, sh.bkp, nb, s);
}

__global__ __launch_bounds__(64) void kbd_mbcr_back(const BandInst *__restrict__ tab, BandShape sh, int nb,
                                                    int s) {
  FINST(I);
  b_mbcr_back(I.bD, I.bDinv, I.bL, I.bU, I.bY, sh.bkp, nb, s);
}

// ---------------------------------------------------------------- wide remainder (block 16, 32, 64)
// The pivot flags of B, parked behind those of S once the factor-only reduction has run
// (k_border_bflags, save): integers only.
__global__ void kbd_border_bflags_save(const BandInst *__restrict__ tab) {
  FINST(I);
  if (threadIdx.x != 0) return;
  I.bsflags[2] = I.flags[0];
  I.bsflags[3] = I.flags[1];
}

// Y <- C over the Nb band rows, the padding rows up to whole B-row blocks zero (the handle's copy
// and memset in front of its panel solve); rows: ceil(Nb / B) B
__global__ void kbd_border_ycopy(const BandInst *__restrict__ tab, BandShape sh, int rows) {
  FINST(I);
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (int64_t)rows * sh.bkp) return;
  I.bY[p] = p < (int64_t)sh.Nb * sh.bkp ? I.bC[p] : 0.0;
}

// ---------------------------------------------------------------- S and its factor
__global__ __launch_bounds__(256) void kbd_border_gram(const BandInst *__restrict__ tab, BandShape sh) {
  FINST(I);
  b_border_gram(I.bC, I.bY, sh.Nb, sh.bkp, I.bpart);
}

__global__ __launch_bounds__(256) void kbd_border_factor_S(const BandInst *__restrict__ tab, BandShape sh) {
  FINST(I);
  if (threadIdx.x == 0) I.bcnt[0] += 1;  // (this instance's one workgroup: nothing else writes it)
  b_border_factor_S(I.bDd, I.bpart, sh.bnchunk, sh.bkp, I.bS, I.bsflags);
}

// ---------------------------------------------------------------- solve phase
// brb <- brhs[Nb, Nb + k) (the band solve writes whole blocks: the border entries do not survive
// it) and the guard's brhs0 <- brhs over all Nb + k entries, in one launch
__global__ void kbd_border_save(const BandInst *__restrict__ tab, BandShape sh) {
  SINST(I);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= sh.Nb + sh.bk) return;
  const double v = I.brhs[i];
  I.brhs0[i] = v;
  if (i >= sh.Nb) I.brb[i - sh.Nb] = v;
}

// the same in front of the wide solve phase, which leaves the pivot flags alone: those of B come
// back from bsflags[2, 4) and flags[2], flags[3] are cleared (k_border_bflags, restore)
__global__ void kbd_border_save_wide(const BandInst *__restrict__ tab, BandShape sh) {
  SINST(I);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    I.flags[0] = I.bsflags[2];
    I.flags[1] = I.bsflags[3];
    I.flags[2] = 0;
    I.flags[3] = 0;
  }
  if (i >= sh.Nb + sh.bk) return;
  const double v = I.brhs[i];
  I.brhs0[i] = v;
  if (i >= sh.Nb) I.brb[i - sh.Nb] = v;
}

// Both with the guard off (sp_border_solve(guard = false): a refinement round inside the
// device-resident controller's loop, whose brhs0 still holds the step's right-hand side): brb alone
__global__ void kbd_border_save_ng(const BandInst *__restrict__ tab, BandShape sh) {
  SINST(I);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < sh.bk) I.brb[i] = I.brhs[sh.Nb + i];
}

__global__ void kbd_border_save_wide_ng(const BandInst *__restrict__ tab, BandShape sh) {
  SINST(I);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i == 0) {
    I.flags[0] = I.bsflags[2];
    I.flags[1] = I.bsflags[3];
    I.flags[2] = 0;
    I.flags[3] = 0;
  }
  if (i < sh.bk) I.brb[i] = I.brhs[sh.Nb + i];
}

__global__ __launch_bounds__(256) void kbd_border_ctv(const BandInst *__restrict__ tab, BandShape sh) {
  SINST(I);
  b_border_ctv(I.bC, I.brhs, sh.Nb, sh.bkp, I.bpartv);
}

__global__ __launch_bounds__(64) void kbd_border_small_solve(const BandInst *__restrict__ tab, BandShape sh) {
  SINST(I);
  if (threadIdx.x == 0) I.bcnt[1] += 1;
  b_border_small_solve(I.bS, sh.bk, sh.bkp, I.brb, I.bpartv, sh.bnchunk, I.bsflags, I.bz, I.brhs + sh.Nb,
                       I.flags);
}

__global__ __launch_bounds__(256) void kbd_border_update(const BandInst *__restrict__ tab, BandShape sh) {
  SINST(I);
  b_border_update(sh.Nb, sh.bk, sh.bkp, I.bY, I.bz, I.brhs);
}

__global__ __launch_bounds__(256) void kbd_border_residual(const BandInst *__restrict__ tab, BandShape sh) {
  SINST(I);
  b_border_residual(I.band, sh.ldb, sh.bw, sh.Nb, sh.bk, sh.bkp, I.bC, I.bDd, I.bpartv, sh.bnchunk, I.brhs,
                    I.brhs0, I.bres, I.stat, I.flags, sh.nred);
}

// ---------------------------------------------------------------- launch wrappers
static inline dim3 gy(int64_t cnt, int per, int B) { return dim3((unsigned)((cnt + per - 1) / per), B); }

// sp_border_assemble and the panel route of sp_border_factor (mbcr_solve, gram, factor_S)
void borderb_launch_factor(hipStream_t s, const BandInst *tab, int B, const BandShape &sh) {
  const unsigned Bu = (unsigned)B;
  const int64_t total = (int64_t)(sh.Nb + 1) * sh.ldb + (int64_t)sh.Nb * sh.bkp + (int64_t)sh.bkp * sh.bkp;
  hipLaunchKernelGGL(kbd_border_zero, gy(total, 256, B), dim3(256), 0, s, tab, sh);
  hipLaunchKernelGGL(kbd_border_set_diag, gy(sh.N + sh.bkp - sh.bk, 256, B), dim3(256), 0, s, tab, sh);
  if (sh.nnzH) hipLaunchKernelGGL(kbd_border_scatter_H, gy(sh.nnzH, 256, B), dim3(256), 0, s, tab, sh);
  if (sh.nnzJ) hipLaunchKernelGGL(kbd_border_scatter_J, gy(sh.nnzJ, 256, B), dim3(256), 0, s, tab, sh);
  if (sh.B > 8) {
    // Wide remainder, the panel route of sp_border_factor under wide_kept: B factorised once by the
    // factor-only KEEP reduction, its flags parked, Y = inv(B) C as one panel solve against the
    // kept factors (pgf_band_wide.hip), all for the instances with ctl[0] != 0.
    BandShape shB = sh;
    shB.N = sh.Nb;
    shB.nb = (sh.Nb + sh.B - 1) / sh.B;
    bandb_launch_wide_factor(s, tab, B, shB);
    hipLaunchKernelGGL(kbd_border_bflags_save, dim3(1, Bu), dim3(64), 0, s, tab);
    const int rows = shB.nb * sh.B;
    hipLaunchKernelGGL(kbd_border_ycopy, gy((int64_t)rows * sh.bkp, 256, B), dim3(256), 0, s, tab, sh, rows);
    bandb_launch_wide_panel(s, tab, B, shB);
    hipLaunchKernelGGL(kbd_border_gram, dim3(sh.bnchunk, Bu), dim3(256), 0, s, tab, sh);
    hipLaunchKernelGGL(kbd_border_factor_S, dim3(1, Bu), dim3(256), 0, s, tab, sh);
    return;
  }
  const int nb = (sh.Nb + 7) / 8;
  hipLaunchKernelGGL(kbd_mbcr_extract, dim3(nb, Bu), dim3(64), 0, s, tab, sh, nb);
  int st = 1;
  for (; st < nb; st *= 2) {
    const int nk = (nb + 2 * st - 1) / (2 * st);  // kept: 0, 2 st, ...
    hipLaunchKernelGGL(kbd_mbcr_level, dim3(nk, Bu), dim3(64), 0, s, tab, sh, nb, st);
  }
  hipLaunchKernelGGL(kbd_mbcr_back, dim3(1, Bu), dim3(64), 0, s, tab, sh, nb, 0);
  for (st /= 2; st >= 1; st /= 2) {
    const int ne = (nb - st + 2 * st - 1) / (2 * st);  // eliminated: st, 3 st, ...
    hipLaunchKernelGGL(kbd_mbcr_back, dim3(ne, Bu), dim3(64), 0, s, tab, sh, nb, st);
  }
  hipLaunchKernelGGL(kbd_border_gram, dim3(sh.bnchunk, Bu), dim3(256), 0, s, tab, sh);
  hipLaunchKernelGGL(kbd_border_factor_S, dim3(1, Bu), dim3(256), 0, s, tab, sh);
}

// sp_border_solve, with the guard on or (a refinement round) off
void borderb_launch_solve(hipStream_t s, const BandInst *tab, int B, const BandShape &sh, bool guard) {
  const unsigned Bu = (unsigned)B;
  BandShape shB = sh;  // v = inv(B) ra over the Nb band rows
  shB.N = sh.Nb;
  if (sh.B > 8) {  // against the factors the instance kept, with the flags of B as parked
    if (guard)
      hipLaunchKernelGGL(kbd_border_save_wide, gy(sh.Nb + sh.bk, 256, B), dim3(256), 0, s, tab, sh);
    else
      hipLaunchKernelGGL(kbd_border_save_wide_ng, gy(sh.bk, 64, B), dim3(64), 0, s, tab, sh);
    shB.nb = (sh.Nb + sh.B - 1) / sh.B;
    bandb_launch_wide_kept_solve(s, tab, B, shB);
  } else {  // the plain band's reduction
    if (guard)
      hipLaunchKernelGGL(kbd_border_save, gy(sh.Nb + sh.bk, 256, B), dim3(256), 0, s, tab, sh);
    else
      hipLaunchKernelGGL(kbd_border_save_ng, gy(sh.bk, 64, B), dim3(64), 0, s, tab, sh);
    shB.nb = (sh.Nb + 7) / 8;
    bandb_launch_solve(s, tab, B, shB, /*residual=*/false, /*save_rhs=*/guard);
  }
  hipLaunchKernelGGL(kbd_border_ctv, dim3(sh.bnchunk, Bu), dim3(256), 0, s, tab, sh);
  hipLaunchKernelGGL(kbd_border_small_solve, dim3(1, Bu), dim3(64), 0, s, tab, sh);
  hipLaunchKernelGGL(kbd_border_update, gy(sh.Nb, 256, B), dim3(256), 0, s, tab, sh);
  if (guard) borderb_launch_residual(s, tab, B, sh);
}

// sp_border_residual
void borderb_launch_residual(hipStream_t s, const BandInst *tab, int B, const BandShape &sh) {
  const unsigned Bu = (unsigned)B;
  hipLaunchKernelGGL(kbd_border_ctv, dim3(sh.bnchunk, Bu), dim3(256), 0, s, tab, sh);
  hipLaunchKernelGGL(kbd_border_residual, dim3(sh.nred, Bu), dim3(256), 0, s, tab, sh);
}
