// Bordered band in a device batch: the kernels of pgf_border.hip with a batch dimension, for the
// narrow route (block size 8) and, with the band part handed to pgf_band_wide_batch.hip, for a wide
// remainder (block size 16, 32, 64; "wide remainder" below).  Every kernel here is the twin of a kernel of one handle: instance =
// blockIdx.y, its pointers from the BandInst table, the pattern arrays from instance 0 and the sizes
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
// Wide remainder: the handle's panel route under wide_kept (pgf_border.hip).  Factor phase: assembly
// as above, the factor-only KEEP reduction of B (bandb_launch_wide_factor), its pivot flags parked in
// bsflags[2, 4) (kbd_border_bflags_save), Y <- C in whole B-row blocks (kbd_border_ycopy), Y <-
// inv(B) Y as one panel solve against the kept factors (bandb_launch_wide_panel), gram, factor_S:
// 11 + 4 L launches for L = ceil(log2(ceil(Nb / B))) levels.  Solve phase: save with the flags of B
// put back (kbd_border_save_wide), v = inv(B) r_a against the kept factors
// (bandb_launch_wide_kept_solve: load, L forward, x_0, L backward), then ctv, small_solve, update,
// ctv, residual as on the narrow route: 8 + 2 L launches.  The copies and the flag kernels are
// integer or plain moves: the contraction rules of this file do not touch them; everything that
// multiplies on the band lives in pgf_band_wide_batch.hip beside the kernels it mirrors.
//
// Grid shape of the one-workgroup kernels: (1, B).  kbd_border_factor_S holds at most 32.5 KB of LDS
// (kp = 64), kbd_border_small_solve the same: several share a CU.
//
// Compiled with -ffp-contract=off like pgf_border.hip (explicit fma() only).
#include "pgf_band_dev.h"
#include "pgf_border_dev.h"
#include "pgf_internal.h"
#include "pgf_sparse.h"

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
    // kept factors (pgf_band_wide_batch.hip), all for the instances with ctl[0] != 0.
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

// sp_border_solve with the guard on
void borderb_launch_solve(hipStream_t s, const BandInst *tab, int B, const BandShape &sh) {
  const unsigned Bu = (unsigned)B;
  BandShape shB = sh;  // v = inv(B) ra over the Nb band rows
  shB.N = sh.Nb;
  if (sh.B > 8) {  // against the factors the instance kept, with the flags of B as parked
    hipLaunchKernelGGL(kbd_border_save_wide, gy(sh.Nb + sh.bk, 256, B), dim3(256), 0, s, tab, sh);
    shB.nb = (sh.Nb + sh.B - 1) / sh.B;
    bandb_launch_wide_kept_solve(s, tab, B, shB);
  } else {  // the plain band's reduction
    hipLaunchKernelGGL(kbd_border_save, gy(sh.Nb + sh.bk, 256, B), dim3(256), 0, s, tab, sh);
    shB.nb = (sh.Nb + 7) / 8;
    bandb_launch_solve(s, tab, B, shB, /*residual=*/false);
  }
  hipLaunchKernelGGL(kbd_border_ctv, dim3(sh.bnchunk, Bu), dim3(256), 0, s, tab, sh);
  hipLaunchKernelGGL(kbd_border_small_solve, dim3(1, Bu), dim3(64), 0, s, tab, sh);
  hipLaunchKernelGGL(kbd_border_update, gy(sh.Nb, 256, B), dim3(256), 0, s, tab, sh);
  hipLaunchKernelGGL(kbd_border_ctv, dim3(sh.bnchunk, Bu), dim3(256), 0, s, tab, sh);
  hipLaunchKernelGGL(kbd_border_residual, dim3(sh.nred, Bu), dim3(256), 0, s, tab, sh);
}
