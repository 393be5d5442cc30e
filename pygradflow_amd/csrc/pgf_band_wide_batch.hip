// Banded device batch on the wide route: the kernels of the wide block cyclic reduction
// (pgf_band_wide.hip; B x B blocks, B in {16, 32, 64}) with a batch dimension.  Every kernel here is
// the twin of a kernel of one handle: instance = blockIdx.y, its pointers from the BandInst table,
// the shape from BandShape, and then the SAME device function from pgf_band_wide_dev.h with the same
// arguments in the same order -- the batch computes, instance by instance, the bits the single handle
// computes.  Grid shapes are those of one handle with the instances in grid.y; the one-workgroup
// launches (last block, x_0) are (1, instances).  LDS per workgroup: one B x (B + 1) block, 33 KB at
// B = 64, so four workgroups share a CU's 160 KB.
//
// Per-instance phase, chosen on the device inside ONE launch sequence.  With the factor / solve split
// on (BandShape::split), ctl[0] == 0 for an instance that is not frozen means: its matrix did not
// change and the last reduction of its band was clean (kbb_band_step_update sets ctl[1], kb_mask_adopt
// and kb_advance clear it) -- the situation in which one handle runs the solve phase against its kept
// factors (SparseDev::kept == 2).  So every twin branches on ctl[0]:
//
//   twin of    ctl[0] != 0, or split off            ctl[0] == 0 and split on
//   extract    whole extraction                     right-hand side part only (k_bw_load's work)
//   invert     invert                               return
//   reduce     k_bw_reduce<B, KEEP = split, true>   k_bw_fwd (same grid: the kept blocks of the level)
//   last       k_bw_last                            k_bw_x0
//   back, residual: the same in both phases
//
// The solve phase returns the bits of the fused reduction (pgf_band_wide.hip), so either branch
// agrees with whatever the single handle did.  A frozen instance (ctl[3]) returns at once everywhere.
// Thread 0 of the extraction's block 0 counts the instance's reductions and solve phases (wcnt).
//
// A bordered batch on the wide route (pgf_border_batch.hip) needs the two phases apart, in one step
// and for different sets of instances, while ctl[0] stays set: the factor-only reduction of B where
// ctl[0] != 0, later the solve against the kept factors for every live instance.  The twins that
// branch therefore take the phase as a template argument (BW_BY_CTL / BW_FACTOR / BW_SOLVE below);
// the unbordered batch launches the BW_BY_CTL instantiations, whose code is what it was.  The panel
// solve Y <- inv(B) Y of the factor phase has its own twins, kbw_fwd_panel / kbw_back_panel.
//
// Compiled WITHOUT -ffp-contract=off, like pgf_band_wide.hip: the twins must see the contraction
// rules of the kernels they mirror.
#include "pgf_band_wide_dev.h"
#include "pgf_internal.h"
#include "pgf_sparse.h"

#define INST(I)                        \
  const BandInst &I = tab[blockIdx.y]; \
  if (I.ctl[3]) return /* frozen: sits this step out */

// Phase selector, a template argument of the twins that branch: which of the two phases an instance
// runs is read from ctl[0] (BW_BY_CTL: the unbordered wide batch, one launch sequence for both), or
// fixed by the caller -- the bordered wide route (pgf_border_batch.hip) runs the factor-only KEEP
// reduction of B for the instances with ctl[0] != 0 (BW_FACTOR) and, later in the SAME step, while
// ctl[0] is still set, the solve phase against the kept factors for every live instance (BW_SOLVE).
// The BW_BY_CTL instantiations are the kernels the unbordered batch has always launched.
enum { BW_BY_CTL = 0, BW_FACTOR = 1, BW_SOLVE = 2 };

// true: this instance reduces in this step; false: it solves against the factors it kept
__device__ __forceinline__ bool bw_reduces(const BandInst &I, const BandShape &sh) {
  return !sh.split || I.ctl[0] != 0;
}

// BW_FACTOR: whole extraction where ctl[0] != 0 (k_bw_extract of sp_launch_bw_factor: no guard copy);
// BW_SOLVE: the right-hand side in whole blocks (k_bw_load's work, no guard copy: the bordered
// solve phase has saved it)
template <int B, int PHASE>
__global__ __launch_bounds__(BW_THREADS) void kbw_extract(const BandInst *__restrict__ tab, BandShape sh) {
  INST(I);
  const int i = blockIdx.x;
  if (PHASE == BW_FACTOR) {
    if (I.ctl[0] == 0) return;
    if (i == 0 && threadIdx.x == 0) ++I.wcnt[0];
    bw_extract_matrix<B>(I.band, sh.ldb, sh.bw, sh.N, sh.nb, I.bD, I.bL, I.bU, I.flags, i);
    bw_extract_rhs<B>(I.brhs, sh.N, I.bF, nullptr, i);
    return;
  }
  if (PHASE == BW_SOLVE) {
    if (i == 0 && threadIdx.x == 0) ++I.wcnt[1];
    bw_extract_rhs<B>(I.brhs, sh.N, I.bF, nullptr, i);
    return;
  }
  const bool red = bw_reduces(I, sh);
  if (i == 0 && threadIdx.x == 0) ++I.wcnt[red ? 0 : 1];
  if (red) bw_extract_matrix<B>(I.band, sh.ldb, sh.bw, sh.N, sh.nb, I.bD, I.bL, I.bU, I.flags, i);
  bw_extract_rhs<B>(I.brhs, sh.N, I.bF, I.brhs0, i);
}

template <int B, int PHASE>
__global__ __launch_bounds__(BW_THREADS) void kbw_invert(const BandInst *__restrict__ tab, BandShape sh,
                                                         int first, int stride) {
  INST(I);
  __shared__ double M[B * (B + 1)];
  const int i = first + blockIdx.x * stride;
  if (i >= sh.nb || !(PHASE == BW_FACTOR ? I.ctl[0] != 0 : bw_reduces(I, sh))) return;
  bw_invert_block<B>(I.bD, I.bDinv, i, M, I.flags, I.bneg);
}

template <int B, int PHASE>
__global__ __launch_bounds__(BW_THREADS) void kbw_reduce(const BandInst *__restrict__ tab, BandShape sh,
                                                         int s) {
  INST(I);
  __shared__ double T[B * (B + 1)];
  const int i = blockIdx.x * 2 * s;
  if (i >= sh.nb) return;
  if (PHASE == BW_FACTOR) {
    if (I.ctl[0] != 0)
      bw_reduce_block<B, true, false>(I.bD, I.bL, I.bU, I.bF, I.bDinv, I.bMr, I.bMl, sh.nb, s, i, T);
  } else if (PHASE == BW_SOLVE)
    bw_fwd_block<B>(I.bMr, I.bMl, I.bF, sh.nb, s, i, T);
  else if (!sh.split)
    bw_reduce_block<B, false, true>(I.bD, I.bL, I.bU, I.bF, I.bDinv, nullptr, nullptr, sh.nb, s, i, T);
  else if (I.ctl[0] != 0)
    bw_reduce_block<B, true, true>(I.bD, I.bL, I.bU, I.bF, I.bDinv, I.bMr, I.bMl, sh.nb, s, i, T);
  else
    bw_fwd_block<B>(I.bMr, I.bMl, I.bF, sh.nb, s, i, T);
}

// (BW_FACTOR: the last block's product goes to the spare block behind F and is not used, as in
// sp_launch_bw_factor)
template <int B, int PHASE>
__global__ __launch_bounds__(BW_THREADS) void kbw_last(const BandInst *__restrict__ tab, BandShape sh) {
  INST(I);
  __shared__ double M[B * (B + 1)];
  __shared__ double t[B];
  __shared__ int part[BW_THREADS / 64];
  if (PHASE == BW_FACTOR) {
    if (I.ctl[0] != 0)
      bw_last_block<B>(I.bD, I.bDinv, I.bF, I.bF + (int64_t)sh.nb * B, sh.nb, I.flags, I.bneg, M, t, part);
  } else if (PHASE == BW_SOLVE)
    bw_x0_block<B>(I.bDinv, I.bF, I.brhs, t);
  else if (bw_reduces(I, sh))
    bw_last_block<B>(I.bD, I.bDinv, I.bF, I.brhs, sh.nb, I.flags, I.bneg, M, t, part);
  else
    bw_x0_block<B>(I.bDinv, I.bF, I.brhs, t);
}

template <int B>
__global__ __launch_bounds__(BW_THREADS) void kbw_back(const BandInst *__restrict__ tab, BandShape sh,
                                                       int s) {
  INST(I);
  __shared__ double xl[B], xr[B], t[B];
  const int i = s + blockIdx.x * 2 * s;
  if (i >= sh.nb) return;
  bw_back_block<B>(I.bDinv, I.bL, I.bU, I.bF, I.brhs, sh.nb, s, i, xl, xr, t);
}

__global__ __launch_bounds__(256) void kbw_residual(const BandInst *__restrict__ tab, BandShape sh) {
  INST(I);
  __shared__ double pr[4], pb[4];
  bw_residual_rows(I.band, sh.ldb, sh.bw, sh.N, I.brhs, I.brhs0, I.bres, I.stat, I.flags, sh.nred,
                   blockIdx.x, pr, pb);
}

// Panel solve against the kept factors on the instance's Y (sh.bkp columns, whole B-row blocks), for
// the instances in their factor phase: twins of k_bw_fwd_panel / k_bw_back_panel.  LDS: one B x 65
// array, 33 KB at B = 64.
template <int B>
__global__ __launch_bounds__(BW_THREADS) void kbw_fwd_panel(const BandInst *__restrict__ tab, BandShape sh,
                                                            int s) {
  const BandInst &I = tab[blockIdx.y];
  if (I.ctl[0] == 0) return;
  const int i = blockIdx.x * 2 * s;
  if (i >= sh.nb) return;
  bw_fwd_panel_block<B>(I.bMr, I.bMl, I.bY, sh.bkp, sh.nb, s, i);
}

template <int B>
__global__ __launch_bounds__(BW_THREADS) void kbw_back_panel(const BandInst *__restrict__ tab, BandShape sh,
                                                             int s, int first, int stride) {
  const BandInst &I = tab[blockIdx.y];
  if (I.ctl[0] == 0) return;
  __shared__ double T[B * 65];
  const int e = first + blockIdx.x * stride;
  if (e >= sh.nb) return;
  bw_back_panel_block<B>(I.bDinv, I.bL, I.bU, I.bY, sh.bkp, sh.nb, s, e, T);
}

// the walk of bw_solve / bw_backsolve (pgf_band_wide.hip), every launch with the instances in grid.y;
// lean: no instance reduces (the host knows), so the inversion launches are left out
template <int B>
static void bandb_wide_solve(hipStream_t s, const BandInst *tab, int Bi, const BandShape &sh, bool lean) {
  const int nb = sh.nb;
  const unsigned Bu = (unsigned)Bi;
  const dim3 blk(BW_THREADS);
  hipLaunchKernelGGL((kbw_extract<B, BW_BY_CTL>), dim3(nb, Bu), blk, 0, s, tab, sh);
  int levels[32], nlev = 0;
  for (int st = 1; st < nb; st *= 2) {
    const int ne = bcr_eliminated(nb, st), nk = bcr_kept(nb, st);
    if (!lean) hipLaunchKernelGGL((kbw_invert<B, BW_BY_CTL>), dim3(ne, Bu), blk, 0, s, tab, sh, st, 2 * st);
    hipLaunchKernelGGL((kbw_reduce<B, BW_BY_CTL>), dim3(nk, Bu), blk, 0, s, tab, sh, st);
    levels[nlev++] = st;
  }
  hipLaunchKernelGGL((kbw_last<B, BW_BY_CTL>), dim3(1, Bu), blk, 0, s, tab, sh);
  for (int q = nlev - 1; q >= 0; --q) {
    const int st = levels[q];
    hipLaunchKernelGGL(kbw_back<B>, dim3(bcr_eliminated(nb, st), Bu), blk, 0, s, tab, sh, st);
  }
  hipLaunchKernelGGL(kbw_residual, dim3((sh.N + 255) / 256, Bu), dim3(256), 0, s, tab, sh);
}

void bandb_launch_wide_solve(hipStream_t s, const BandInst *tab, int B, const BandShape &sh, bool lean) {
  if (!sh.N) return;
  switch (sh.B) {
    case 16: bandb_wide_solve<16>(s, tab, B, sh, lean); break;
    case 32: bandb_wide_solve<32>(s, tab, B, sh, lean); break;
    default: bandb_wide_solve<64>(s, tab, B, sh, lean); break;
  }
}

// ---- bordered wide route: the band part of pgf_border_batch.hip's two phases -----------------------
// sh: the shape copy with N = Nb and nb = ceil(Nb / B).  Factor-only KEEP reduction of B for the
// instances with ctl[0] != 0: the walk of bw_solve(keep, no right-hand side).
template <int B>
static void bandb_wide_factor(hipStream_t s, const BandInst *tab, int Bi, const BandShape &sh) {
  const int nb = sh.nb;
  const unsigned Bu = (unsigned)Bi;
  const dim3 blk(BW_THREADS);
  hipLaunchKernelGGL((kbw_extract<B, BW_FACTOR>), dim3(nb, Bu), blk, 0, s, tab, sh);
  for (int st = 1; st < nb; st *= 2) {
    hipLaunchKernelGGL((kbw_invert<B, BW_FACTOR>), dim3(bcr_eliminated(nb, st), Bu), blk, 0, s, tab, sh, st,
                       2 * st);
    hipLaunchKernelGGL((kbw_reduce<B, BW_FACTOR>), dim3(bcr_kept(nb, st), Bu), blk, 0, s, tab, sh, st);
  }
  hipLaunchKernelGGL((kbw_last<B, BW_FACTOR>), dim3(1, Bu), blk, 0, s, tab, sh);
}

// Y <- inv(B) Y against the factors just kept, same instances: the walk of bw_panel_solve
template <int B>
static void bandb_wide_panel(hipStream_t s, const BandInst *tab, int Bi, const BandShape &sh) {
  const int nb = sh.nb;
  const unsigned Bu = (unsigned)Bi;
  const dim3 blk(BW_THREADS);
  int levels[32], nlev = 0;
  for (int st = 1; st < nb; st *= 2) {
    hipLaunchKernelGGL(kbw_fwd_panel<B>, dim3(bcr_kept(nb, st), Bu), blk, 0, s, tab, sh, st);
    levels[nlev++] = st;
  }
  hipLaunchKernelGGL(kbw_back_panel<B>, dim3(1, Bu), blk, 0, s, tab, sh, 0, 0, 1);
  for (int q = nlev - 1; q >= 0; --q) {
    const int st = levels[q];
    hipLaunchKernelGGL(kbw_back_panel<B>, dim3(bcr_eliminated(nb, st), Bu), blk, 0, s, tab, sh, st, st, 2 * st);
  }
}

// solve phase of every live instance against its kept factors, whatever ctl[0] says: the walk of
// bw_backsolve without the guard (load, forward per level, x_0, backward per level)
template <int B>
static void bandb_wide_kept_solve(hipStream_t s, const BandInst *tab, int Bi, const BandShape &sh) {
  const int nb = sh.nb;
  const unsigned Bu = (unsigned)Bi;
  const dim3 blk(BW_THREADS);
  hipLaunchKernelGGL((kbw_extract<B, BW_SOLVE>), dim3(nb, Bu), blk, 0, s, tab, sh);
  int levels[32], nlev = 0;
  for (int st = 1; st < nb; st *= 2) {
    hipLaunchKernelGGL((kbw_reduce<B, BW_SOLVE>), dim3(bcr_kept(nb, st), Bu), blk, 0, s, tab, sh, st);
    levels[nlev++] = st;
  }
  hipLaunchKernelGGL((kbw_last<B, BW_SOLVE>), dim3(1, Bu), blk, 0, s, tab, sh);
  for (int q = nlev - 1; q >= 0; --q) {
    const int st = levels[q];
    hipLaunchKernelGGL(kbw_back<B>, dim3(bcr_eliminated(nb, st), Bu), blk, 0, s, tab, sh, st);
  }
}

#define BW_DISPATCH(fn, ...)                 \
  switch (sh.B) {                            \
    case 16: fn<16>(__VA_ARGS__); break;     \
    case 32: fn<32>(__VA_ARGS__); break;     \
    default: fn<64>(__VA_ARGS__); break;     \
  }

void bandb_launch_wide_factor(hipStream_t s, const BandInst *tab, int B, const BandShape &sh) {
  if (!sh.N) return;
  BW_DISPATCH(bandb_wide_factor, s, tab, B, sh);
}
void bandb_launch_wide_panel(hipStream_t s, const BandInst *tab, int B, const BandShape &sh) {
  if (!sh.N) return;
  BW_DISPATCH(bandb_wide_panel, s, tab, B, sh);
}
void bandb_launch_wide_kept_solve(hipStream_t s, const BandInst *tab, int B, const BandShape &sh) {
  if (!sh.N) return;
  BW_DISPATCH(bandb_wide_kept_solve, s, tab, B, sh);
}
