// Banded device batch: the kernels of the narrow banded Newton step (pgf_sparse.hip) with a batch
// dimension.  Every kernel here is the twin of a kernel of one handle: instance = blockIdx.y, its
// pointers from the BandInst table, the pattern arrays (equal across the instances by construction)
// from instance 0 through BandShape, and then the SAME device function from pgf_band_dev.h with the
// same arguments in the same order -- the batch computes, instance by instance, the bits the single
// handle computes.  One launch sequence serves the whole batch: the launch plan of the reduction
// depends on N only (sp_bcr_plan).
//
// The batch's control words (BInst::ctl): a frozen instance's workgroups return at once (ctl[3]); an
// instance whose matrix did not change skips the assembly (ctl[0] == 0) but still runs the
// reduction -- the 8 x 8 reduction keeps no factors, and leaves the band intact.  Pivot flags and
// negative-pivot counts are the instance's own arrays.
//
// kbb_step_final has no twin: it is what band_batch_sync does on the host after a step, one wavefront
// per instance, for the device-resident controller's loop (narrow and wide route alike).
//
// Grid shape of the one-workgroup LDS tail: (1, B) workgroups of 1024 threads.  The tail holds
// 94 KB of the CU's 160 KB of LDS, so a CU takes one at a time: up to 256 instances the tails run
// side by side, one per CU, beyond that in waves of 256.
//
// Compiled with -ffp-contract=off like pgf_sparse.hip (explicit fma() only).
#include "pgf_band_dev.h"
#include "pgf_internal.h"
#include "pgf_sparse.h"

#define INST(I)                           \
  const BandInst &I = tab[blockIdx.y];    \
  if (I.ctl[3]) return /* frozen: sits this step out */

// ---------------------------------------------------------------- evaluation
__global__ void kbb_sp_eval_c(const BandInst *__restrict__ tab, BandShape sh) {
  const BandInst &I = tab[blockIdx.y];  // (also of a frozen instance: its norms are read)
  b_sp_eval_c(sh.m, sh.Jptr, sh.Jcol, I.Jval, I.x, I.b, I.ps[BPS_RHO], I.y, I.c, I.w);
}

__global__ void kbb_sp_eval_g(const BandInst *__restrict__ tab, BandShape sh) {
  const BandInst &I = tab[blockIdx.y];
  b_sp_eval_g(sh.n, sh.Hptr, sh.Hcol, I.Hval, sh.JTptr, sh.JTrow, sh.JTmap, I.Jval, I.x, I.w, I.q, I.g);
}

// the banded measure evaluation: c = J x - b ; tmpn = q + J' y ; F[0:n] = H x + tmpn
__global__ void kbb_meas_c(const BandInst *__restrict__ tab, BandShape sh) {
  const BandInst &I = tab[blockIdx.y];
  b_csr_spmv(sh.m, sh.Jptr, sh.Jcol, I.Jval, I.x, I.b, -1.0, I.c);
}
__global__ void kbb_meas_t(const BandInst *__restrict__ tab, BandShape sh) {
  const BandInst &I = tab[blockIdx.y];
  b_csc_spmvT(sh.n, sh.JTptr, sh.JTrow, sh.JTmap, I.Jval, I.y, I.q, I.tmpn);
}
__global__ void kbb_meas_f(const BandInst *__restrict__ tab, BandShape sh) {
  const BandInst &I = tab[blockIdx.y];
  b_csr_spmv(sh.n, sh.Hptr, sh.Hcol, I.Hval, I.x, I.tmpn, 1.0, I.F);
}

// ---------------------------------------------------------------- right-hand side, assembly
__global__ void kbb_band_rhs_fused(const BandInst *__restrict__ tab, BandShape sh) {
  INST(I);
  b_band_rhs_fused(sh.n, sh.m, I.mask, I.F, I.b0full, sh.Hptr, sh.Hcol, I.Hval, sh.Jptr, sh.Jcol, I.Jval,
                   I.ps[BPS_FACT], sh.pos, I.brhs);
}

// (the single handle clears its band with a memset; B memsets would be B launches)
__global__ void kbb_band_zero(const BandInst *__restrict__ tab, BandShape sh) {
  const BandInst &I = tab[blockIdx.y];
  if (I.ctl[0] == 0) return;
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < (int64_t)(sh.N + 1) * sh.ldb) I.band[p] = 0.0;
}

__global__ void kbb_band_set_diag(const BandInst *__restrict__ tab, BandShape sh) {
  const BandInst &I = tab[blockIdx.y];
  if (I.ctl[0] == 0) return;
  b_band_set_diag(sh.n, sh.m, sh.pos, I.mask, I.ps[BPS_LAMB], I.ps[BPS_DELTA], I.band, sh.ldb);
}

__global__ void kbb_band_scatter_H(const BandInst *__restrict__ tab, BandShape sh) {
  const BandInst &I = tab[blockIdx.y];
  if (I.ctl[0] == 0) return;
  b_band_scatter_H(sh.nnzH, sh.Hrow, sh.Hcol, I.Hval, sh.Hslot, I.mask, I.band);
}

__global__ void kbb_band_scatter_J(const BandInst *__restrict__ tab, BandShape sh) {
  const BandInst &I = tab[blockIdx.y];
  if (I.ctl[0] == 0) return;
  b_band_scatter_J(sh.nnzJ, sh.Jcol, I.Jval, sh.Jslot, I.mask, I.band);
}

// ---------------------------------------------------------------- block cyclic reduction
// set: which of the instance's two block sets (SparseDev::bstride blocks apart)
#define SETP(I, arr, set, w) ((I).arr + (size_t)(set) * sh.bstride * (w))

__global__ __launch_bounds__(64) void kbb_bcr_extract(const BandInst *__restrict__ tab, BandShape sh) {
  INST(I);
  b_bcr_extract(I.band, sh.ldb, sh.bw, I.brhs, sh.N, sh.nb, I.bD, I.bL, I.bU, I.bF, I.brhs0, I.flags);
}

__global__ __launch_bounds__(64) void kbb_bcr_invert(const BandInst *__restrict__ tab, BandShape sh,
                                                     int set, int s, int first, int stride) {
  INST(I);
  __shared__ double sm[BCR_SCRATCH];
  const int i = first + blockIdx.x * stride;
  if (i >= sh.nb) return;
  bcr_invert_block(SETP(I, bD, set, 64), I.bDinv, i, threadIdx.x, sm, I.flags, I.bneg, i);
}

__global__ __launch_bounds__(64) void kbb_bcr_reduce(const BandInst *__restrict__ tab, BandShape sh,
                                                     int set, int s) {
  INST(I);
  __shared__ double sm[BCR_SCRATCH];
  const int i = blockIdx.x * 2 * s;
  if (i >= sh.nb) return;
  bcr_reduce_block(SETP(I, bD, set, 64), SETP(I, bL, set, 64), SETP(I, bU, set, 64), SETP(I, bF, set, 8),
                   I.bDinv, sh.nb, s, i, threadIdx.x, sm);
}

__global__ __launch_bounds__(64) void kbb_bcr_level(const BandInst *__restrict__ tab, BandShape sh,
                                                    int set, int s) {
  INST(I);
  __shared__ double sm[BCR_SCRATCH];
  const int i = blockIdx.x * 2 * s;
  if (i >= sh.nb) return;
  double *D = SETP(I, bD, set, 64), *L = SETP(I, bL, set, 64), *U = SETP(I, bU, set, 64);
  double *F = SETP(I, bF, set, 8);
  bcr_level_block(D, L, U, F, I.bDinv, sh.nb, s, i, threadIdx.x, sm, I.flags, I.bneg, D, L, U, F, i, true,
                  i + s);
}

__global__ __launch_bounds__(192) void kbb_bcr_level2(const BandInst *__restrict__ tab, BandShape sh,
                                                      int set, int s) {
  INST(I);
  b_bcr_level2(SETP(I, bD, set, 64), SETP(I, bL, set, 64), SETP(I, bU, set, 64), SETP(I, bF, set, 8),
               SETP(I, bD, set ^ 1, 64), SETP(I, bL, set ^ 1, 64), SETP(I, bU, set ^ 1, 64),
               SETP(I, bF, set ^ 1, 8), I.bDinv, sh.nb, s, I.flags, I.bneg);
}

__global__ __launch_bounds__(1024) void kbb_bcr_tail(const BandInst *__restrict__ tab, BandShape sh,
                                                     int set, int s0) {
  INST(I);
  b_bcr_tail(SETP(I, bD, set, 64), SETP(I, bL, set, 64), SETP(I, bU, set, 64), SETP(I, bF, set, 8), I.brhs,
             sh.nb, s0, I.flags, I.bneg);
}

__global__ __launch_bounds__(64) void kbb_bcr_back(const BandInst *__restrict__ tab, BandShape sh,
                                                   int set, int s, int first, int stride) {
  INST(I);
  __shared__ double sm[BCR_SCRATCH];
  const int i = first + blockIdx.x * stride;
  if (i >= sh.nb) return;
  bcr_back_block(I.bDinv, SETP(I, bL, set, 64), SETP(I, bU, set, 64), SETP(I, bF, set, 8), I.brhs, sh.nb, s,
                 i, threadIdx.x, sm);
}

__global__ __launch_bounds__(128) void kbb_bcr_back2(const BandInst *__restrict__ tab, BandShape sh,
                                                     int s1, int s2, int s) {
  INST(I);
  b_bcr_back2(I.bDinv, SETP(I, bL, s1, 64), SETP(I, bU, s1, 64), SETP(I, bF, s1, 8), SETP(I, bL, s2, 64),
              SETP(I, bU, s2, 64), SETP(I, bF, s2, 8), I.brhs, sh.nb, s);
}

__global__ __launch_bounds__(256) void kbb_band_residual(const BandInst *__restrict__ tab, BandShape sh) {
  INST(I);
  b_band_residual(I.band, sh.ldb, sh.bw, sh.N, I.brhs, I.brhs0, I.bres, I.stat, I.flags, sh.nred);
}

// ---------------------------------------------------------------- step update
__global__ __launch_bounds__(256) void kbb_band_step_update(const BandInst *__restrict__ tab,
                                                            BandShape sh) {
  INST(I);
  b_band_step_update(sh.n, sh.m, sh.pos, I.brhs, I.ps[BPS_FACT], I.ps[BPS_RHO], I.x, I.y, I.lb, I.ub, I.F,
                     I.dx, I.dy, I.xn, I.yn, I.stat + 2 * sh.nred);
  const bool bad = I.flags[0] != 0;  // (final: the reduction's last launch is behind us)
  // the band assembled this step is the valid one from here on (kb_mask_adopt reads ctl[1])
  if (blockIdx.x == 0 && threadIdx.x == 0 && I.ctl[0]) I.ctl[1] = bad ? 0 : 1;
  // A zero or non-finite pivot: the point stays where it was.  Otherwise the new point replaces the
  // current one and the old one stays in (xn, yn), as after the pointer swap of a single handle: the
  // host repairs an instance whose residual misses the tolerance from there (each lane re-reads its
  // own entries).
  if (bad) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < sh.n) {
    const double v = I.xn[i];
    I.xn[i] = I.x[i];
    I.x[i] = v;
  } else if (i < sh.n + sh.m) {
    const int r = i - sh.n;
    const double v = I.yn[r];
    I.yn[r] = I.y[r];
    I.y[r] = v;
  }
}

// The device-resident controller's end of a step: one wavefront per instance, four instances per
// workgroup, grid ceil(B / 4).  A frozen instance took no step: its outputs stay as they are
// (kb_dctl_end reads them only for an instance that was live in step two).
__global__ __launch_bounds__(256) void kbb_step_final(const BandInst *__restrict__ tab, int B, BandShape sh,
                                                      const double *__restrict__ guard,
                                                      double *__restrict__ diff_out,
                                                      int *__restrict__ flags_out, int *__restrict__ rejects) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= B) return;
  const BandInst &I = tab[i];
  if (I.ctl[3]) return;
  b_band_step_final(I.stat, sh.nred, I.counts[0], guard[2 * i] != 0.0, guard[2 * i + 1], diff_out + i,
                    flags_out + 3 * i, rejects + 2 * i);
}

// ---------------------------------------------------------------- launch wrappers
static inline dim3 gy(int64_t cnt, int per, int B) { return dim3((unsigned)((cnt + per - 1) / per), B); }

void bandb_launch_eval(hipStream_t s, const BandInst *tab, int B, const BandShape &sh) {
  if (sh.m) hipLaunchKernelGGL(kbb_sp_eval_c, gy(sh.m, 256, B), dim3(256), 0, s, tab, sh);
  if (sh.n) hipLaunchKernelGGL(kbb_sp_eval_g, gy(sh.n, 256, B), dim3(256), 0, s, tab, sh);
}

void bandb_launch_measures_eval(hipStream_t s, const BandInst *tab, int B, const BandShape &sh) {
  if (sh.m) hipLaunchKernelGGL(kbb_meas_c, gy(sh.m, 256, B), dim3(256), 0, s, tab, sh);
  if (sh.n) {
    hipLaunchKernelGGL(kbb_meas_t, gy(sh.n, 256, B), dim3(256), 0, s, tab, sh);
    hipLaunchKernelGGL(kbb_meas_f, gy(sh.n, 256, B), dim3(256), 0, s, tab, sh);
  }
}

void bandb_launch_rhs(hipStream_t s, const BandInst *tab, int B, const BandShape &sh) {
  if (sh.N) hipLaunchKernelGGL(kbb_band_rhs_fused, gy(sh.N, 256, B), dim3(256), 0, s, tab, sh);
}

void bandb_launch_assemble(hipStream_t s, const BandInst *tab, int B, const BandShape &sh) {
  if (!sh.N) return;
  hipLaunchKernelGGL(kbb_band_zero, gy((int64_t)(sh.N + 1) * sh.ldb, 256, B), dim3(256), 0, s, tab, sh);
  hipLaunchKernelGGL(kbb_band_set_diag, gy(sh.N, 256, B), dim3(256), 0, s, tab, sh);
  if (sh.nnzH) hipLaunchKernelGGL(kbb_band_scatter_H, gy(sh.nnzH, 256, B), dim3(256), 0, s, tab, sh);
  if (sh.nnzJ) hipLaunchKernelGGL(kbb_band_scatter_J, gy(sh.nnzJ, 256, B), dim3(256), 0, s, tab, sh);
}

// the walk of sp_launch_bcr_solve over the same plan, every launch with the instances in grid.y
// (a bordered batch passes a shape whose N, nb are those of the band rows, and residual == false)
void bandb_launch_solve(hipStream_t s, const BandInst *tab, int B, const BandShape &sh, bool residual) {
  if (!sh.N) return;
  const int nb = sh.nb;
  const unsigned Bu = (unsigned)B;
  hipLaunchKernelGGL(kbb_bcr_extract, dim3(nb, Bu), dim3(64), 0, s, tab, sh);
  const BcrPlan plan = sp_bcr_plan(nb);
  for (int q = 0; q < plan.nlev; ++q) {
    const int st = plan.lev[q].s, cur = plan.lev[q].set;
    if (plan.lev[q].pair_set2 >= 0) {
      hipLaunchKernelGGL(kbb_bcr_level2, dim3(bcr_pair_groups(nb, st), Bu), dim3(192), 0, s, tab, sh, cur, st);
      continue;
    }
    const int nk = bcr_kept(nb, st);
    if (plan.fused) {
      hipLaunchKernelGGL(kbb_bcr_level, dim3(nk, Bu), dim3(64), 0, s, tab, sh, cur, st);
    } else {
      const int ne = bcr_eliminated(nb, st);
      if (ne > 0) hipLaunchKernelGGL(kbb_bcr_invert, dim3(ne, Bu), dim3(64), 0, s, tab, sh, cur, st, st, 2 * st);
      hipLaunchKernelGGL(kbb_bcr_reduce, dim3(nk, Bu), dim3(64), 0, s, tab, sh, cur, st);
    }
  }
  hipLaunchKernelGGL(kbb_bcr_tail, dim3(1, Bu), dim3(1024), 0, s, tab, sh, plan.tail_set, plan.tail_s);
  for (int q = plan.nlev - 1; q >= 0; --q) {
    const int bs = plan.lev[q].s;
    if (plan.lev[q].pair_set2 >= 0) {
      const int nj = bcr_back_pair_groups(nb, bs);
      if (nj > 0)
        hipLaunchKernelGGL(kbb_bcr_back2, dim3(nj, Bu), dim3(128), 0, s, tab, sh, plan.lev[q].set,
                           plan.lev[q].pair_set2, bs);
      continue;
    }
    const int ne = bcr_eliminated(nb, bs);
    if (ne > 0)
      hipLaunchKernelGGL(kbb_bcr_back, dim3(ne, Bu), dim3(64), 0, s, tab, sh, plan.lev[q].set, bs, bs, 2 * bs);
  }
  if (residual) hipLaunchKernelGGL(kbb_band_residual, gy(sh.N, 256, B), dim3(256), 0, s, tab, sh);
}

void bandb_launch_step_update(hipStream_t s, const BandInst *tab, int B, const BandShape &sh) {
  if (sh.N) hipLaunchKernelGGL(kbb_band_step_update, gy(sh.N, 256, B), dim3(256), 0, s, tab, sh);
}

void bandb_launch_step_final(hipStream_t s, const BandInst *tab, int B, const BandShape &sh,
                             const double *guard, double *diff_out, int *flags_out, int *rejects) {
  if (sh.N)
    hipLaunchKernelGGL(kbb_step_final, dim3((B + 3) / 4), dim3(256), 0, s, tab, B, sh, guard, diff_out,
                       flags_out, rejects);
}
