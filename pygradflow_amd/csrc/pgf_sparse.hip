// Sparse (banded) variant of the Newton/KKT step: CSR Hessian / Jacobian resident in HBM,
// KKT matrix assembled into a symmetric band (after a host-computed bandwidth-reducing
// permutation of the FIXED full pattern), banded LDL^T and banded triangular solves.
//
// The reduced system of the reference (symmetric_step_solver.py:49-94) drops the active
// rows / columns; here the system keeps its full size n + m and an active variable a
// becomes an identity row / column with right-hand side b0[a].  The two systems have the
// same solution on the inactive set, s[a] = b0[a] is what the reference scatters into
// dx[A] anyway (symmetric_step_solver.py:115-121), the added unit pivots are positive so
// the inertia count is unchanged, and -- the point -- the sparsity pattern, permutation
// and band layout never change while the mask churns.
//
// Band layout: row i of the permuted matrix stores K[i][i - d] at band[i * ldb + d],
// d = 0 .. bw (lower band, row-major); ldb = bw + 1 rounded up to even.
//
// Compiled with -ffp-contract=off like pgf_kernels.hip (explicit fma() only).
#include "pgf_sparse.h"
#include "pgf_band_dev.h"
#include "pgf_band_batch.h"
#include "pgf_batch.h"
#include "pgf_env.h"

#define ACTIVE_EPS 1e-8

// ---------------------------------------------------------------- kernels of one handle
// Thin wrappers of the device bodies in pgf_band_dev.h (shared with the batched twins at the end
// of this file).
__global__ void k_csr_spmv(int rows, const int *__restrict__ ptr, const int *__restrict__ col,
                           const double *__restrict__ val, const double *__restrict__ x,
                           const double *__restrict__ add, double sgn, double *__restrict__ y) {
  b_csr_spmv(rows, ptr, col, val, x, add, sgn, y);
}

__global__ void k_csc_spmvT(int cols, const int *__restrict__ tptr, const int *__restrict__ trow,
                            const int *__restrict__ tmap, const double *__restrict__ val,
                            const double *__restrict__ w, const double *__restrict__ base,
                            double *__restrict__ out) {
  b_csc_spmvT(cols, tptr, trow, tmap, val, w, base, out);
}

__global__ void k_sp_eval_c(int m, const int *__restrict__ ptr, const int *__restrict__ col,
                            const double *__restrict__ val, const double *__restrict__ x,
                            const double *__restrict__ b, double rho, const double *__restrict__ y,
                            double *__restrict__ c, double *__restrict__ w) {
  b_sp_eval_c(m, ptr, col, val, x, b, rho, y, c, w);
}

__global__ void k_sp_eval_g(int n, const int *__restrict__ hptr, const int *__restrict__ hcol,
                            const double *__restrict__ hval, const int *__restrict__ tptr,
                            const int *__restrict__ trow, const int *__restrict__ tmap,
                            const double *__restrict__ jval, const double *__restrict__ x,
                            const double *__restrict__ w, const double *__restrict__ q,
                            double *__restrict__ g) {
  b_sp_eval_g(n, hptr, hcol, hval, tptr, trow, tmap, jval, x, w, q, g);
}

__global__ void k_band_rhs_fused(int n, int m, const uint8_t *__restrict__ mask,
                                 const double *__restrict__ F, const double *__restrict__ b0full,
                                 const int *__restrict__ hptr, const int *__restrict__ hcol,
                                 const double *__restrict__ hval, const int *__restrict__ jptr,
                                 const int *__restrict__ jcol, const double *__restrict__ jval,
                                 double fact, const int *__restrict__ pos, double *__restrict__ brhs) {
  b_band_rhs_fused(n, m, mask, F, b0full, hptr, hcol, hval, jptr, jcol, jval, fact, pos, brhs);
}

__global__ void k_band_set_diag(int n, int m, const int *__restrict__ pos,
                                const uint8_t *__restrict__ mask, double lamb, double delta,
                                double *__restrict__ band, int ldb) {
  b_band_set_diag(n, m, pos, mask, lamb, delta, band, ldb);
}

__global__ void k_band_scatter_H(int nnz, const int *__restrict__ row, const int *__restrict__ col,
                                 const double *__restrict__ val, const int *__restrict__ slot,
                                 const uint8_t *__restrict__ mask, double *__restrict__ band) {
  b_band_scatter_H(nnz, row, col, val, slot, mask, band);
}

__global__ void k_band_scatter_J(int nnz, const int *__restrict__ col,
                                 const double *__restrict__ val, const int *__restrict__ slot,
                                 const uint8_t *__restrict__ mask, double *__restrict__ band) {
  b_band_scatter_J(nnz, col, val, slot, mask, band);
}

// full-length vector <-> permuted band order (LinearSolver.solve against the banded factor)
__global__ void k_band_permute(int N, const int *__restrict__ pos, const double *__restrict__ in,
                               double *__restrict__ out, int gather) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  if (gather) out[i] = in[pos[i]];
  else out[pos[i]] = in[i];
}


__global__ __launch_bounds__(256) void k_band_step_update(
    int n, int m, const int *__restrict__ pos, const double *__restrict__ sol, double fact,
    double rho, const double *__restrict__ x, const double *__restrict__ y,
    const double *__restrict__ lb, const double *__restrict__ ub, const double *__restrict__ F,
    double *__restrict__ dx, double *__restrict__ dy, double *__restrict__ xn,
    double *__restrict__ yn, double *__restrict__ red) {
  b_band_step_update(n, m, pos, sol, fact, rho, x, y, lb, ub, F, dx, dy, xn, yn, red);
}


// ---------------------------------------------------------------- launch wrappers
static inline dim3 g1(int n, int b = 256) { return dim3((n + b - 1) / b); }

void sp_launch_spmv(hipStream_t s, int rows, const int *ptr, const int *col, const double *val,
                    const double *x, const double *add, double sgn, double *y) {
  if (rows) hipLaunchKernelGGL(k_csr_spmv, g1(rows), dim3(256), 0, s, rows, ptr, col, val, x, add, sgn, y);
}

void sp_launch_spmvT(hipStream_t s, int cols, const int *tptr, const int *trow, const int *tmap,
                     const double *val, const double *w, const double *base, double *out) {
  if (cols)
    hipLaunchKernelGGL(k_csc_spmvT, g1(cols), dim3(256), 0, s, cols, tptr, trow, tmap, val, w, base, out);
}

void sp_launch_eval(hipStream_t s, const SparseDev &sp, int n, int m, const double *x, const double *y,
                    const double *b, const double *q, double rho, double *c, double *w, double *g) {
  if (m) hipLaunchKernelGGL(k_sp_eval_c, g1(m), dim3(256), 0, s, m, sp.pat.Jptr, sp.pat.Jcol, sp.pat.Jval, x, b, rho, y, c, w);
  if (n)
    hipLaunchKernelGGL(k_sp_eval_g, g1(n), dim3(256), 0, s, n, sp.pat.Hptr, sp.pat.Hcol, sp.pat.Hval, sp.pat.JTptr, sp.pat.JTrow,
                       sp.pat.JTmap, sp.pat.Jval, x, w, q, g);
}

void sp_launch_assemble(hipStream_t s, const SparseDev &sp, int n, int m, const uint8_t *mask,
                        double lamb, double delta) {
  const int N = n + m;
  (void)hipMemsetAsync(sp.pat.band, 0, (size_t)(N + 1) * sp.pat.ldb * sizeof(double), s);
  hipLaunchKernelGGL(k_band_set_diag, g1(N), dim3(256), 0, s, n, m, sp.pat.pos, mask, lamb, delta,
                     sp.pat.band, sp.pat.ldb);
  sp_launch_scatter(s, sp, mask);
}

// the stored entries of H and J into their slots (band, or the border store behind it)
void sp_launch_scatter(hipStream_t s, const SparseDev &sp, const uint8_t *mask) {
  if (sp.pat.nnzH)
    hipLaunchKernelGGL(k_band_scatter_H, g1(sp.pat.nnzH), dim3(256), 0, s, sp.pat.nnzH, sp.pat.Hrow, sp.pat.Hcol,
                       sp.pat.Hval, sp.pat.Hslot, mask, sp.pat.band);
  if (sp.pat.nnzJ)
    hipLaunchKernelGGL(k_band_scatter_J, g1(sp.pat.nnzJ), dim3(256), 0, s, sp.pat.nnzJ, sp.pat.Jcol, sp.pat.Jval,
                       sp.pat.Jslot, mask, sp.pat.band);
}

void sp_launch_rhs(hipStream_t s, const SparseDev &sp, int n, int m, const uint8_t *mask,
                   const double *F, const double *b0full, double fact, double *Hb0, double *Jb0) {
  (void)Hb0;
  (void)Jb0;
  if (n + m)
    hipLaunchKernelGGL(k_band_rhs_fused, g1(n + m), dim3(256), 0, s, n, m, mask, F, b0full, sp.pat.Hptr, sp.pat.Hcol,
                       sp.pat.Hval, sp.pat.Jptr, sp.pat.Jcol, sp.pat.Jval, fact, sp.pat.pos, sp.vec.brhs);
}

void sp_launch_permute(hipStream_t s, const SparseDev &sp, int N, const double *in, double *out,
                       int gather) {
  if (N) hipLaunchKernelGGL(k_band_permute, g1(N), dim3(256), 0, s, N, sp.pat.pos, in, out, gather);
}

void sp_launch_step_update(hipStream_t s, const SparseDev &sp, int n, int m, double fact,
                           double rho, const double *x, const double *y, const double *lb,
                           const double *ub, const double *F, double *dx, double *dy, double *xn,
                           double *yn, double *red) {
  const int nb = (n + m + 255) / 256;
  if (nb)
    hipLaunchKernelGGL(k_band_step_update, dim3(nb), dim3(256), 0, s, n, m, sp.pat.pos, sp.vec.brhs, fact,
                       rho, x, y, lb, ub, F, dx, dy, xn, yn, red);
}

// ================================================================= block cyclic reduction
// (the algorithm and the per-block device functions: pgf_band_dev.h)
__global__ __launch_bounds__(64) void k_bcr_extract(const double *__restrict__ band, int ldb, int bw,
                                                    const double *__restrict__ rhs, int N, int nb,
                                                    double *__restrict__ D, double *__restrict__ L,
                                                    double *__restrict__ U, double *__restrict__ F,
                                                    double *__restrict__ rhs0,
                                                    int *__restrict__ flags) {
  b_bcr_extract(band, ldb, bw, rhs, N, nb, D, L, U, F, rhs0, flags);
}

// invert the blocks eliminated at this level: i = s, 3s, 5s, ... (i mod 2s == s)
__global__ __launch_bounds__(64) void k_bcr_invert(const double *__restrict__ D,
                                                   double *__restrict__ Dinv, int nb, int s,
                                                   int first, int stride, int *__restrict__ flags,
                                                   int *__restrict__ negcnt) {
  __shared__ double sm[BCR_SCRATCH];
  const int i = first + blockIdx.x * stride;
  if (i >= nb) return;
  bcr_invert_block(D, Dinv, i, threadIdx.x, sm, flags, negcnt, i);
  (void)s;
}

// reduce the kept blocks of this level: i = 0, 2s, 4s, ...
__global__ __launch_bounds__(64) void k_bcr_reduce(double *__restrict__ D, double *__restrict__ L,
                                                   double *__restrict__ U, double *__restrict__ F,
                                                   const double *__restrict__ Dinv, int nb, int s) {
  __shared__ double sm[BCR_SCRATCH];
  const int i = blockIdx.x * 2 * s;
  if (i >= nb) return;
  bcr_reduce_block(D, L, U, F, Dinv, nb, s, i, threadIdx.x, sm);
}

// invert + reduce of one level (blocks 0, 2s, 4s, ... are kept)
__global__ __launch_bounds__(64) void k_bcr_level(double *__restrict__ D, double *__restrict__ L,
                                                  double *__restrict__ U, double *__restrict__ F,
                                                  double *__restrict__ Dinv, int nb, int s,
                                                  int *__restrict__ flags,
                                                  int *__restrict__ negcnt) {
  __shared__ double sm[BCR_SCRATCH];
  const int i = blockIdx.x * 2 * s;
  if (i >= nb) return;
  bcr_level_block(D, L, U, F, Dinv, nb, s, i, threadIdx.x, sm, flags, negcnt, D, L, U, F, i, true,
                  i + s);
}

// two levels (strides s and 2 s) in one launch
__global__ __launch_bounds__(192) void k_bcr_level2(const double *__restrict__ Di,
                                                    const double *__restrict__ Li,
                                                    const double *__restrict__ Ui,
                                                    const double *__restrict__ Fi,
                                                    double *__restrict__ Do, double *__restrict__ Lo,
                                                    double *__restrict__ Uo, double *__restrict__ Fo,
                                                    double *__restrict__ Dinv, int nb, int s,
                                                    int *__restrict__ flags,
                                                    int *__restrict__ negcnt) {
  b_bcr_level2(Di, Li, Ui, Fi, Do, Lo, Uo, Fo, Dinv, nb, s, flags, negcnt);
}

// back-substitution of the blocks eliminated at this level (i mod 2s == s)
__global__ __launch_bounds__(64) void k_bcr_back(const double *__restrict__ Dinv,
                                                 const double *__restrict__ L,
                                                 const double *__restrict__ U,
                                                 const double *__restrict__ F,
                                                 double *__restrict__ X, int nb, int s, int first,
                                                 int stride) {
  __shared__ double sm[BCR_SCRATCH];
  const int i = first + blockIdx.x * stride;
  if (i >= nb) return;
  bcr_back_block(Dinv, L, U, F, X, nb, s, i, threadIdx.x, sm);
}

// back-substitution of two levels in one launch (the mirror of k_bcr_level2)
__global__ __launch_bounds__(128) void k_bcr_back2(const double *__restrict__ Dinv,
                                                   const double *__restrict__ L1,
                                                   const double *__restrict__ U1,
                                                   const double *__restrict__ F1,
                                                   const double *__restrict__ L2,
                                                   const double *__restrict__ U2,
                                                   const double *__restrict__ F2,
                                                   double *__restrict__ X, int nb, int s) {
  b_bcr_back2(Dinv, L1, U1, F1, L2, U2, F2, X, nb, s);
}

// all levels from stride s0 upwards, the last block and the matching back-substitution levels in
// one workgroup, in LDS
#define BCR_PAIR_MAX 4096  // blocks in play up to which two levels share a launch
__global__ __launch_bounds__(1024) void k_bcr_tail(const double *__restrict__ D,
                                                   const double *__restrict__ L,
                                                   const double *__restrict__ U,
                                                   const double *__restrict__ F,
                                                   double *__restrict__ X, int nb, int s0,
                                                   int *__restrict__ flags,
                                                   int *__restrict__ negcnt) {
  b_bcr_tail(D, L, U, F, X, nb, s0, flags, negcnt);
}


// accuracy guard: residual of the solution against the intact band (b_band_residual)
__global__ __launch_bounds__(256) void k_band_residual(const double *__restrict__ band, int ldb, int bw,
                                                       int N, const double *__restrict__ x,
                                                       const double *__restrict__ rhs0,
                                                       double *__restrict__ r,
                                                       double *__restrict__ rsmax,
                                                       const int *__restrict__ flags, int nred) {
  b_band_residual(band, ldb, bw, N, x, rhs0, r, rsmax, flags, nred);
}

void sp_launch_band_residual(hipStream_t s, const SparseDev &sp, int N, const int *flags) {
  if (N == 0) return;
  hipLaunchKernelGGL(k_band_residual, g1(N), dim3(256), 0, s, sp.pat.band, sp.pat.ldb, sp.pat.bw, N, sp.vec.brhs, sp.vec.brhs0,
                     sp.vec.bres, sp.vec.bred, flags, sp.vec.nred);
}

// x = saved + correction (refinement step of the guard)
__global__ void k_band_axpy(int N, const double *__restrict__ a, double *__restrict__ x) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < N) x[i] += a[i];
}
void sp_launch_band_axpy(hipStream_t s, int N, const double *a, double *x) {
  if (N) hipLaunchKernelGGL(k_band_axpy, g1(N), dim3(256), 0, s, N, a, x);
}

// The launch plan of the reduction for nb blocks (it depends on nb and the process's switches
// only: one plan serves every instance of a banded batch, below).
// levels with many blocks: one workgroup per block; from the first level with at most
// BCR_TAIL_BLOCKS blocks left: everything in one workgroup, in LDS
// (tests/band_util.py, bcr_launch_plan, restates this loop on the host so that the schedule tests
// can assert the plan each switch gives: keep the two in step)
BcrPlan sp_bcr_plan(int nb) {
  // PGF_BCR_FUSED=0: separate invert / reduce launches per level
  static const bool fused_levels = env_on("PGF_BCR_FUSED");
  // PGF_BCR_PAIRS=0: one level per launch throughout (two per launch where two more levels
  // are due before the tail and the level is launch-bound: at most BCR_PAIR_MAX blocks in play)
  static const bool pairs = env_on("PGF_BCR_PAIRS");
  static const int pair_max = env_int("PGF_BCR_PAIR_MAX", BCR_PAIR_MAX);
  BcrPlan p;
  p.fused = fused_levels;
  int cur = 0;  // set holding the blocks in play
  int st = 1;
  while (st < nb) {
    const int left = (nb + st - 1) / st;  // blocks still in play before this level
    if (left <= BCR_TAIL_BLOCKS) break;
    const int left2 = (nb + 2 * st - 1) / (2 * st);
    if (fused_levels && pairs && left <= pair_max && left2 > BCR_TAIL_BLOCKS && 2 * st < nb) {
      p.lev[p.nlev++] = {st, cur, cur ^ 1};
      cur ^= 1;
      st *= 4;
      continue;
    }
    p.lev[p.nlev++] = {st, cur, -1};
    st *= 2;
  }
  // st: first level NOT done above (st >= nb: only the last block is left)
  p.tail_s = st;
  p.tail_set = cur;
  return p;
}

// Solve the banded system in sp.pat.band / sp.vec.brhs by block cyclic reduction; the solution
// replaces sp.vec.brhs.  flags[0] zero pivot, flags[1] negative pivots.
// guard: keep the right-hand side and finish with the residual of the solution (bres, bred);
// a correction solve of the refinement runs without.
void sp_launch_bcr_solve(hipStream_t s, const SparseDev &sp, int N, int *flags, bool guard) {
  if (N == 0) {
    (void)hipMemsetAsync(flags, 0, 4 * sizeof(int), s);
    return;
  }
  const int nb = (N + 7) / 8;
  hipLaunchKernelGGL(k_bcr_extract, dim3(nb), dim3(64), 0, s, sp.pat.band, sp.pat.ldb, sp.pat.bw, sp.vec.brhs, N, nb,
                     sp.blk.bD, sp.blk.bL, sp.blk.bU, sp.blk.bF, guard ? sp.vec.brhs0 : nullptr, flags);
  const BcrPlan plan = sp_bcr_plan(nb);
  auto Dp = [&](int set) { return sp.blk.bD + (size_t)set * sp.blk.bstride * 64; };
  auto Lp = [&](int set) { return sp.blk.bL + (size_t)set * sp.blk.bstride * 64; };
  auto Up = [&](int set) { return sp.blk.bU + (size_t)set * sp.blk.bstride * 64; };
  auto Fp = [&](int set) { return sp.blk.bF + (size_t)set * sp.blk.bstride * 8; };
  for (int q = 0; q < plan.nlev; ++q) {
    const int st = plan.lev[q].s, cur = plan.lev[q].set;
    if (plan.lev[q].pair_set2 >= 0) {
      hipLaunchKernelGGL(k_bcr_level2, dim3(bcr_pair_groups(nb, st)), dim3(192), 0, s, Dp(cur), Lp(cur),
                         Up(cur), Fp(cur), Dp(cur ^ 1), Lp(cur ^ 1), Up(cur ^ 1), Fp(cur ^ 1), sp.blk.bDinv, nb,
                         st, flags, sp.blk.bneg);
      continue;
    }
    const int nk = bcr_kept(nb, st);
    if (plan.fused) {
      hipLaunchKernelGGL(k_bcr_level, dim3(nk), dim3(64), 0, s, Dp(cur), Lp(cur), Up(cur), Fp(cur),
                         sp.blk.bDinv, nb, st, flags, sp.blk.bneg);
    } else {
      const int ne = bcr_eliminated(nb, st);
      if (ne > 0)
        hipLaunchKernelGGL(k_bcr_invert, dim3(ne), dim3(64), 0, s, Dp(cur), sp.blk.bDinv, nb, st, st,
                           2 * st, flags, sp.blk.bneg);
      hipLaunchKernelGGL(k_bcr_reduce, dim3(nk), dim3(64), 0, s, Dp(cur), Lp(cur), Up(cur), Fp(cur),
                         sp.blk.bDinv, nb, st);
    }
  }
  const int cur = plan.tail_set;
  hipLaunchKernelGGL(k_bcr_tail, dim3(1), dim3(1024), 0, s, Dp(cur), Lp(cur), Up(cur), Fp(cur), sp.vec.brhs, nb,
                     plan.tail_s, flags, sp.blk.bneg);
  for (int q = plan.nlev - 1; q >= 0; --q) {
    const int bs = plan.lev[q].s;
    if (plan.lev[q].pair_set2 >= 0) {
      const int s2 = plan.lev[q].pair_set2, s1 = plan.lev[q].set;
      const int nj = bcr_back_pair_groups(nb, bs);
      if (nj > 0)
        hipLaunchKernelGGL(k_bcr_back2, dim3(nj), dim3(128), 0, s, sp.blk.bDinv, Lp(s1), Up(s1), Fp(s1),
                           Lp(s2), Up(s2), Fp(s2), sp.vec.brhs, nb, bs);
      continue;
    }
    const int ne = bcr_eliminated(nb, bs);
    if (ne > 0)
      hipLaunchKernelGGL(k_bcr_back, dim3(ne), dim3(64), 0, s, sp.blk.bDinv, Lp(plan.lev[q].set),
                         Up(plan.lev[q].set), Fp(plan.lev[q].set), sp.vec.brhs, nb, bs, bs, 2 * bs);
  }
  // (the back-substitution has written the solution into sp.vec.brhs, where the caller reads it)
  if (guard) sp_launch_band_residual(s, sp, N, flags);
}

// ================================================================= banded device batch, narrow route
// The kernels of the narrow banded Newton step (above) with a batch dimension.  Every kernel here is the twin of a kernel of one handle: instance = blockIdx.y, its
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
// (Handle kernel and twin share this file, so they share its -ffp-contract=off.)
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
// set: which of the instance's two block sets (SparseDev::blk.bstride blocks apart)
#define SETP(I, arr, set, w) ((I).arr + (size_t)(set) * sh.bstride * (w))

__global__ __launch_bounds__(64) void kbb_bcr_extract(const BandInst *__restrict__ tab, BandShape sh) {
  INST(I);
  b_bcr_extract(I.band, sh.ldb, sh.bw, I.brhs, sh.N, sh.nb, I.bD, I.bL, I.bU, I.bF, I.brhs0, I.flags);
}

// the same with the guard off (a refinement round): brhs0 keeps the step's right-hand side
__global__ __launch_bounds__(64) void kbb_bcr_extract_ng(const BandInst *__restrict__ tab, BandShape sh) {
  INST(I);
  b_bcr_extract(I.band, sh.ldb, sh.bw, I.brhs, sh.N, sh.nb, I.bD, I.bL, I.bU, I.bF, nullptr, I.flags);
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
                                                            BandShape sh, int move) {
  INST(I);
  b_band_step_update(sh.n, sh.m, sh.pos, I.brhs, I.ps[BPS_FACT], I.ps[BPS_RHO], I.x, I.y, I.lb, I.ub, I.F,
                     I.dx, I.dy, I.xn, I.yn, I.stat + 2 * sh.nred);
  const bool bad = I.flags[0] != 0;  // (final: the reduction's last launch is behind us)
  // the band assembled this step is the valid one from here on (kb_mask_adopt reads ctl[1])
  if (blockIdx.x == 0 && threadIdx.x == 0 && I.ctl[0]) I.ctl[1] = bad ? 0 : 1;
  // A zero or non-finite pivot: the point stays where it was.  Otherwise the new point replaces the
  // current one and the old one stays in (xn, yn), as after the pointer swap of a single handle: the
  // host repairs an instance whose residual misses the tolerance from there (each lane re-reads its
  // own entries).  move == 0 (a Globalized step, whose table names the outer point): only the clipped
  // direction is wanted, kb_ls_finish moves the point.
  if (bad || !move) return;
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
                                                      int *__restrict__ flags_out, int *__restrict__ rejects,
                                                      const int *__restrict__ rctl) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= B) return;
  const BandInst &I = tab[i];
  if (I.ctl[3]) return;
  const double *g = guard + (size_t)BG_STRIDE * i;
  b_band_step_final(I.stat, sh.nred, I.counts[0], g[0] != 0.0, g[1], diff_out + i, flags_out + 3 * i,
                    rejects + 2 * i, rctl ? rctl + 4 * i : nullptr, g[2]);
}

// ---------------------------------------------------------------- refinement inside the loop
// (PGF_BATCH_CTL_REFINE) band_refine's round for the instances that refine.  kbb_refine_decide has
// kbb_step_final's grid and reads the batch's own table; the others take the refinement table, whose
// ctl is the instance's refinement words: INST returns for an instance that sits the round out.
__global__ __launch_bounds__(256) void kbb_refine_decide(const BandInst *__restrict__ tab, int B, BandShape sh,
                                                         const double *__restrict__ guard,
                                                         int *__restrict__ rctl, double *__restrict__ rrel,
                                                         int *__restrict__ rcnt, int round) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= B) return;
  const BandInst &I = tab[i];
  const double *g = guard + (size_t)BG_STRIDE * i;
  b_band_refine_decide(I.stat, sh.nred, I.ctl[3] != 0, g[0] != 0.0, g[1], round, rctl + 4 * i, rrel + i,
                       rcnt + 2 * i);
}

// bsol <- brhs, brhs <- bres (band_refine's two copies) over the n + m entries, and the point the
// step started from back in (x, y) (band_batch_repair's two): kbb_band_step_update swapped it out
__global__ void kbb_refine_load(const BandInst *__restrict__ tab, BandShape sh) {
  INST(I);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= sh.n + sh.m) return;
  I.bsol[i] = I.brhs[i];
  I.brhs[i] = I.bres[i];
  if (i < sh.n)
    I.x[i] = I.xn[i];
  else
    I.y[i - sh.n] = I.yn[i - sh.n];
}

// twin of k_band_axpy: solution = saved + correction
__global__ void kbb_refine_axpy(const BandInst *__restrict__ tab, BandShape sh) {
  INST(I);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < sh.n + sh.m) I.brhs[i] += I.bsol[i];
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
void bandb_launch_solve(hipStream_t s, const BandInst *tab, int B, const BandShape &sh, bool residual,
                        bool save_rhs) {
  if (!sh.N) return;
  const int nb = sh.nb;
  const unsigned Bu = (unsigned)B;
  if (save_rhs)
    hipLaunchKernelGGL(kbb_bcr_extract, dim3(nb, Bu), dim3(64), 0, s, tab, sh);
  else
    hipLaunchKernelGGL(kbb_bcr_extract_ng, dim3(nb, Bu), dim3(64), 0, s, tab, sh);
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

void bandb_launch_step_update(hipStream_t s, const BandInst *tab, int B, const BandShape &sh, bool move) {
  if (sh.N) hipLaunchKernelGGL(kbb_band_step_update, gy(sh.N, 256, B), dim3(256), 0, s, tab, sh, move ? 1 : 0);
}

void bandb_launch_step_final(hipStream_t s, const BandInst *tab, int B, const BandShape &sh,
                             const double *guard, double *diff_out, int *flags_out, int *rejects,
                             const int *rctl) {
  if (sh.N)
    hipLaunchKernelGGL(kbb_step_final, dim3((B + 3) / 4), dim3(256), 0, s, tab, B, sh, guard, diff_out,
                       flags_out, rejects, rctl);
}

void bandb_launch_refine_decide(hipStream_t s, const BandInst *tab, int B, const BandShape &sh,
                                const double *guard, int *rctl, double *rrel, int *rcnt, int round) {
  if (sh.N)
    hipLaunchKernelGGL(kbb_refine_decide, dim3((B + 3) / 4), dim3(256), 0, s, tab, B, sh, guard, rctl, rrel,
                       rcnt, round);
}

void bandb_launch_refine_load(hipStream_t s, const BandInst *rtab, int B, const BandShape &sh) {
  if (sh.N) hipLaunchKernelGGL(kbb_refine_load, gy(sh.n + sh.m, 256, B), dim3(256), 0, s, rtab, sh);
}

void bandb_launch_refine_axpy(hipStream_t s, const BandInst *rtab, int B, const BandShape &sh) {
  if (sh.N) hipLaunchKernelGGL(kbb_refine_axpy, gy(sh.n + sh.m, 256, B), dim3(256), 0, s, rtab, sh);
}

void bandb_launch_residual(hipStream_t s, const BandInst *rtab, int B, const BandShape &sh) {
  if (sh.N) hipLaunchKernelGGL(kbb_band_residual, gy(sh.N, 256, B), dim3(256), 0, s, rtab, sh);
}
