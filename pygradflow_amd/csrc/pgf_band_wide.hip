// Wide block cyclic reduction of the banded KKT system: half-bandwidths 11 .. 64 (or any
// bw <= B on request), B x B blocks with B in {16, 32, 64}.
//
// Same algorithm as the 8 x 8 code in pgf_sparse.hip (see the comment above k_bcr_extract):
// with B >= bw the permuted band is block tridiagonal, D_i (diagonal), L_i (coupling to the
// left neighbour), U_i = L_{i+1}^T.  Each level eliminates every other block row:
//   kept block i, eliminated neighbours i-s, i+s:
//     alpha = L_i inv(D_{i-s}),  gamma = U_i inv(D_{i+s})
//     D_i -= alpha U_{i-s} + gamma L_{i+s};  f_i -= alpha f_{i-s} + gamma f_{i+s}
//     L_i <- -alpha L_{i-s};  U_i <- -gamma U_{i+s}
// The eliminated blocks are inverted without pivoting (Gauss-Jordan; every principal block and
// Schur complement of a symmetric permutation of a quasi-definite matrix is quasi-definite, and
// the residual guard catches the rest).  Their pivots give the inertia (Haynsworth additivity),
// counted per block in negcnt[i] and summed once at the end.
//
// Differences from the 8 x 8 code:
//   * one 256-thread workgroup per block; the B x B x B products run on v_mfma_f64_16x16x4_f64
//     (one 16 x 16 output tile per wavefront and pass: 1, 4 or 16 tiles for B = 16, 32, 64);
//   * no LDS-resident tail: a 64 x 64 f64 block is 32 KiB, so the 32-block tail of the 8 x 8
//     code would need 4 MiB.  The levels run down to ONE block (tail threshold 1 for every B),
//     and that block is inverted and solved by a single workgroup (k_bw_last);
//   * one level per launch pair (invert, then reduce): at B >= 16 the block count, and with it
//     the number of levels, is 2 .. 8 x smaller than at B = 8, and the levels do real
//     arithmetic rather than being bound by their launch.
//
// Factor / solve split.  A block e != 0 is eliminated at exactly one level s; from then on
// inv(D_e), L_e, U_e (its couplings to e -+ s at that level) are final, and so are the two forward
// multipliers that the kept neighbours formed from it:
//   Mr[e] = L_{e+s} inv(D_e)   (used by the kept block e + s)
//   Ml[e] = U_{e-s} inv(D_e)   (used by the kept block e - s)
// The KEEP variant of k_bw_reduce stores them (2 B^2 doubles per block; the arithmetic of D, L, U, F
// is untouched), and a solve against the kept factors (sp_launch_bw_backsolve, one right-hand side;
// sp_launch_bw_panel_solve, a panel of them on the matrix pipes) runs no inversion:
//   forward, per level: f_i -= Mr[i-s] f_{i-s} + Ml[i+s] f_{i+s} for the kept blocks i;
//   x_0 = inv(D_0) f_0;  backward, per level: k_bw_back as in the fused solve.
// The single right-hand side forward step shares bw_f_dot with k_bw_reduce, so it returns the bits
// of the fused reduction.  Without kept factors every solve re-runs the reduction on the intact
// band, as the 8 x 8 code does.
//
// Block storage (one set): D, L, U, inv D, Mr, Ml row-major B x B at block * B * B; F at block * B.
//
// The bodies of the kernels live in pgf_band_wide_dev.h as device functions; the kernels here and
// their batched twins (the second half of this file) are thin callers of the same functions.
#include "pgf_band_wide_dev.h"
#include "pgf_sparse.h"

// block extraction from the band (+ identity padding of the last block); the right-hand side
// is copied to F and, for the guard, to rhs0
template <int B>
__global__ __launch_bounds__(BW_THREADS) void k_bw_extract(const double *__restrict__ band, int ldb,
                                                           int bw, const double *__restrict__ rhs,
                                                           int N, int nb, double *__restrict__ D,
                                                           double *__restrict__ L,
                                                           double *__restrict__ U,
                                                           double *__restrict__ F,
                                                           double *__restrict__ rhs0,
                                                           int *__restrict__ flags) {
  const int i = blockIdx.x;
  bw_extract_matrix<B>(band, ldb, bw, N, nb, D, L, U, flags, i);
  bw_extract_rhs<B>(rhs, N, F, rhs0, i);
}

// invert the blocks eliminated at this level: i = first, first + stride, ...
template <int B>
__global__ __launch_bounds__(BW_THREADS) void k_bw_invert(const double *__restrict__ D,
                                                          double *__restrict__ Dinv, int nb,
                                                          int first, int stride,
                                                          int *__restrict__ flags,
                                                          int *__restrict__ negcnt) {
  __shared__ double M[B * (B + 1)];
  const int i = first + blockIdx.x * stride;
  if (i >= nb) return;
  bw_invert_block<B>(D, Dinv, i, M, flags, negcnt);
}

// Reduce the kept blocks of this level: i = 0, 2s, 4s, ... (bw_reduce_block)
template <int B, bool KEEP, bool RHS>
__global__ __launch_bounds__(BW_THREADS) void k_bw_reduce(double *__restrict__ D, double *__restrict__ L,
                                                          double *__restrict__ U, double *__restrict__ F,
                                                          const double *__restrict__ Dinv,
                                                          double *__restrict__ Mr, double *__restrict__ Ml,
                                                          int nb, int s) {
  __shared__ double T[B * (B + 1)];  // alpha, then gamma
  const int i = blockIdx.x * 2 * s;
  if (i >= nb) return;
  bw_reduce_block<B, KEEP, RHS>(D, L, U, F, Dinv, Mr, Ml, nb, s, i, T);
}

template <int B>
__global__ __launch_bounds__(BW_THREADS) void k_bw_back(const double *__restrict__ Dinv,
                                                        const double *__restrict__ L,
                                                        const double *__restrict__ U,
                                                        const double *__restrict__ F,
                                                        double *__restrict__ X, int nb, int s) {
  __shared__ double xl[B], xr[B], t[B];
  const int i = s + blockIdx.x * 2 * s;
  if (i >= nb) return;
  bw_back_block<B>(Dinv, L, U, F, X, nb, s, i, xl, xr, t);
}

// the last block left (block 0): invert, solve, and sum the per-block negative pivots
template <int B>
__global__ __launch_bounds__(BW_THREADS) void k_bw_last(const double *__restrict__ D,
                                                        double *__restrict__ Dinv,
                                                        const double *__restrict__ F,
                                                        double *__restrict__ X, int nb,
                                                        int *__restrict__ flags,
                                                        int *__restrict__ negcnt) {
  __shared__ double M[B * (B + 1)];
  __shared__ double t[B];
  __shared__ int part[BW_THREADS / 64];
  bw_last_block<B>(D, Dinv, F, X, nb, flags, negcnt, M, t, part);
}

// ---- solve phase against the kept factors, one right-hand side ----
// F <- the right-hand side in whole blocks (zero padding), rhs0 <- its copy for the guard
__global__ __launch_bounds__(256) void k_bw_load(const double *__restrict__ rhs, int N, int nrows,
                                                 double *__restrict__ F, double *__restrict__ rhs0) {
  bw_load_row(rhs, N, nrows, F, rhs0, blockIdx.x * 256 + threadIdx.x);
}

// forward step of one level for the kept blocks i = 0, 2s, ... (bw_fwd_block)
template <int B>
__global__ __launch_bounds__(BW_THREADS) void k_bw_fwd(const double *__restrict__ Mr,
                                                       const double *__restrict__ Ml,
                                                       double *__restrict__ F, int nb, int s) {
  __shared__ double T[B * (B + 1)];
  const int i = blockIdx.x * 2 * s;
  if (i >= nb) return;
  bw_fwd_block<B>(Mr, Ml, F, nb, s, i, T);
}

// x_0 = inv(D_0) f_0 (the operation order of k_bw_last's product)
template <int B>
__global__ __launch_bounds__(BW_THREADS) void k_bw_x0(const double *__restrict__ Dinv,
                                                      const double *__restrict__ F,
                                                      double *__restrict__ X) {
  __shared__ double t[B];
  bw_x0_block<B>(Dinv, F, X, t);
}

// ---- solve phase against the kept factors, a panel of kp right-hand sides (bw_fwd_panel_block,
// bw_back_panel_block in pgf_band_wide_dev.h describe the layout and the tiles), in place.
//
// In place without races (the argument of k_mbcr_level, pgf_sparse.hip): forward, a kept block
// writes only its own rows and reads rows of blocks eliminated at its level, which no block of
// that launch writes; backward, an eliminated block writes only its own rows and reads rows of
// blocks solved at earlier launches.
template <int B>
__global__ __launch_bounds__(BW_THREADS) void k_bw_fwd_panel(const double *__restrict__ Mr,
                                                             const double *__restrict__ Ml,
                                                             double *__restrict__ P, int ld, int kp,
                                                             int nb, int s) {
  const int i = blockIdx.x * 2 * s;
  if (i >= nb) return;
  // slice blockIdx.y: columns [64 y, 64 y + kp) of a panel with row stride ld
  bw_fwd_panel_block<B>(Mr, Ml, P + 64 * blockIdx.y, ld, kp, nb, s, i);
}

// X_e = inv(D_e) (F_e - L_e X_{e-s} - U_e X_{e+s}) for e = first, first + stride, ...; s == 0: the
// last block, no neighbours (bw_back_panel_block).
template <int B>
__global__ __launch_bounds__(BW_THREADS) void k_bw_back_panel(const double *__restrict__ Dinv,
                                                              const double *__restrict__ L,
                                                              const double *__restrict__ U,
                                                              double *__restrict__ P, int ld, int kp,
                                                              int nb, int s, int first, int stride) {
  __shared__ double T[B * 65];
  const int e = first + blockIdx.x * stride;
  if (e >= nb) return;
  bw_back_panel_block<B>(Dinv, L, U, P + 64 * blockIdx.y, ld, kp, nb, s, e, T);
}
// Accuracy guard for bw <= 64 (bw_residual_rows)
__global__ __launch_bounds__(256) void k_bw_residual(const double *__restrict__ band, int ldb, int bw,
                                                     int N, const double *__restrict__ x,
                                                     const double *__restrict__ rhs0,
                                                     double *__restrict__ r,
                                                     double *__restrict__ rsmax,
                                                     const int *__restrict__ flags, int nred) {
  __shared__ double pr[4], pb[4];
  bw_residual_rows(band, ldb, bw, N, x, rhs0, r, rsmax, flags, nred, blockIdx.x, pr, pb);
}

void sp_launch_bw_residual(hipStream_t s, const SparseDev &sp, int N, const int *flags) {
  if (N == 0) return;
  hipLaunchKernelGGL(k_bw_residual, dim3((N + 255) / 256), dim3(256), 0, s, sp.pat.band, sp.pat.ldb, sp.pat.bw, N,
                     sp.vec.brhs, sp.vec.brhs0, sp.vec.bres, sp.vec.bred, flags, sp.vec.nred);
}

// the fused reduction (+ solve when with_rhs); keep: the KEEP variant, which leaves the factors
template <int B>
static void bw_solve(hipStream_t s, const SparseDev &sp, int N, int *flags, bool guard, bool keep,
                     bool with_rhs) {
  const int nb = (N + B - 1) / B;
  const dim3 blk(BW_THREADS);
  ++sp.cnt.stat_bw_reduce;
  // (the extraction always fills F; a factor-only reduction just does not carry it along)
  hipLaunchKernelGGL(k_bw_extract<B>, dim3(nb), blk, 0, s, sp.pat.band, sp.pat.ldb, sp.pat.bw, sp.vec.brhs, N, nb, sp.blk.bD,
                     sp.blk.bL, sp.blk.bU, sp.blk.bF, guard ? sp.vec.brhs0 : nullptr, flags);
  int levels[32], nlev = 0;
  for (int st = 1; st < nb; st *= 2) {
    const int ne = (nb - st + 2 * st - 1) / (2 * st);  // eliminated: st, 3st, ...
    const int nk = (nb + 2 * st - 1) / (2 * st);       // kept: 0, 2st, ...
    hipLaunchKernelGGL(k_bw_invert<B>, dim3(ne), blk, 0, s, sp.blk.bD, sp.blk.bDinv, nb, st, 2 * st, flags, sp.blk.bneg);
    if (!with_rhs)
      hipLaunchKernelGGL((k_bw_reduce<B, true, false>), dim3(nk), blk, 0, s, sp.blk.bD, sp.blk.bL, sp.blk.bU, sp.blk.bF,
                         sp.blk.bDinv, sp.blk.bMr, sp.blk.bMl, nb, st);
    else if (keep)
      hipLaunchKernelGGL((k_bw_reduce<B, true, true>), dim3(nk), blk, 0, s, sp.blk.bD, sp.blk.bL, sp.blk.bU, sp.blk.bF,
                         sp.blk.bDinv, sp.blk.bMr, sp.blk.bMl, nb, st);
    else
      hipLaunchKernelGGL((k_bw_reduce<B, false, true>), dim3(nk), blk, 0, s, sp.blk.bD, sp.blk.bL, sp.blk.bU, sp.blk.bF,
                         sp.blk.bDinv, nullptr, nullptr, nb, st);
    levels[nlev++] = st;
  }
  // (factor-only: the last block's product goes to the spare block behind F and is not used)
  hipLaunchKernelGGL(k_bw_last<B>, dim3(1), blk, 0, s, sp.blk.bD, sp.blk.bDinv, sp.blk.bF,
                     with_rhs ? sp.vec.brhs : sp.blk.bF + (int64_t)nb * B, nb, flags, sp.blk.bneg);
  if (!with_rhs) return;
  for (int q = nlev - 1; q >= 0; --q) {
    const int st = levels[q];
    const int ne = (nb - st + 2 * st - 1) / (2 * st);
    hipLaunchKernelGGL(k_bw_back<B>, dim3(ne), blk, 0, s, sp.blk.bDinv, sp.blk.bL, sp.blk.bU, sp.blk.bF, sp.vec.brhs, nb, st);
  }
  if (guard) sp_launch_bw_residual(s, sp, N, flags);
}

template <int B>
static void bw_backsolve(hipStream_t s, const SparseDev &sp, int N, const int *flags, bool guard) {
  const int nb = (N + B - 1) / B;
  const dim3 blk(BW_THREADS);
  ++sp.cnt.stat_bw_solve;
  hipLaunchKernelGGL(k_bw_load, dim3((nb * B + 255) / 256), dim3(256), 0, s, sp.vec.brhs, N, nb * B, sp.blk.bF,
                     guard ? sp.vec.brhs0 : nullptr);
  int levels[32], nlev = 0;
  for (int st = 1; st < nb; st *= 2) {
    const int nk = (nb + 2 * st - 1) / (2 * st);
    hipLaunchKernelGGL(k_bw_fwd<B>, dim3(nk), blk, 0, s, sp.blk.bMr, sp.blk.bMl, sp.blk.bF, nb, st);
    levels[nlev++] = st;
  }
  hipLaunchKernelGGL(k_bw_x0<B>, dim3(1), blk, 0, s, sp.blk.bDinv, sp.blk.bF, sp.vec.brhs);
  for (int q = nlev - 1; q >= 0; --q) {
    const int st = levels[q];
    const int ne = (nb - st + 2 * st - 1) / (2 * st);
    hipLaunchKernelGGL(k_bw_back<B>, dim3(ne), blk, 0, s, sp.blk.bDinv, sp.blk.bL, sp.blk.bU, sp.blk.bF, sp.vec.brhs, nb, st);
  }
  if (guard) sp_launch_bw_residual(s, sp, N, flags);
}

template <int B>
static void bw_panel_solve(hipStream_t s, const SparseDev &sp, int N, double *P, int kp) {
  const int nb = (N + B - 1) / B;
  const dim3 blk(BW_THREADS);
  ++sp.cnt.stat_bw_panel;
  // a panel wider than 64 columns (a multiple of 64 then): one 64-column slice per blockIdx.y, in
  // the same launches -- the slices share the factors and nothing else
  const int ld = kp, kw = kp > 64 ? 64 : kp;
  const unsigned ns = (unsigned)((kp + 63) / 64);
  int levels[32], nlev = 0;
  for (int st = 1; st < nb; st *= 2) {
    const int nk = (nb + 2 * st - 1) / (2 * st);
    hipLaunchKernelGGL(k_bw_fwd_panel<B>, dim3(nk, ns), blk, 0, s, sp.blk.bMr, sp.blk.bMl, P, ld, kw, nb, st);
    levels[nlev++] = st;
  }
  hipLaunchKernelGGL(k_bw_back_panel<B>, dim3(1, ns), blk, 0, s, sp.blk.bDinv, sp.blk.bL, sp.blk.bU, P, ld, kw, nb, 0, 0, 1);
  for (int q = nlev - 1; q >= 0; --q) {
    const int st = levels[q];
    const int ne = (nb - st + 2 * st - 1) / (2 * st);
    hipLaunchKernelGGL(k_bw_back_panel<B>, dim3(ne, ns), blk, 0, s, sp.blk.bDinv, sp.blk.bL, sp.blk.bU, P, ld, kw, nb, st,
                       st, 2 * st);
  }
}

// Solve the banded system in sp.pat.band / sp.vec.brhs with B = sp.blk.B x sp.blk.B blocks (16, 32, 64); the
// solution replaces sp.vec.brhs (which holds whole blocks).  flags[0] zero pivot, flags[1]
// negative pivots; guard: keep the right-hand side and finish with the residual (bres, bred).
// keep: also leave the forward multipliers in sp.blk.bMr / sp.blk.bMl (the same solution, bit for bit).
void sp_launch_bw_solve(hipStream_t s, const SparseDev &sp, int N, int *flags, bool guard, bool keep) {
  if (N == 0) {
    (void)hipMemsetAsync(flags, 0, 4 * sizeof(int), s);
    return;
  }
  switch (sp.blk.B) {
    case 16: bw_solve<16>(s, sp, N, flags, guard, keep, true); break;
    case 32: bw_solve<32>(s, sp, N, flags, guard, keep, true); break;
    default: bw_solve<64>(s, sp, N, flags, guard, keep, true); break;
  }
}

// The KEEP reduction without a right-hand side: factors and pivot flags only; sp.vec.brhs survives.
void sp_launch_bw_factor(hipStream_t s, const SparseDev &sp, int N, int *flags) {
  if (N == 0) {
    (void)hipMemsetAsync(flags, 0, 4 * sizeof(int), s);
    return;
  }
  switch (sp.blk.B) {
    case 16: bw_solve<16>(s, sp, N, flags, false, true, false); break;
    case 32: bw_solve<32>(s, sp, N, flags, false, true, false); break;
    default: bw_solve<64>(s, sp, N, flags, false, true, false); break;
  }
}

// Solve phase against the factors a KEEP reduction left, for the right-hand side in sp.vec.brhs: load,
// one forward launch per level, x_0, one backward launch per level (2 levels + 3 launches with the
// guard's residual; no inversion, no MFMA).  The pivot flags stay what the reduction reported.
void sp_launch_bw_backsolve(hipStream_t s, const SparseDev &sp, int N, const int *flags, bool guard) {
  if (N == 0) return;
  switch (sp.blk.B) {
    case 16: bw_backsolve<16>(s, sp, N, flags, guard); break;
    case 32: bw_backsolve<32>(s, sp, N, flags, guard); break;
    default: bw_backsolve<64>(s, sp, N, flags, guard); break;
  }
}

// column j of the panel <-> a vector: P[pos[i]][j] = in[i] (natural order in, put), and
// out[g] = P[g][j] (permuted order out, get)
__global__ __launch_bounds__(256) void k_bw_panel_put(int N, const int *__restrict__ pos,
                                                      const double *__restrict__ in,
                                                      double *__restrict__ P, int kp, int j) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < N) P[(int64_t)pos[i] * kp + j] = in[i];
}
__global__ __launch_bounds__(256) void k_bw_panel_get(int N, const double *__restrict__ P, int kp, int j,
                                                      double *__restrict__ out) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g < N) out[g] = P[(int64_t)g * kp + j];
}
void sp_launch_bw_panel_put(hipStream_t s, const SparseDev &sp, int N, const double *in, double *P, int kp,
                            int j) {
  if (N) hipLaunchKernelGGL(k_bw_panel_put, dim3((N + 255) / 256), dim3(256), 0, s, N, sp.pat.pos, in, P, kp, j);
}
void sp_launch_bw_panel_get(hipStream_t s, int N, const double *P, int kp, int j, double *out) {
  if (N) hipLaunchKernelGGL(k_bw_panel_get, dim3((N + 255) / 256), dim3(256), 0, s, N, P, kp, j, out);
}
// the guard's residual of sp.vec.brhs against sp.vec.brhs0 with the pairs written to `pairs`
void sp_launch_bw_residual_to(hipStream_t s, const SparseDev &sp, int N, const int *flags, double *pairs) {
  if (N == 0) return;
  hipLaunchKernelGGL(k_bw_residual, dim3((N + 255) / 256), dim3(256), 0, s, sp.pat.band, sp.pat.ldb, sp.pat.bw, N,
                     sp.vec.brhs, sp.vec.brhs0, sp.vec.bres, pairs, flags, sp.vec.nred);
}

// Solve phase for a panel: P is (nb B) x kp row-major, kp a multiple of 16 up to 64 or a multiple
// of 64 beyond (64-column slices on blockIdx.y of the same launches), rows >= N zero on entry; the
// solutions replace the right-hand sides.
void sp_launch_bw_panel_solve(hipStream_t s, const SparseDev &sp, int N, double *P, int kp) {
  if (N == 0) return;
  switch (sp.blk.B) {
    case 16: bw_panel_solve<16>(s, sp, N, P, kp); break;
    case 32: bw_panel_solve<32>(s, sp, N, P, kp); break;
    default: bw_panel_solve<64>(s, sp, N, P, kp); break;
  }
}

// ================================================================= banded device batch, wide route
// The kernels of the wide block cyclic reduction above with a batch dimension.  Every kernel here is
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
// factors (SparseDev::blk.kept == 2).  So every twin branches on ctl[0]:
//
//   twin of    ctl[0] != 0, or split off            ctl[0] == 0 and split on
//   extract    whole extraction                     right-hand side part only (k_bw_load's work)
//   invert     invert                               return
//   reduce     k_bw_reduce<B, KEEP = split, true>   k_bw_fwd (same grid: the kept blocks of the level)
//   last       k_bw_last                            k_bw_x0
//   back, residual: the same in both phases
//
// The solve phase returns the bits of the fused reduction (the head of this file), so either branch
// agrees with whatever the single handle did.  A frozen instance (ctl[3]) returns at once everywhere.
// Thread 0 of the extraction's block 0 counts the instance's reductions and solve phases (wcnt).
//
// A bordered batch on the wide route (pgf_border.hip) needs the two phases apart, in one step
// and for different sets of instances, while ctl[0] stays set: the factor-only reduction of B where
// ctl[0] != 0, later the solve against the kept factors for every live instance.  The twins that
// branch therefore take the phase as a template argument (BW_BY_CTL / BW_FACTOR / BW_SOLVE below);
// the unbordered batch launches the BW_BY_CTL instantiations, whose code is what it was.  The panel
// solve Y <- inv(B) Y of the factor phase has its own twins, kbw_fwd_panel / kbw_back_panel.
//
// The twins see the contraction rules of the kernels they mirror: this file is compiled WITHOUT
// -ffp-contract=off.
#include "pgf_band_batch.h"

#define INST(I)                        \
  const BandInst &I = tab[blockIdx.y]; \
  if (I.ctl[3]) return /* frozen: sits this step out */

// Phase selector, a template argument of the twins that branch: which of the two phases an instance
// runs is read from ctl[0] (BW_BY_CTL: the unbordered wide batch, one launch sequence for both), or
// fixed by the caller -- the bordered wide route (pgf_border.hip) runs the factor-only KEEP
// reduction of B for the instances with ctl[0] != 0 (BW_FACTOR) and, later in the SAME step, while
// ctl[0] is still set, the solve phase against the kept factors for every live instance (BW_SOLVE).
// The BW_BY_CTL instantiations are the kernels the unbordered batch has always launched.
// BW_NO_GUARD: BW_BY_CTL's extraction without the guard's copy of the right-hand side, for a
// refinement round with the split off (sp_launch_bw_solve with guard == false); the other twins of
// such a round are the BW_BY_CTL ones.
enum { BW_BY_CTL = 0, BW_FACTOR = 1, BW_SOLVE = 2, BW_NO_GUARD = 3 };

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
  bw_extract_rhs<B>(I.brhs, sh.N, I.bF, PHASE == BW_NO_GUARD ? nullptr : I.brhs0, i);
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
  bw_fwd_panel_block<B>(I.bMr, I.bMl, I.bY, sh.bkp, sh.bkp, sh.nb, s, i);
}

template <int B>
__global__ __launch_bounds__(BW_THREADS) void kbw_back_panel(const BandInst *__restrict__ tab, BandShape sh,
                                                             int s, int first, int stride) {
  const BandInst &I = tab[blockIdx.y];
  if (I.ctl[0] == 0) return;
  __shared__ double T[B * 65];
  const int e = first + blockIdx.x * stride;
  if (e >= sh.nb) return;
  bw_back_panel_block<B>(I.bDinv, I.bL, I.bU, I.bY, sh.bkp, sh.bkp, sh.nb, s, e, T);
}

// the walk of bw_solve / bw_backsolve (pgf_band_wide.hip), every launch with the instances in grid.y;
// lean: no instance reduces (the host knows), so the inversion launches are left out
template <int B>
static void bandb_wide_solve(hipStream_t s, const BandInst *tab, int Bi, const BandShape &sh, bool lean,
                             bool guard) {
  const int nb = sh.nb;
  const unsigned Bu = (unsigned)Bi;
  const dim3 blk(BW_THREADS);
  if (guard)
    hipLaunchKernelGGL((kbw_extract<B, BW_BY_CTL>), dim3(nb, Bu), blk, 0, s, tab, sh);
  else
    hipLaunchKernelGGL((kbw_extract<B, BW_NO_GUARD>), dim3(nb, Bu), blk, 0, s, tab, sh);
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
  if (guard) hipLaunchKernelGGL(kbw_residual, dim3((sh.N + 255) / 256, Bu), dim3(256), 0, s, tab, sh);
}

void bandb_launch_wide_solve(hipStream_t s, const BandInst *tab, int B, const BandShape &sh, bool lean,
                             bool guard) {
  if (!sh.N) return;
  switch (sh.B) {
    case 16: bandb_wide_solve<16>(s, tab, B, sh, lean, guard); break;
    case 32: bandb_wide_solve<32>(s, tab, B, sh, lean, guard); break;
    default: bandb_wide_solve<64>(s, tab, B, sh, lean, guard); break;
  }
}

void bandb_launch_wide_residual(hipStream_t s, const BandInst *tab, int B, const BandShape &sh) {
  if (sh.N) hipLaunchKernelGGL(kbw_residual, dim3((sh.N + 255) / 256, (unsigned)B), dim3(256), 0, s, tab, sh);
}

// ---- bordered wide route: the band part of pgf_border.hip's two batch phases -----------------------
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
