// Sparse (banded) mode of the step solver: device data and launch wrappers (pgf_sparse.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

struct DenseLdlt;

// One banded handle's device state, in groups of one lifetime each.  Every group that owns memory
// has one release function in pgf_api_band_setup.hip, which frees and nulls its pointers and resets
// its scalars; band_free is those in a row.  Launch wrappers take a const SparseDev &: the counters
// and bor.gram_ready are all they change (mutable).
struct SparseDev {
  bool active = false;  // a pattern is set

  // ---- the pattern (pgf_api_band_setup.hip: pgf_sparse_set_pattern; band_release_pattern) ----
  struct {
    int bw = 0, ldb = 0;
    int nnzH = 0, nnzJ = 0;
    int *pos = nullptr;                       // permuted position of variable i / constraint n + r
    int *Hptr = nullptr, *Hrow = nullptr, *Hcol = nullptr, *Hslot = nullptr;
    int *Jptr = nullptr, *Jcol = nullptr, *Jslot = nullptr;
    int *JTptr = nullptr, *JTrow = nullptr, *JTmap = nullptr;
    double *Hval = nullptr, *Jval = nullptr;
    bool values_set = false;
    uint64_t hash = 0;  // of what pgf_sparse_set_pattern received (pgf_sparse_pattern_hash)
    // (N + 1) x ldb; under a border (Nb + 1) x ldb with C and D behind it (band_declare_border
    // allocates it anew)
    double *band = nullptr;
    double *Hb0 = nullptr, *Jb0 = nullptr;
  } pat;

  // ---- solve vectors and the accuracy guard (pgf_api_band_setup.hip: pgf_sparse_set_pattern, the
  // status block again by band_declare_border; band_release_vectors) ----
  struct {
    double *brhs = nullptr;  // permuted right-hand side / solution, whole B-row blocks
    // the right-hand side as it was, the residual of the solution, a saved solution (refinement)
    double *brhs0 = nullptr, *bres = nullptr, *bsol = nullptr;
    // bred: [0, 2 nred) (max |r|, max |rhs|) per 256 rows, [2 nred, 3 nred) partial sums of the step
    // update (guarded steps), [3 nred, 3 nred + 4) the solve's pivot flags: band_stat_stride(nred)
    double *bred = nullptr;
    double *h_bred = nullptr;   // pinned mirror of bred
    int nred = 0;               // band_nred
    bool guarded = false;       // the last solve carried the residual check
    bool stat_pending = false;  // a guarded step's status block is on its way to h_bred
  } vec;

  // ---- work blocks of the cyclic reduction (pgf_api_band_setup.hip: sp_alloc_blocks, for the
  // pattern, pgf_sparse_set_block_size and pgf_sparse_set_factor_split; band_release_blocks) ----
  struct {
    // block size: 8 (pgf_sparse.hip), 16 / 32 / 64 (pgf_band_wide.hip); never 0 once a pattern is set
    int B = 0;
    // (N/B) blocks of B x B (D, L, U, inv D) and the rhs.  bD, bL, bU, bF hold TWO sets of blocks
    // at B = 8, the second bstride blocks behind the first: a launch that does two levels at once
    // reads one set and writes the other
    int64_t bstride = 0;
    double *bD = nullptr, *bL = nullptr, *bU = nullptr, *bDinv = nullptr, *bF = nullptr;
    int *bneg = nullptr;                      // negative pivots met while inverting block i
    // Factor / solve split of the wide reduction (B > 8): the forward multipliers of the eliminated
    // block e, Mr[e] = L_{e+s} inv(D_e) and Ml[e] = U_{e-s} inv(D_e); allocated only while `split`
    // (the caller's setting: it outlives the blocks) is on.  kept: 0 no factors, 1 a KEEP reduction
    // is enqueued whose pivot flags the host has not seen yet, 2 its flags were clean: solves run
    // the solve phase.
    double *bMr = nullptr, *bMl = nullptr;
    bool split = true;
    int kept = 0;
  } blk;

  // ---- pgf_linear_solve_multi on a wide band (pgf_api_band_setup.hip: band_panel_reserve on the first
  // use; band_release_panel, with the blocks) ---- the panel (whole blocks x 64) and, per column,
  // the residual pairs + flags of k_bw_residual (device and pinned mirror)
  struct {
    double *bP = nullptr, *bredm = nullptr, *h_bredm = nullptr;
  } pan;

  // ---- bordered band (pgf_api_band_setup.hip: band_declare_border behind both border entry points;
  // band_release_border) ----
  // The last bk positions of `pos` are border nodes, the band holds the Nb = n + m - bk others.
  // K = [[B, C], [C', D]]: C (Nb x bkp, row-major) and the lower triangle of D (bkp x bkp; bkp = bk
  // rounded up to 16, padding = identity) lie behind the band array, where the plan's slots point.
  // bk == 0: no border.
  struct {
    int bk = 0, bkp = 0, Nb = 0;
    int bnchunk = 0;                           // chunks of SP_BORDER_CHUNK rows
    double *bC = nullptr, *bDd = nullptr;      // into pat.band (not owned)
    double *bY = nullptr;                      // Y = inv(B) C, whole 8-row blocks x bkp
    double *bS = nullptr;                      // L D L' of S = D - C' Y: L below, 1 / d on the diagonal
    double *bpart = nullptr, *bpartv = nullptr;  // per-chunk sums of C' Y and of (C' v, |C|' |v|, tail of C' v)
    double *brb = nullptr, *bz = nullptr;      // border part of the right-hand side / of the solution
    int *bsflags = nullptr;                    // [0] bad pivot in S, [1] negative pivots of S
    // Large border (pgf_border_large.hip), 65 <= bk <= 1024: bkp = bk rounded up to 64, S = D - C' Y
    // factorised by a dense L D L' of its own on the handle's stream (blf; bS holds the right-hand
    // side of the solve with S, and the one-workgroup kernels of S are not used).  bG: kp x kp, the
    // lower triangle of C' Y (zero above), which survives the factorisation (pgf_debug_border_gram;
    // S itself goes into blf->K alone and is formed again from bpart and D when a factorisation is
    // repeated); bpart: bgchunks partial sums of bgrows rows for each 64 x 64 tile of C' Y's lower
    // triangle.
    DenseLdlt *blf = nullptr;
    double *bG = nullptr;
    int bgrows = 0, bgchunks = 0;
    mutable bool gram_ready = false;  // a factor phase has run since the border was declared
  } bor;

  // ---- phases enqueued, read only by the pgf_debug_* hooks (counted by the launch wrappers) ----
  struct Counters {
    int stat_bw_reduce = 0, stat_bw_solve = 0, stat_bw_panel = 0;  // pgf_debug_band_stats
    int stat_bfactor = 0, stat_bsolve = 0;                         // pgf_debug_border_stats
  };
  mutable Counters cnt;
};
// sp.bor.bkp > 64: the large border's route behind the four entry points below
static inline bool sp_border_large(const SparseDev &sp) { return sp.bor.bkp > 64; }
#define SP_BORDER_CHUNK 512

void sp_launch_spmv(hipStream_t s, int rows, const int *ptr, const int *col, const double *val,
                    const double *x, const double *add, double sgn, double *y);
void sp_launch_spmvT(hipStream_t s, int cols, const int *tptr, const int *trow, const int *tmap,
                     const double *val, const double *w, const double *base, double *out);
// c = J x - b ; w = rho c + y ; g = H x + (q + J' w)
void sp_launch_eval(hipStream_t s, const SparseDev &sp, int n, int m, const double *x, const double *y,
                    const double *b, const double *q, double rho, double *c, double *w, double *g);
void sp_launch_assemble(hipStream_t s, const SparseDev &sp, int n, int m, const uint8_t *mask,
                        double lamb, double delta);
void sp_launch_scatter(hipStream_t s, const SparseDev &sp, const uint8_t *mask);
void sp_launch_rhs(hipStream_t s, const SparseDev &sp, int n, int m, const uint8_t *mask,
                   const double *F, const double *b0full, double fact, double *Hb0, double *Jb0);
// out[pos[i]] = in[i] (gather == 0) or out[i] = in[pos[i]] (gather != 0)
void sp_launch_permute(hipStream_t s, const SparseDev &sp, int N, const double *in, double *out,
                       int gather);
void sp_launch_bcr_solve(hipStream_t s, const SparseDev &sp, int N, int *flags, bool guard = true);
// The launch plan of the 8 x 8 reduction for nb blocks: the levels before the LDS tail in launch
// order (s: stride; set: the block set holding the level's eliminated blocks' L, U, F; pair_set2 >=
// 0: first level of a fused pair whose second level's blocks are in that set), the stride and set
// the tail starts with, and whether a single level is one launch (fused) or invert + reduce.  It
// depends on nb only: sp_launch_bcr_solve and the batched driver (bandb_launch_solve) walk the same.
struct BcrPlan {
  struct Lev {
    int s, set, pair_set2;
  };
  Lev lev[40];
  int nlev = 0;
  int tail_s = 1, tail_set = 0;
  bool fused = true;
};
BcrPlan sp_bcr_plan(int nb);
// workgroups of a level with stride s over nb blocks
static inline int bcr_kept(int nb, int s) { return (nb + 2 * s - 1) / (2 * s); }            // 0, 2s, ...
static inline int bcr_eliminated(int nb, int s) { return (nb - s + 2 * s - 1) / (2 * s); }  // s, 3s, ...
static inline int bcr_pair_groups(int nb, int s) { return (nb + 4 * s - 1) / (4 * s); }     // kept through both: 0, 4s, ...
// j = 2 s + 4 s q with j - s < nb
static inline int bcr_back_pair_groups(int nb, int s) { return (nb + s - 2 * s + 4 * s - 1) / (4 * s); }
void sp_launch_band_residual(hipStream_t s, const SparseDev &sp, int N, const int *flags);
// B = 16, 32, 64 (pgf_band_wide.hip): the same contract as sp_launch_bcr_solve /
// sp_launch_band_residual for half-bandwidths up to 64
// keep: the reduction also leaves its forward multipliers in sp.blk.bMr / sp.blk.bMl (same solution bits)
void sp_launch_bw_solve(hipStream_t s, const SparseDev &sp, int N, int *flags, bool guard,
                        bool keep = false);
// the KEEP reduction without a right-hand side (factors and pivot flags only)
void sp_launch_bw_factor(hipStream_t s, const SparseDev &sp, int N, int *flags);
// solve phase against the kept factors: the right-hand side in sp.vec.brhs / a row-major panel P of kp
// columns (a multiple of 16 up to 64, a multiple of 64 beyond; whole blocks, rows >= N zero), in
// place.  The pivot flags are left as the reduction reported them.
void sp_launch_bw_backsolve(hipStream_t s, const SparseDev &sp, int N, const int *flags, bool guard);
void sp_launch_bw_panel_solve(hipStream_t s, const SparseDev &sp, int N, double *P, int kp);
// column j of a panel: P[pos[i]][j] = in[i] / out[g] = P[g][j]; the residual of sp.vec.brhs against
// sp.vec.brhs0 with its pairs and flags written to `pairs` (3 nred + 4 doubles) instead of sp.vec.bred
void sp_launch_bw_panel_put(hipStream_t s, const SparseDev &sp, int N, const double *in, double *P, int kp,
                            int j);
void sp_launch_bw_panel_get(hipStream_t s, int N, const double *P, int kp, int j, double *out);
void sp_launch_bw_residual_to(hipStream_t s, const SparseDev &sp, int N, const int *flags, double *pairs);
void sp_launch_bw_residual(hipStream_t s, const SparseDev &sp, int N, const int *flags);
void sp_launch_band_axpy(hipStream_t s, int N, const double *a, double *x);
void sp_launch_step_update(hipStream_t s, const SparseDev &sp, int n, int m, double fact,
                           double rho, const double *x, const double *y, const double *lb,
                           const double *ub, const double *F, double *dx, double *dy, double *xn,
                           double *yn, double *red);

// ---- bordered band (pgf_border.hip) ----
// assemble band, C and D for the mask
void sp_border_assemble(hipStream_t s, const SparseDev &sp, int n, int m, const uint8_t *mask,
                        double lamb, double delta);
// factor phase on the assembled matrix: Y = inv(B) C, S = D - C' Y, L D L' of S.  sp.vec.brhs survives.
void sp_border_factor(hipStream_t s, const SparseDev &sp, int *flags);
// solve phase for the right-hand side in sp.vec.brhs (Nb band entries, then bk border entries); the
// solution replaces it.  flags[0] zero pivot, flags[1] negative pivots of B plus those of S.
// guard: keep the right-hand side and finish with the residual over all Nb + bk rows.
void sp_border_solve(hipStream_t s, const SparseDev &sp, int *flags, bool guard);
void sp_border_residual(hipStream_t s, const SparseDev &sp, const int *flags);
// ---- large border (pgf_border_large.hip): the same three phases for sp.bor.bkp > 64, reached through
// the entry points above (assembly is shared: the store has the same shape)
// the wide remainder's halves of the two phases, shared with pgf_border.hip: the kept factors of B
// with its flags parked and Y = inv(B) C / v = inv(B) ra in sp.vec.brhs with the flags of B put back
void sp_border_wide_Y(hipStream_t s, const SparseDev &sp, int *flags);
void sp_border_wide_v(hipStream_t s, const SparseDev &sp, int *flags);
void sp_borderL_factor(hipStream_t s, const SparseDev &sp, int *flags);
void sp_borderL_solve(hipStream_t s, const SparseDev &sp, int *flags, bool guard);
void sp_borderL_residual(hipStream_t s, const SparseDev &sp, const int *flags);
// rows per chunk and chunks of the Gram kernel for Nb rows and kp columns (the partial sums stay
// below 256 MB)
void sp_borderL_gram_plan(int Nb, int kp, int *rows, int *chunks);
void sp_border_gram_fma(hipStream_t s, const SparseDev &sp);  // k_border_gram alone (kp <= 64)
// device time per launch of the two Gram kernels on the last factor phase's C and Y (kp % 64 == 0;
// *ms_fma = -1 for kp > 64)
hipError_t sp_borderL_gram_time(hipStream_t s, const SparseDev &sp, int reps, double *ms_mfma, double *ms_fma);
