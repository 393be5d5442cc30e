// The banded batch: the per-instance table (BandInst), the shared shape (BandShape) and the
// launchers of the batched twins in pgf_sparse.hip, pgf_band_wide.hip and pgf_border.hip.
// gfx950 (MI355X / CDNA4) only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgf_sparse.h"

// ---- banded batch (pgf_sparse.hip, pgf_band_wide.hip, pgf_border.hip) ----------
// One entry per banded instance: what differs between the instances of a batch of banded handles
// (ONE sparsity pattern; block size 8, with the same border of up to 64 nodes or none, or 16 / 32 / 64
// for every instance -- the wide route) -- the values of H and J, the band, the work blocks of the
// cyclic reduction, the vectors, the flags.  The pattern arrays, equal by construction, come from
// instance 0 (BandShape) so that every workgroup hits the same lines.  The batched twins of the banded
// kernels (the second halves of pgf_sparse.hip, pgf_band_wide.hip, pgf_border.hip) pick their
// instance with blockIdx.y; the vector kernels shared with the dense batch (kb_advance,
// kb_mask_adopt, kb_residual, ...) read the same instance from the BInst table beside it.  ctl, ps:
// as in BInst (ctl[0]: assemble the band this step).
struct BandInst {
  const double *Hval, *Jval;
  double *band, *brhs, *brhs0, *bres;
  double *bsol;  // the solution a refinement round keeps (PGF_BATCH_CTL_REFINE; SparseDev::vec.bsol)
  double *bD, *bL, *bU, *bDinv, *bF;  // two block sets, bstride blocks apart (SparseDev::blk; wide: one)
  double *bMr, *bMl;                  // wide route with the factor / solve split: the kept multipliers
  int *bneg, *flags;
  int *wcnt;  // wide route: [0] reductions, [1] solve phases this instance's workgroups ran
  // bordered routes, narrow and wide (pgf_border.hip; SparseDev names them): C and D behind
  // the band, Y (whole B-row blocks on the wide route),
  // the factor of S, the chunk sums, the border part of the right-hand side / solution, the flags
  // of S; bcnt: [0] factor phases, [1] solve phases this instance ran
  double *bC, *bDd, *bY, *bS, *bpart, *bpartv, *brb, *bz;
  int *bsflags, *bcnt;
  // the instance's slice of the batch's status block: [0, 2 nred) residual pairs, [2 nred, 3 nred)
  // partial sums of the step update, [3 nred, 3 nred + 4) pivot flags (as SparseDev::vec.bred)
  double *stat;
  const double *lb, *ub, *q, *b;
  double *x, *y, *xn, *yn, *g, *c, *w, *F, *b0full, *dx, *dy, *tmpn;
  const uint8_t *mask;
  const int *counts;  // [0] |I| (reported by kbb_step_final, as kb_step_final does)
  int *ctl;
  const double *ps;
};
struct BandShape {
  int n, m, N, nb, bw, ldb, nnzH, nnzJ, nred;
  int B, split;  // block size of the reduction; wide route: the factor / solve split is on
  // bordered band (bk != 0): N = n + m is the size of the vector kernels, the reduction runs over
  // the Nb = N - bk band rows, nred = max(ceil(N / 256), ceil(Nb / 256) + 1) as on the handle
  int bk, bkp, Nb, bnchunk;
  int64_t bstride;
  const int *pos, *Hptr, *Hrow, *Hcol, *Hslot, *Jptr, *Jcol, *Jslot, *JTptr, *JTrow, *JTmap;
};
// The SparseDev part of a BandInst: the arrays of one handle.  flags: where the reduction reports
// its pivots; stat: where the residual pairs go (SparseDev::vec.bred, or a batch's status slice).  The
// vectors of the step, ctl, ps and the counters stay null: band_batch_create adds them.
inline BandInst band_inst_of(const SparseDev &sp, int *flags, double *stat) {
  BandInst u{};
  u.Hval = sp.pat.Hval;
  u.Jval = sp.pat.Jval;
  u.band = sp.pat.band;
  u.brhs = sp.vec.brhs;  // (the back-substitution writes the solution there)
  u.brhs0 = sp.vec.brhs0;
  u.bres = sp.vec.bres;
  u.bsol = sp.vec.bsol;
  u.bD = sp.blk.bD;
  u.bL = sp.blk.bL;
  u.bU = sp.blk.bU;
  u.bDinv = sp.blk.bDinv;
  u.bF = sp.blk.bF;
  u.bMr = sp.blk.bMr;
  u.bMl = sp.blk.bMl;
  u.bneg = sp.blk.bneg;
  u.flags = flags;
  u.bC = sp.bor.bC;
  u.bDd = sp.bor.bDd;
  u.bY = sp.bor.bY;
  u.bS = sp.bor.bS;
  u.bpart = sp.bor.bpart;
  u.bpartv = sp.bor.bpartv;
  u.brb = sp.bor.brb;
  u.bz = sp.bor.bz;
  u.bsflags = sp.bor.bsflags;
  u.stat = stat;
  return u;
}
// The SparseDev part of a BandShape for a reduction over N rows (n + m, or the Nb band rows under a
// border); n and m are the caller's.  split: the factor / solve split is in force only where the
// multipliers are allocated.  sp.blk.B is the block size of a pattern that is set (8, 16, 32 or 64), never
// the 0 of a fresh SparseDev.
inline BandShape band_shape_of(const SparseDev &sp, int N) {
  BandShape sh{};
  sh.N = N;
  sh.B = sp.blk.B;
  sh.split = (sp.blk.B > 8 && sp.blk.split && sp.blk.bMr) ? 1 : 0;
  sh.nb = (N + sp.blk.B - 1) / sp.blk.B;
  sh.bw = sp.pat.bw;
  sh.ldb = sp.pat.ldb;
  sh.nnzH = sp.pat.nnzH;
  sh.nnzJ = sp.pat.nnzJ;
  sh.nred = sp.vec.nred;
  sh.bk = sp.bor.bk;
  sh.bkp = sp.bor.bkp;
  sh.Nb = sp.bor.bk ? sp.bor.Nb : N;
  sh.bnchunk = sp.bor.bnchunk;
  sh.bstride = sp.blk.bstride;
  sh.pos = sp.pat.pos;
  sh.Hptr = sp.pat.Hptr;
  sh.Hrow = sp.pat.Hrow;
  sh.Hcol = sp.pat.Hcol;
  sh.Hslot = sp.pat.Hslot;
  sh.Jptr = sp.pat.Jptr;
  sh.Jcol = sp.pat.Jcol;
  sh.Jslot = sp.pat.Jslot;
  sh.JTptr = sp.pat.JTptr;
  sh.JTrow = sp.pat.JTrow;
  sh.JTmap = sp.pat.JTmap;
  return sh;
}
// ---- narrow route and the vector kernels (pgf_sparse.hip) ----------------------
// c, w, g at every instance's point
void bandb_launch_eval(hipStream_t s, const BandInst *tab, int B, const BandShape &sh);
// permuted right-hand side from F, b0full (kb_residual before it)
void bandb_launch_rhs(hipStream_t s, const BandInst *tab, int B, const BandShape &sh);
// band of the instances with ctl[0] != 0: zero, diagonal, entries of H and J
void bandb_launch_assemble(hipStream_t s, const BandInst *tab, int B, const BandShape &sh);
// cyclic reduction of every instance that is not frozen (one launch plan: it depends on N only),
// then the residual of the solution into the status block (residual == false: left out; the
// bordered route reduces over sh.N = Nb rows and has a residual of its own)
// save_rhs == false: the extraction leaves brhs0 alone (sp_launch_bcr_solve with the guard off: a
// refinement round, whose brhs0 still holds the step's right-hand side)
void bandb_launch_solve(hipStream_t s, const BandInst *tab, int B, const BandShape &sh, bool residual = true,
                        bool save_rhs = true);
// ---- bordered routes (pgf_border.hip; both wrappers branch on sh.B > 8) --------
// Factor phase of the
// instances with ctl[0] != 0: band, C and D cleared and assembled, Y = inv(B) C by the panel reduction
// (wide: B factorised once, Y by one panel solve against the kept factors), S and its factor.
void borderb_launch_factor(hipStream_t s, const BandInst *tab, int B, const BandShape &sh);
// solve phase of every instance that is not frozen, guard included: the border part of the
// right-hand side and the whole of it saved, the 8 x 8 reduction of B (wide: the solve against the
// kept factors), z, x_a, the residual
// guard == false (a refinement round): brhs0 is not saved and the residual is left out
// (borderb_launch_residual is sp_border_residual's twin)
void borderb_launch_solve(hipStream_t s, const BandInst *tab, int B, const BandShape &sh, bool guard = true);
void borderb_launch_residual(hipStream_t s, const BandInst *tab, int B, const BandShape &sh);
// ---- wide route (pgf_band_wide.hip) ---------------------------------------------
// the same on the wide route (sh.B > 8): per instance the reduction, or with the split on and
// ctl[0] == 0 the solve phase against its kept factors; lean: the host knows that no instance reduces
// guard == false (a refinement round with the split off): no copy to brhs0, no residual
// (bandb_launch_wide_residual is sp_launch_bw_residual's twin)
void bandb_launch_wide_solve(hipStream_t s, const BandInst *tab, int B, const BandShape &sh, bool lean,
                             bool guard = true);
void bandb_launch_wide_residual(hipStream_t s, const BandInst *tab, int B, const BandShape &sh);
// The band part of a bordered batch on the wide route (sh: the copy with N = Nb, nb = ceil(Nb / B)),
// each phase fixed by the caller instead of read from ctl[0] alone.  For the instances with ctl[0]
// != 0: the factor-only KEEP reduction of B (flags, inertia, kept multipliers; brhs survives), and
// Y <- inv(B) Y as one panel solve of sh.bkp columns against those factors.  For every live
// instance: brhs[0, Nb) <- inv(B) brhs[0, Nb) against the kept factors, flags untouched, no residual.
void bandb_launch_wide_factor(hipStream_t s, const BandInst *tab, int B, const BandShape &sh);
void bandb_launch_wide_panel(hipStream_t s, const BandInst *tab, int B, const BandShape &sh);
void bandb_launch_wide_kept_solve(hipStream_t s, const BandInst *tab, int B, const BandShape &sh);
// ---- step update, controller and refinement (pgf_sparse.hip) -------------------
// (xn, yn), dx, dy and the partial sums; the new point replaces the old one, which stays in
// (xn, yn), unless the instance met a bad pivot -- or move == false (a Globalized step on the table
// that names the outer point): the current point stays, the line search's finish moves it
void bandb_launch_step_update(hipStream_t s, const BandInst *tab, int B, const BandShape &sh, bool move = true);
// The step finished per instance on the device, behind the step update (the device-resident
// controller; what band_batch_sync does on the host): diff_out[i] the step length; flags_out[3 i]
// bit 0 a zero or non-finite pivot, bit 2 the guard's measure above the instance's tolerance
// (guard[BG_STRIDE i] != 0: the guard is on, [+ 1]: refine_tol, [+ 2]: refine_fail), [3 i + 1]
// negative pivots, [3 i + 2] |I|; rejects[2 i], [2 i + 1]: steps that set bit 0 / bit 2, counted.
// rctl != nullptr (PGF_BATCH_CTL_REFINE): the refinement rounds have run, and bit 2 is band_refine's
// verdict -- the step missed refine_tol as it came out of the solve (rctl[4 i + 2]) and the measure
// is above refine_fail now.
#define BG_STRIDE 3
void bandb_launch_step_final(hipStream_t s, const BandInst *tab, int B, const BandShape &sh,
                             const double *guard, double *diff_out, int *flags_out, int *rejects,
                             const int *rctl = nullptr);
// Refinement inside the device-resident controller's loop (PGF_BATCH_CTL_REFINE): what band_refine
// does on an instance's handle, one round.  decide: tab is the batch's OWN table (whose ctl[3] and
// status block it reads); per instance it sets rctl[4 i + 3] = 1 (sits the round out) unless the
// instance refines in this round, by band_refine's rule, and counts in rcnt.  The other launches
// take the refinement table (ctl -> rctl): load is bsol <- brhs, brhs <- bres and the point the step
// started from back in (x, y); the route's solve with the guard off follows (the launchers above),
// then axpy brhs += bsol, the route's residual and bandb_launch_step_update.
void bandb_launch_refine_decide(hipStream_t s, const BandInst *tab, int B, const BandShape &sh,
                                const double *guard, int *rctl, double *rrel, int *rcnt, int round);
void bandb_launch_refine_load(hipStream_t s, const BandInst *rtab, int B, const BandShape &sh);
void bandb_launch_refine_axpy(hipStream_t s, const BandInst *rtab, int B, const BandShape &sh);
void bandb_launch_residual(hipStream_t s, const BandInst *rtab, int B, const BandShape &sh);
// c = J x - b and F[0:n] = H x + q + J' y for the termination measures
void bandb_launch_measures_eval(hipStream_t s, const BandInst *tab, int B, const BandShape &sh);
