// Internal declarations shared by the HIP translation units of libpgf_hip.so.
// gfx950 (MI355X / CDNA4) only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstdlib>
#include <string>
#include <vector>

#include "pgf_sparse.h"

// The PGF_* environment switches (host).  Each call site keeps its value in a `static const', so a
// variable is read once per process, the first time its code path runs.
inline bool env_on(const char *name) {  // on unless set to 0
  const char *e = getenv(name);
  return !(e && atoi(e) == 0);
}
inline int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return e ? atoi(e) : dflt;
}
inline double env_double(const char *name, double dflt) {
  const char *e = getenv(name);
  return e ? atof(e) : dflt;
}

#define PGF_NB 64  // diagonal-block / triangular-solve block size (one wavefront of rows)

struct PgfProfile {
  bool enabled = false;
  // 1: the factorisation's kernels as separate launches, one span each (per-kernel figures);
  // 2: the PRODUCTION launches (diagonal chain beside the trailing update, T(k) with the next
  //    diagonal block's update), one span per launch
  int mode = 1;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> fused_spans, trsmud_spans;
  std::vector<double> fused_flops, fused_bytes;
  double acc_fused_ms = 0, acc_fused_flops = 0, acc_fused_bytes = 0, acc_trsmud_ms = 0;
  int64_t acc_fused_launches = 0;
  std::vector<hipEvent_t> pool;  // recycled event pairs
  std::vector<std::pair<hipEvent_t, hipEvent_t>> update_spans;
  std::vector<double> update_flops;
  std::vector<double> update_bytes;  // algorithmic bytes: C tile read + write, both panels once
  std::vector<std::pair<hipEvent_t, hipEvent_t>> factor_spans;
  // look-ahead schedule, instrumented (unfused) pass: the diagonal chain, the TRSM below it
  // and the diagonal-block update, one span per launch
  std::vector<std::pair<hipEvent_t, hipEvent_t>> chain_spans, trsm_spans, udiag_spans;
  double acc_update_ms = 0, acc_update_flops = 0, acc_update_bytes = 0, acc_factor_ms = 0;
  double acc_chain_ms = 0, acc_trsm_ms = 0, acc_udiag_ms = 0;
  int64_t acc_update_launches = 0, acc_chain_launches = 0;
};

// Dense symmetric factor  K = L D L^T  (unit lower L, diagonal D), lower triangle,
// row-major in HBM with row stride ldk.  Row N (when nrows == N + 1) carries a
// right-hand side through the elimination (forward substitution for free).
// update launches of one factorisation that can have their own persistent-tile counter (behind
// flags[0..3]; reused modulo this number: a launch is long finished 256 launches later)
#define LDLT_UPD_COUNTERS 256
// outer block width: the diagonal blocks of the chain, the K-depth of the bulk trailing update
#define LDLT_OB 256

struct DenseLdlt {
  int Nmax = 0;
  int64_t ldk = 0;
  double *K = nullptr;      // (Nmax + 1) x ldk
  double *W = nullptr;      // (Nmax + 1) x LDLT_OB workspace: W = L * D of the outer block
  double *dvec = nullptr;   // D
  double *dinv = nullptr;   // 1 / D
  double *zwork = nullptr;  // solve work vector (Nmax)
  double *Linv = nullptr;   // inverse of every 64 x 64 diagonal block of L, [block][row][64]
  double *LinvT = nullptr;  // the transposes
  int *flags = nullptr;     // [0] zero-pivot flag, [1] negative pivots, [2] chain helpers failed
  // chained solves: [2S] XCC slot, [2S+1] bad (S = chain_stride = 64-row blocks of capacity);
  // xpub: two halves of S * 64 published solution entries (sentinel = all bits set)
  int *chain = nullptr;
  double *xpub = nullptr;
  int chain_stride = 0;
  int *hctl = nullptr;      // stamps between the diagonal chain and its helper workgroups
  int *h_flags = nullptr;   // pinned host mirror ([3]: status word of the chained solves)
  hipStream_t stream = nullptr;
  size_t wstride = 0;       // doubles per W buffer (two buffers)
  int N = 0;
  bool factored = false;
  int n_neg = 0;
  PgfProfile *prof = nullptr;
  // A pre-eliminated diagonal block (the condensed KKT system, pgf_api_factor.hip): when vdepth > 0 the
  // matrix to factorise is K - V diag(vd) V^T, V = (N + 1) x vdepth row-major (row N rides along
  // like row N of K); the look-ahead schedule applies it as `virtual' column blocks that are
  // already factorised, lazily, like any other pending block.  vneg = the negative pivots of the
  // block eliminated beforehand; ldlt_finish adds them whatever vdepth is: a caller that has put
  // the block's Schur term into K itself (the resident Gram matrix, pgf_api_factor.hip) factorises with
  // vdepth = 0 and still owes them to the inertia.  Whoever sets vdepth sets vneg with it.
  double *V = nullptr;
  int64_t ldv = 0;
  double *vd = nullptr;
  int vdepth = 0;  // multiple of 32 (zero-padded columns)
  int vneg = 0;
  size_t vcap = 0, vdcap = 0;  // allocated doubles
  int inject_chain_failure = 0;  // test hook: the next chained solve reports a failure
  int inject_helper_failure = 0;  // test hook: the next factorisation reports failed helpers
  // Status words of a dense Newton step (pgf_api_step.hip): flags_zeroed -- the caller's assembly
  // launch has already cleared flags [0, 4 + LDLT_UPD_COUNTERS), so the next factorisation skips
  // its memset (consumed by it); defer_status -- the factorisation's flags and the chained solve's
  // status word are NOT copied to h_flags here: status_words records what is pending (bit 0: flags
  // [0, 4), bit 1: the chained solve's word), and the caller's step-update launch gathers them
  // into its status block, read with one copy.
  bool flags_zeroed = false;
  bool defer_status = false;
  int status_words = 0;
};

// Head work of a dense Newton step (pgf_api_factor.hip, factor_async): what the step writes in front of
// a factorisation whose first diagonal chain reads nothing but K[0:256, 0:256].  Given to
// ldlt_factor_async, the rows below 256 of the assembly and the panel V = J_I^T are written by
// the idle workgroups of the first chain's launch (k_chain_head, pgf_factor2.hip) instead of by
// launches of their own in front of it.  The operands are those of launch_assemble_kkt,
// launch_cond_panel and launch_cond_rhs.
struct LdltHead {
  const double *H = nullptr, *J = nullptr;
  int64_t ldh = 0, ldj = 0;
  const int *idxI = nullptr;
  int nI = 0, m = 0;  // m: constraint rows assembled into K (0 in the condensed order)
  double lamb = 0, delta = 0;
  const double *G = nullptr;  // the resident Gram matrix (condensed order) or null
  int64_t ldg = 0;
  const double *row_src = nullptr;  // natural order: copied to row_dst[0, row_n) (the rhs row)
  double *row_dst = nullptr;
  int row_n = 0;
  double *V = nullptr;  // the panel (condensed order) or null: pm constraint columns padded to mp
  int64_t ldv = 0;
  int mp = 0, pm = 0;
  double *vd = nullptr;
  const double *rhs_y = nullptr;
  // row nI of K <- crhs[0:nI] + V crhs[nI:] / delta behind the first chain's launch
  // (launch_cond_rhs reads V); null: none
  const double *crhs = nullptr;
  double *crhs_out = nullptr;
};
#define HEAD_ASM_ROWS 8  // rows of an assembly unit (ASM_ROWS of pgf_head_dev.h), 256 columns
// One unit of the head workers' list.  kind 0: assembly rows [8 b, 8 b + 8) x columns
// [256 a, 256 a + 256) of K (what lies on or below the diagonal and inside N); kind 1: the
// 32 x 32 tile of V at rows [32 a, 32 a + 32), columns [32 b, 32 b + 32), and for a == 0 the same
// columns of the tail row nI and of vd; kind -1: past the end.
struct HeadUnit {
  int kind, a, b;
};
// assembly units: the row groups of rows >= 256, one unit per column block up to the diagonal's
__host__ __device__ inline int head_asm_units(int N) {
  const int nrg = (N + HEAD_ASM_ROWS - 1) / HEAD_ASM_ROWS, per = LDLT_OB / HEAD_ASM_ROWS;
  int cnt = 0;
  for (int B = 1; B * per < nrg; ++B) cnt += ((nrg < (B + 1) * per ? nrg : (B + 1) * per) - B * per) * (B + 1);
  return cnt;
}
__host__ __device__ inline int head_panel_units(int nI, int mp) {
  return (nI > 0 && mp > 0) ? ((nI + 31) / 32) * (mp / 32) : 0;
}
// THE unit -> (rows, columns) mapping, on the device (k_chain_head) and on the host
// (pgf_debug_head_plan): assembly units first, band of 256 rows by band, a row group's column
// blocks side by side; then the panel's tiles, a row of tiles side by side.
__host__ __device__ inline HeadUnit head_unit(int u, int N, int nI, int mp) {
  const int nrg = (N + HEAD_ASM_ROWS - 1) / HEAD_ASM_ROWS, per = LDLT_OB / HEAD_ASM_ROWS;
  if (u < 0) return HeadUnit{-1, 0, 0};
  for (int B = 1; B * per < nrg; ++B) {
    const int cnt = ((nrg < (B + 1) * per ? nrg : (B + 1) * per) - B * per) * (B + 1);
    if (u < cnt) return HeadUnit{0, u % (B + 1), B * per + u / (B + 1)};
    u -= cnt;
  }
  if (u < head_panel_units(nI, mp)) return HeadUnit{1, u / (mp / 32), u % (mp / 32)};
  return HeadUnit{-1, 0, 0};
}

hipError_t ldlt_alloc(DenseLdlt &f, int Nmax, hipStream_t stream);
void ldlt_free(DenseLdlt &f);
void ldlt_chain_discard(DenseLdlt &f, int word);
// true: a factorisation of size N enqueued now takes an LdltHead (PGF_HEAD_FUSED, the production
// launches, more than one outer block, no pre-eliminated panel: the virtual blocks' first launch
// already carries update jobs that read the assembled K and V)
bool ldlt_head_wanted(const DenseLdlt &f, int N);
// enqueue the factorisation of the leading N x N lower triangle (+ rows up to nrows): the
// look-ahead schedule of pgf_factor2.hip.  head (only where ldlt_head_wanted): K's assembly, the
// panel and the zeroing of the flags are enqueued here, around the first chain -- the caller has
// issued none of them.
hipError_t ldlt_factor_async(DenseLdlt &f, int N, int nrows, const LdltHead *head = nullptr);
// G <- V V^T (lower triangle of n x n, row stride ldg) with the trailing update's own tiles: G is
// zeroed, then C -= V diag(vd) V^T runs over the whole triangle as ONE virtual-only job (vd = -1
// in all `depth' entries, depth a multiple of 32; V has row stride ldv).  ctr: a counter word of the
// caller's for the persistent tile loop -- never one of a factorisation's (f.flags), which may be
// in flight on the same stream's neighbours and is zeroed on another schedule.
hipError_t ldlt_gram_async(hipStream_t s, double *G, int64_t ldg, int n, const double *V, int64_t ldv,
                           const double *vd, int depth, int *ctr);
// wait and read flags: returns 0 ok / 1 singular / 2 the diagonal chain's helper workgroups
// failed their checks (they are switched off, factorise again); sets f.n_neg.  (A chained solve that failed
// its own checks is reported by ldlt_chain_check after any host synchronisation.)
int ldlt_finish(DenseLdlt &f, hipError_t *err);
// sol <- K^{-1} rhs on device vectors of length N (rhs preserved if rhs != sol)
hipError_t ldlt_solve_async(DenseLdlt &f, const double *rhs, double *sol);
// backward half only: sol <- L^{-T} w, w already equals D^{-1} L^{-1} rhs (row N trick)
hipError_t ldlt_backsolve_async(DenseLdlt &f, const double *w, double *sol);
// after a host sync: nonzero if a chained solve reported a timeout / placement problem
int ldlt_chain_check(DenseLdlt &f);
void ldlt_chain_set_enabled(bool on);  // test hook: undo the switch-off of a failed check
void ldlt_chain_helpers_off();
void ldlt_inject_helper_failure(hipStream_t s, int *flags);  // test hook: flags[2] |= 1
bool ldlt_chain_helpers_enabled();     // helpers requested (PGF_CHAIN_HELP) and not switched off
void ldlt_chain_helpers_set(bool on);  // test hook: undo / force the switch-off
void ldlt_chain_timing_dump();  // PGF_CHAIN_TIMING diagnostic
// shared launch helper (pgf_ldlt.hip)
hipEvent_t prof_event(PgfProfile *p);

// ---- dense LU with partial pivoting (pgf_lu.hip): P A = L U, row-major, in place ----------
struct DenseLu {
  int N = 0;
  int64_t ld = 0;
  double *A = nullptr;     // N x ld: unit-lower L below the diagonal, U on and above it
  int *piv = nullptr;      // row interchanged with row i at step i (LAPACK convention)
  int *perm = nullptr;     // the interchanges as one permutation: (P b)[i] = b[perm[i]]
  double *work = nullptr;  // N
  double *PT = nullptr;    // the current panel, column-major (32 x ldp): pivot search and rank-1
  int64_t ldp = 0;         // updates run along rows, coalesced
  int *flags = nullptr;    // [0] zero / non-finite pivot
  hipStream_t stream = nullptr;
  bool factored = false;
  int reg_panels = 0, streamed_panels = 0;  // of the last factorisation: k_lu_panel_reg / k_lu_panel
};
hipError_t lu_alloc(DenseLu &f, int N, hipStream_t stream);
void lu_free(DenseLu &f);
int lu_factor(DenseLu &f, hipError_t *err);  // 0 ok / 1 singular / -1 HIP error
hipError_t lu_solve_async(DenseLu &f, const double *rhs, double *sol, int trans);

// ---- batched mode ----------------------------------------------------------
// One entry per instance of a batch (all instances share n, m): the device addresses of an
// ordinary solver handle.  Batched kernels pick their instance with blockIdx.z and read the
// instance's own reduced size N = counts[0] + m on the device, so a whole batched Newton
// step is enqueued without a host round trip.  ctl: [0] factor this step, [1] factor
// valid, [2] mask valid, [3] frozen (the instance sits this Newton step out).
// ps: the instance's own outer-step scalars [dt, lambda, rho, fact, delta] -- every instance
// has its own step-size controller.
struct BInst {
  const double *H, *J;
  int64_t ldh, ldj;
  const double *lb, *ub, *q, *b;
  double *slb, *sub, *xhat, *yhat, *x, *y, *xn, *yn, *g, *c, *F, *b0full, *rhs, *sol, *dx, *dy;
  double *w, *tmpn, *partial, *red;
  uint8_t *mask, *mask_new;
  int *idxI, *idxA, *pos, *counts, *ctl;
  const double *ps;
  double *K;
  int64_t ldk;
  double *W;
  int64_t wstride;
  double *dvec, *dinv, *zwork, *Linv, *LinvT;
  int *flags;
  int *hctl;  // stamps between the instance's chain and its helper workgroups (small batches)
  // chained triangular solves: both publication halves (capblk * 64 entries each) and the
  // control words [0] XCC slot, [1] status, [2] solve counter of the instance's handle
  double *xpub;
  int *cctl;
  int capblk;
  // condensed order (pgf_api_batch.hip, pgf_batch_s::cond_wanted): the instance's panel V = J_I^T
  // ((n + 1) x ldv, row nI = the constraint part of the right-hand side) and its scaling -1 / delta
  double *V;
  int64_t ldv;
  double *vd;
};

struct BatchScalars {
  int n, m;
};
#define BPS_DT 0
#define BPS_LAMB 1
#define BPS_RHO 2
#define BPS_FACT 3
#define BPS_DELTA 4
// ||H||_inf, ||J||_1, ||J||_inf of the instance (residual_norms): the normwise measure of
// kb_sample_residual bounds ||K||_inf with them and the current lambda, delta
#define BPS_NORM_H 5
#define BPS_NORM_J1 6
#define BPS_NORM_JINF 7
#define BPS_STRIDE 8

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
  double *bsol;  // the solution a refinement round keeps (PGF_BATCH_CTL_REFINE; SparseDev::bsol)
  double *bD, *bL, *bU, *bDinv, *bF;  // two block sets, bstride blocks apart (SparseDev; wide: one)
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
  // partial sums of the step update, [3 nred, 3 nred + 4) pivot flags (as SparseDev::bred)
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
// its pivots; stat: where the residual pairs go (SparseDev::bred, or a batch's status slice).  The
// vectors of the step, ctl, ps and the counters stay null: band_batch_create adds them.
inline BandInst band_inst_of(const SparseDev &sp, int *flags, double *stat) {
  BandInst u{};
  u.Hval = sp.Hval;
  u.Jval = sp.Jval;
  u.band = sp.band;
  u.brhs = sp.brhs;  // (SparseDev::bX is brhs: the back-substitution writes the solution there)
  u.brhs0 = sp.brhs0;
  u.bres = sp.bres;
  u.bsol = sp.bsol;
  u.bD = sp.bD;
  u.bL = sp.bL;
  u.bU = sp.bU;
  u.bDinv = sp.bDinv;
  u.bF = sp.bF;
  u.bMr = sp.bMr;
  u.bMl = sp.bMl;
  u.bneg = sp.bneg;
  u.flags = flags;
  u.bC = sp.bC;
  u.bDd = sp.bDd;
  u.bY = sp.bY;
  u.bS = sp.bS;
  u.bpart = sp.bpart;
  u.bpartv = sp.bpartv;
  u.brb = sp.brb;
  u.bz = sp.bz;
  u.bsflags = sp.bsflags;
  u.stat = stat;
  return u;
}
// The SparseDev part of a BandShape for a reduction over N rows (n + m, or the Nb band rows under a
// border); n and m are the caller's.  split: the factor / solve split is in force only where the
// multipliers are allocated.  sp.B is the block size of a pattern that is set (8, 16, 32 or 64), never
// the 0 of a fresh SparseDev.
inline BandShape band_shape_of(const SparseDev &sp, int N) {
  BandShape sh{};
  sh.N = N;
  sh.B = sp.B;
  sh.split = (sp.B > 8 && sp.split && sp.bMr) ? 1 : 0;
  sh.nb = (N + sp.B - 1) / sp.B;
  sh.bw = sp.bw;
  sh.ldb = sp.ldb;
  sh.nnzH = sp.nnzH;
  sh.nnzJ = sp.nnzJ;
  sh.nred = sp.nred;
  sh.bk = sp.bk;
  sh.bkp = sp.bkp;
  sh.Nb = sp.bk ? sp.Nb : N;
  sh.bnchunk = sp.bnchunk;
  sh.bstride = sp.bstride;
  sh.pos = sp.pos;
  sh.Hptr = sp.Hptr;
  sh.Hrow = sp.Hrow;
  sh.Hcol = sp.Hcol;
  sh.Hslot = sp.Hslot;
  sh.Jptr = sp.Jptr;
  sh.Jcol = sp.Jcol;
  sh.Jslot = sp.Jslot;
  sh.JTptr = sp.JTptr;
  sh.JTrow = sp.JTrow;
  sh.JTmap = sp.JTmap;
  return sh;
}
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
// bordered routes (pgf_border.hip; both wrappers branch on sh.B > 8).  Factor phase of the
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
// (xn, yn), dx, dy and the partial sums; the new point replaces the old one, which stays in
// (xn, yn), unless the instance met a bad pivot
void bandb_launch_step_update(hipStream_t s, const BandInst *tab, int B, const BandShape &sh);
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

// device-resident step controller: per-instance state (cs) and constants (cp)
#define DCS_LAMB 0      // lambda of the next outer iteration
#define DCS_INTEGRAL 1  // integral of the PI law (log scale)
#define DCS_FIRST 2     // step length of the first Newton step
#define DCS_ACCEPTED 3  // 1: the last outer step was accepted
#define DCS_DONE 4      // 1: decided after the first Newton step
#define DCS_NEXT 5      // lambda decided so far
#define DCS_USED 6      // lambda the current iteration ran with
#define DCS_STRIDE 8
#define DCP_RHO 0
#define DCP_NEWTON_TOL 1
#define DCP_LAMB_RED 2
#define DCP_LAMB_MIN 3
#define DCP_LAMB_INC 4
#define DCP_THETA_MAX 5
#define DCP_K_P 6
#define DCP_K_I 7
#define DCP_LOG_THETA_REF 8
#define DCP_COUNT 16
void batch_launch_dctl_begin(hipStream_t s, int B, const double *cs, const double *cp, double *ps,
                             uint8_t *accept);
void batch_launch_dctl_mid(hipStream_t s, const BInst *tab, int B, double *cs, const double *cp,
                           const double *diff, const int *flags, const double *norm);
void batch_launch_dctl_end(hipStream_t s, int B, double *cs, const double *cp, const double *diff,
                           const int *flags, double *log3);

// pgf_kernels.hip
// accept[i] != 0: (x^, y^) <- (x, y); == 0: (x, y) <- (x^, y^) (a rejected step goes back)
void batch_launch_advance(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc,
                          const uint8_t *accept);
void batch_launch_set_frozen(hipStream_t s, const BInst *tab, int B, const uint8_t *frozen);
void batch_launch_eval(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc, int nparts);
// mode 1: adopt mask_new where it differs (or no mask yet); 2: always adopt; 0: keep
void batch_launch_mask(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc, int mode,
                       double tau);
// cond_mp > 0: the condensed order -- only A = H[I,I] + lamb I is assembled (+ b_x in row nI), the
// constraint block goes into the instances' panels V (cond_mp columns, zero-padded)
void batch_launch_rhs_assemble(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc,
                               int cond_mp = 0);
// condensed order: zwork <- b_x + V b_y / delta before a forward solve (instances that reuse their
// factor), sol_y <- (V^T sol_x - b_y) / delta after the backward solve (all instances)
void batch_launch_residual(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc);
void batch_launch_cond_prep_fwd(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc);
void batch_launch_cond_y(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc);
// flags_out: [3 i] zero-pivot flag, [3 i + 1] negative pivots, [3 i + 2] |I| of instance i
void batch_launch_step_update(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc,
                              double *diff_out, int *flags_out);
void batch_launch_res_norm(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc,
                           double *norm_out);
void batch_launch_measures(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc,
                           int nparts, double active_tol, double *red4, double *out);
void batch_launch_measures_final(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc,
                                 double active_tol, double *red4, double *out);
// pgf_ldlt.hip
// batched wrappers of the look-ahead schedule's chain and T(k) kernels (pgf_factor2.hip)
// helpers: 3 B workgroups of 1024 threads must be resident together (small batches only)
void ldlt_batch_launch_chain(hipStream_t s, const BInst *tab, int B, int m, int c0, bool helpers);
void ldlt_batch_launch_update_diag(hipStream_t s, const BInst *tab, int B, int m, int wbuf, int c1);
void ldlt_batch_launch_chain_update(hipStream_t s, const BInst *tab, int B, int Nmax, int m, int wbuf,
                                    int c1, bool helpers, int vdepth = 0);
void ldlt_batch_launch_virtual_diag(hipStream_t s, const BInst *tab, int B, int vdepth);
void ldlt_batch_launch_trsm(hipStream_t s, const BInst *tab, int B, int per, int m, int wbuf, int c0);
void ldlt_batch_factor_async(hipStream_t s, const BInst *tab, int B, int Nmax, int m, PgfProfile *p,
                             int vdepth = 0);
bool ldlt_chain_enabled();  // chained solves requested (PGF_TRSV_CHAIN) and not switched off
void ldlt_batch_solve_async(hipStream_t s, const BInst *tab, int B, int Nmax, int m,
                            bool any_unfactored_solve, bool cond_prep = false);

// ---- elementwise / assembly launches (pgf_kernels.hip) --------------------
struct StepDev;  // opaque here

// micro-benchmark of the trailing update (pgf_ldlt.hip)
hipError_t ldlt_bench_update(int N, int KB, int variant, int reps, double *ms_out,
                             double *flops_out);
