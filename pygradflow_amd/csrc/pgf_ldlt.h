// The dense LDL^T factorisation: its storage (DenseLdlt), the head work a step hands to the first
// chain's launch (LdltHead, HeadUnit), the profile and the host interface of pgf_ldlt.hip and
// pgf_factor2.hip, single handle and batch.  gfx950 (MI355X / CDNA4) only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <utility>
#include <vector>

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
  // false: the triangular solves of this factor always take the per-block kernels, never the
  // chained single-launch ones -- for an owner that has no host synchronisation of its own behind a
  // solve at which ldlt_chain_check could run (the large border's S, pgf_border_large.hip)
  bool chain_solves = true;
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

// ---- pgf_ldlt.hip: storage, status words, triangular solves ----------------
hipError_t ldlt_alloc(DenseLdlt &f, int Nmax, hipStream_t stream);
void ldlt_free(DenseLdlt &f);
void ldlt_chain_discard(DenseLdlt &f, int word);
// wait and read flags: returns 0 ok / 1 singular / 2 the diagonal chain's helper workgroups
// failed their checks (they are switched off, factorise again); sets f.n_neg.  (A chained solve that failed
// its own checks is reported by ldlt_chain_check after any host synchronisation.)
// (awaited: the caller has already seen everything enqueued on f.stream complete -- no runtime call)
int ldlt_finish(DenseLdlt &f, hipError_t *err, bool awaited = false);
// sol <- K^{-1} rhs on device vectors of length N (rhs preserved if rhs != sol)
hipError_t ldlt_solve_async(DenseLdlt &f, const double *rhs, double *sol);
// backward half only: sol <- L^{-T} w, w already equals D^{-1} L^{-1} rhs (row N trick)
hipError_t ldlt_backsolve_async(DenseLdlt &f, const double *w, double *sol);
// after a host sync: nonzero if a chained solve reported a timeout / placement problem
int ldlt_chain_check(DenseLdlt &f);
void ldlt_chain_set_enabled(bool on);  // test hook: undo the switch-off of a failed check
// shared launch helper
hipEvent_t prof_event(PgfProfile *p);

// ---- pgf_factor2.hip: the look-ahead schedule ------------------------------
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
void ldlt_chain_helpers_off();
void ldlt_inject_helper_failure(hipStream_t s, int *flags);  // test hook: flags[2] |= 1
bool ldlt_chain_helpers_enabled();     // helpers requested (PGF_CHAIN_HELP) and not switched off
void ldlt_chain_helpers_set(bool on);  // test hook: undo / force the switch-off
void ldlt_chain_timing_dump();  // PGF_CHAIN_TIMING diagnostic

// ---- batch (BInst: pgf_batch.h) --------------------------------------------
struct BInst;
// batched wrappers of the look-ahead schedule's chain and T(k) kernels (pgf_factor2.hip)
// helpers: 3 B workgroups of 1024 threads must be resident together (small batches only)
void ldlt_batch_launch_chain(hipStream_t s, const BInst *tab, int B, int m, int c0, bool helpers);
void ldlt_batch_launch_update_diag(hipStream_t s, const BInst *tab, int B, int m, int wbuf, int c1);
void ldlt_batch_launch_chain_update(hipStream_t s, const BInst *tab, int B, int Nmax, int m, int wbuf,
                                    int c1, bool helpers, int vdepth = 0);
void ldlt_batch_launch_virtual_diag(hipStream_t s, const BInst *tab, int B, int vdepth);
void ldlt_batch_launch_trsm(hipStream_t s, const BInst *tab, int B, int per, int m, int wbuf, int c0);
// pgf_ldlt.hip
void ldlt_batch_factor_async(hipStream_t s, const BInst *tab, int B, int Nmax, int m, PgfProfile *p,
                             int vdepth = 0);
void ldlt_batch_solve_async(hipStream_t s, const BInst *tab, int B, int Nmax, int m,
                            bool any_unfactored_solve, bool cond_prep = false);

// micro-benchmark of the trailing update (pgf_ldlt.hip)
hipError_t ldlt_bench_update(int N, int KB, int variant, int reps, double *ms_out,
                             double *flops_out);
