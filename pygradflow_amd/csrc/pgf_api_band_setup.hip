// Configuration and lifetimes of the banded handle: the pgf_sparse_* setters (pattern, values, block
// size, factor / solve split, both borders), the pgf_debug_band_* / pgf_debug_border_* hooks, and the
// one release function of every group of SparseDev (pgf_sparse.h) that owns memory.  The solve
// driver is pgf_api_band.hip.
#include <algorithm>
#include <new>

#include "pgf_api_internal.h"
#include "pgf_env.h"

// PGF_BW_SPLIT=0: new handles start with the wide band's factor / solve split off
bool band_split_default() { static const bool on = env_on("PGF_BW_SPLIT"); return on; }

// ---------------------------------------------------------------- the groups' lifetimes
// Each release frees every pointer of its group, nulls it and resets the group's scalars.
static void band_release_pattern(SparseDev &sp) {
  auto &g = sp.pat;
  dev_free(g.pos, g.Hptr, g.Hrow, g.Hcol, g.Hslot, g.Jptr, g.Jcol, g.Jslot, g.JTptr, g.JTrow, g.JTmap,
           g.Hval, g.Jval, g.band, g.Hb0, g.Jb0);
  g = {};
  sp.active = false;
}
static void band_release_vectors(SparseDev &sp) {
  auto &g = sp.vec;
  dev_free(g.brhs, g.brhs0, g.bres, g.bsol, g.bred);
  pinned_free(g.h_bred);
  g = {};
}
static void band_release_panel(SparseDev &sp) {
  dev_free(sp.pan.bP, sp.pan.bredm);
  pinned_free(sp.pan.h_bredm);
}
// (split is the caller's setting, not the blocks': it stays; the panel is sized by the blocks)
static void band_release_blocks(SparseDev &sp) {
  auto &g = sp.blk;
  dev_free(g.bD, g.bL, g.bU, g.bDinv, g.bF, g.bneg, g.bMr, g.bMl);
  g.B = g.kept = 0;
  g.bstride = 0;
  band_release_panel(sp);
}
// (bC, bDd point into pat.band; the border's two counters start again with it)
static void band_release_border(SparseDev &sp) {
  auto &g = sp.bor;
  dev_free(g.bY, g.bS, g.bpart, g.bpartv, g.brb, g.bz, g.bsflags, g.bG);
  if (g.blf) {
    ldlt_free(*g.blf);
    delete g.blf;
  }
  g = {};
  sp.cnt.stat_bfactor = sp.cnt.stat_bsolve = 0;
}
void band_free(pgf_handle h) {
  band_release_border(h->sp);
  band_release_blocks(h->sp);
  band_release_vectors(h->sp);
  band_release_pattern(h->sp);
}

// One allocation of a list behind one hipError_t: a no-op once *e holds an error (as batch_alloc).
template <typename T>
static void band_alloc(hipError_t *e, T **p, size_t count) {
  if (*e == hipSuccess) *e = dalloc(p, count);
}

// Residual pairs of a band of N = Nb + k rows: one per 256 band rows and one per 256 border rows, and
// never fewer than the step update's partial sums over N rows need.  k == 0: ceil(N / 256).
static int band_nred(int N, int Nb, int k) { return std::max((N + 255) / 256, (Nb + 255) / 256 + (k + 255) / 256); }

// the status block (SparseDev::vec.bred) and its pinned mirror for nred pairs, in place of what is there
static void band_alloc_status(hipError_t *e, SparseDev &sp, int nred) {
  dev_free(sp.vec.bred);
  pinned_free(sp.vec.h_bred);
  sp.vec.nred = nred;
  band_alloc(e, &sp.vec.bred, band_stat_stride(nred));
  if (*e == hipSuccess) *e = hipHostMalloc((void **)&sp.vec.h_bred, band_stat_stride(nred) * sizeof(double));
}

// bw <= 8: 8 x 8 cyclic reduction; 9 .. 64: the smallest of 16, 32, 64 that holds the band
static int auto_block_size(int bw) { return bw <= 8 ? 8 : bw <= 16 ? 16 : bw <= 32 ? 32 : 64; }

// work arrays of the cyclic reduction for block size B, in place of what is there.  B = 8 keeps two
// block sets (k_bcr_level2 reads one and writes the other); the wide kernels use one.
static int sp_alloc_blocks(pgf_handle h, int B) {
  auto &g = h->sp.blk;
  band_release_blocks(h->sp);
  g.B = B;
  const int N = h->n + h->m;
  const size_t nsets = (B == 8) ? 2 : 1, Bk = (size_t)B;
  const size_t nbk = ((size_t)N + Bk - 1) / Bk + 1;
  g.bstride = (int64_t)nbk;
  hipError_t e = hipSuccess;
  band_alloc(&e, &g.bD, nsets * nbk * Bk * Bk);
  band_alloc(&e, &g.bL, nsets * nbk * Bk * Bk);
  band_alloc(&e, &g.bU, nsets * nbk * Bk * Bk);
  band_alloc(&e, &g.bDinv, nbk * Bk * Bk);
  band_alloc(&e, &g.bF, nsets * nbk * Bk);
  band_alloc(&e, &g.bneg, nbk);
  if (B > 8 && g.split) {  // the kept forward multipliers of the wide reduction
    band_alloc(&e, &g.bMr, nbk * Bk * Bk);
    band_alloc(&e, &g.bMl, nbk * Bk * Bk);
  }
  return e == hipSuccess ? PGF_OK : hip_fail(h, e, "band work blocks");
}

// the panel of band_linear_solve_multi and, behind it, the right-hand sides as they came (natural
// order); per column the residual pairs + flags (device and pinned mirror)
int band_panel_reserve(pgf_handle h) {
  auto &g = h->sp.pan;
  if (g.bP) return PGF_OK;
  const size_t prows = (size_t)h->sp.blk.bstride * h->sp.blk.B, pairs = band_stat_stride(h->sp.vec.nred);
  HIPCHK(h, dalloc(&g.bP, prows * 64 + (size_t)64 * (h->n + h->m)));
  HIPCHK(h, dalloc(&g.bredm, 64 * pairs));
  HIPCHK(h, hipHostMalloc((void **)&g.h_bredm, 64 * pairs * sizeof(double)));
  return PGF_OK;
}

// no border: the band and the status block as pgf_sparse_set_pattern leaves them
static hipError_t band_plain_store(pgf_handle h) {
  SparseDev &sp = h->sp;
  const int N = h->n + h->m;
  band_release_border(sp);
  dev_free(sp.pat.band);
  hipError_t e = hipSuccess;
  band_alloc(&e, &sp.pat.band, (size_t)(N + 1) * sp.pat.ldb);
  band_alloc_status(&e, sp, band_nred(N, N, 0));
  return e;
}

// One border declaration behind both entry points, which have checked k (0: the border goes): the
// store is band + C + D in one array, which the plan's slots index as a whole.  Everything is
// computed and refused before anything of the handle is released.  The allocations are a list behind
// one error, whose exit leaves no border and the plain band of the pattern.
static int band_declare_border(pgf_handle h, int k, int kp, bool large) {
  SparseDev &sp = h->sp;
  auto &g = sp.bor;
  const int N = h->n + h->m, Nb = N - k;
  const size_t band_doubles = (size_t)(Nb + 1) * sp.pat.ldb;
  if (k > 0 && band_doubles + (size_t)Nb * kp + (size_t)kp * kp > (size_t)INT32_MAX)
    return fail(h, PGF_INVALID, "band and border store exceed 2^31 entries");
  (void)hipSetDevice(h->device);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  const bool had = g.bk > 0;
  band_release_border(sp);
  invalidate_factor(h);
  if (k == 0) {
    if (had) HIPCHK(h, band_plain_store(h));
    return PGF_OK;
  }
  dev_free(sp.pat.band);
  hipError_t e = hipSuccess;
  band_alloc(&e, &sp.pat.band, band_doubles + (size_t)Nb * kp + (size_t)kp * kp);
  band_alloc_status(&e, sp, band_nred(N, Nb, k));
  const int nchunk = (Nb + SP_BORDER_CHUNK - 1) / SP_BORDER_CHUNK;
  const size_t ntiles = (size_t)(kp / 64) * (kp / 64 + 1) / 2;
  if (large) sp_borderL_gram_plan(Nb, kp, &g.bgrows, &g.bgchunks);
  band_alloc(&e, &g.bY, ((size_t)Nb + 64) * kp);
  // large: the right-hand side of the solve with S, and the Gram kernel's partial sums per tile
  band_alloc(&e, &g.bS, large ? (size_t)kp : (size_t)kp * kp);
  band_alloc(&e, &g.bpart, large ? (size_t)g.bgchunks * ntiles * 4096 : (size_t)nchunk * kp * kp);
  band_alloc(&e, &g.bpartv, (size_t)nchunk * 3 * kp);
  band_alloc(&e, &g.brb, (size_t)kp);
  band_alloc(&e, &g.bz, (size_t)kp);
  band_alloc(&e, &g.bsflags, 4);
  if (large) {
    band_alloc(&e, &g.bG, (size_t)kp * kp);
    if (e == hipSuccess && !(g.blf = new (std::nothrow) DenseLdlt())) e = hipErrorOutOfMemory;
    if (e == hipSuccess) e = ldlt_alloc(*g.blf, kp, h->stream);
    if (e == hipSuccess) {
      g.blf->chain_solves = false;  // (no host synchronisation of its own behind a solve phase)
      e = hipMemsetAsync(g.blf->K, 0, ((size_t)kp + 1 + PGF_NB) * g.blf->ldk * sizeof(double), h->stream);
    }
    if (e == hipSuccess) e = hipMemsetAsync(g.bsflags, 0, 4 * sizeof(int), h->stream);
  }
  if (e == hipSuccess) e = hipMemsetAsync(g.brb, 0, (size_t)kp * sizeof(double), h->stream);  // padding stays zero
  if (e == hipSuccess) e = hipMemsetAsync(sp.vec.bred, 0, band_stat_stride(sp.vec.nred) * sizeof(double), h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    (void)band_plain_store(h);
    return hip_fail(h, e, "border allocation");
  }
  g.bk = k;
  g.bkp = kp;
  g.Nb = Nb;
  g.bnchunk = nchunk;
  g.bC = sp.pat.band + band_doubles;
  g.bDd = g.bC + (size_t)Nb * kp;
  return PGF_OK;
}

extern "C" {

int pgf_sparse_pattern_hash(int n, int m, int bw, const int *pos, int nnzH, const int *Hptr,
                            const int *Hrow, const int *Hcol, const int *Hslot, int nnzJ,
                            const int *Jptr, const int *Jcol, const int *Jslot, const int *JTptr,
                            const int *JTrow, const int *JTmap, uint64_t *hash_out) {
  if (!hash_out || n < 0 || m < 0 || nnzH < 0 || nnzJ < 0 || !pos || !Hptr || !Jptr || !JTptr ||
      (nnzH && (!Hrow || !Hcol || !Hslot)) || (nnzJ && (!Jcol || !Jslot || !JTrow || !JTmap)))
    return PGF_INVALID;
  uint64_t hsh = 1469598103934665603ull;  // FNV-1a, 64 bit
  auto eat = [&](const int *a, size_t count) {
    const unsigned char *p = reinterpret_cast<const unsigned char *>(a);
    for (size_t k = 0; k < count * sizeof(int); ++k) hsh = (hsh ^ p[k]) * 1099511628211ull;
  };
  const int head[5] = {n, m, bw, nnzH, nnzJ};
  eat(head, 5);
  eat(pos, (size_t)n + m);
  eat(Hptr, (size_t)n + 1);
  eat(Hrow, (size_t)nnzH);
  eat(Hcol, (size_t)nnzH);
  eat(Hslot, (size_t)nnzH);
  eat(Jptr, (size_t)m + 1);
  eat(Jcol, (size_t)nnzJ);
  eat(Jslot, (size_t)nnzJ);
  eat(JTptr, (size_t)n + 1);
  eat(JTrow, (size_t)nnzJ);
  eat(JTmap, (size_t)nnzJ);
  *hash_out = hsh;
  return PGF_OK;
}

int pgf_sparse_set_pattern(pgf_handle h, int bw, const int *pos, int nnzH, const int *Hptr,
                           const int *Hrow, const int *Hcol, const int *Hslot, int nnzJ,
                           const int *Jptr, const int *Jcol, const int *Jslot, const int *JTptr,
                           const int *JTrow, const int *JTmap) {
  if (!h) return PGF_INVALID;
  if (!h->sparse) return fail(h, PGF_NOT_READY, "handle was not created with PGF_CREATE_SPARSE");
  if (bw < 0 || bw > 64) return fail(h, PGF_INVALID, "bandwidth must be 0..64 in this version");
  if (nnzH < 0 || nnzJ < 0 || !pos || !Hptr || !Jptr || !JTptr)
    return fail(h, PGF_INVALID, "null pattern");
  const int n = h->n, m = h->m, N = n + m;
  // (what a banded batch compares: its instances share one pattern)
  uint64_t hash;
  if (pgf_sparse_pattern_hash(n, m, bw, pos, nnzH, Hptr, Hrow, Hcol, Hslot, nnzJ, Jptr, Jcol, Jslot, JTptr,
                              JTrow, JTmap, &hash) != PGF_OK)
    return fail(h, PGF_INVALID, "null pattern");
  (void)hipSetDevice(h->device);
  SparseDev &sp = h->sp;
  band_free(h);  // (a border is declared after the pattern: pgf_sparse_set_border)
  invalidate_factor(h);
  auto &g = sp.pat;
  g.bw = bw;
  g.ldb = ((bw + 1) + 1) / 2 * 2;
  g.nnzH = nnzH;
  g.nnzJ = nnzJ;
  g.hash = hash;
  int rc;
  if ((rc = up_new(h, &g.pos, pos, (size_t)N))) return rc;
  if ((rc = up_new(h, &g.Hptr, Hptr, (size_t)n + 1))) return rc;
  if ((rc = up_new(h, &g.Hrow, Hrow, (size_t)nnzH))) return rc;
  if ((rc = up_new(h, &g.Hcol, Hcol, (size_t)nnzH))) return rc;
  if ((rc = up_new(h, &g.Hslot, Hslot, (size_t)nnzH))) return rc;
  if ((rc = up_new(h, &g.Jptr, Jptr, (size_t)m + 1))) return rc;
  if ((rc = up_new(h, &g.Jcol, Jcol, (size_t)nnzJ))) return rc;
  if ((rc = up_new(h, &g.Jslot, Jslot, (size_t)nnzJ))) return rc;
  if ((rc = up_new(h, &g.JTptr, JTptr, (size_t)n + 1))) return rc;
  if ((rc = up_new(h, &g.JTrow, JTrow, (size_t)nnzJ))) return rc;
  if ((rc = up_new(h, &g.JTmap, JTmap, (size_t)nnzJ))) return rc;
  hipError_t e = hipSuccess;
  band_alloc(&e, &g.Hval, (size_t)nnzH);
  band_alloc(&e, &g.Jval, (size_t)nnzJ);
  band_alloc(&e, &g.band, (size_t)(N + 1) * g.ldb);
  band_alloc(&e, &sp.vec.brhs, (size_t)N + 64);  // whole B-row blocks: the cyclic reduction's X
  band_alloc(&e, &sp.vec.brhs0, (size_t)N + 1);
  band_alloc(&e, &sp.vec.bres, (size_t)N + 1);
  band_alloc(&e, &sp.vec.bsol, (size_t)N + 1);
  band_alloc_status(&e, sp, band_nred(N, N, 0));
  band_alloc(&e, &g.Hb0, (size_t)n + 1);
  band_alloc(&e, &g.Jb0, (size_t)m + 1);
  if (e != hipSuccess) return hip_fail(h, e, "band pattern arrays");
  if ((rc = sp_alloc_blocks(h, auto_block_size(bw)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  sp.active = true;
  return PGF_OK;
}

int pgf_sparse_set_border(pgf_handle h, int k) {
  if (!h) return PGF_INVALID;
  if (!h->sparse) return fail(h, PGF_INVALID, "pgf_sparse_set_border: banded handles only");
  if (k < 0 || k > 64) return fail(h, PGF_INVALID, "border size must be 0..64");
  if (!h->sp.active) return fail(h, PGF_NOT_READY, "pgf_sparse_set_pattern first");
  if (k > 0 && k >= h->n + h->m) return fail(h, PGF_INVALID, "the border must leave at least one band row");
  return band_declare_border(h, k, (k + 15) / 16 * 16, /*large=*/false);
}

int pgf_sparse_set_border_large(pgf_handle h, int k) {
  if (!h) return PGF_INVALID;
  if (!h->sparse) return fail(h, PGF_INVALID, "pgf_sparse_set_border_large: banded handles only");
  if (k < 65 || k > 1024) return fail(h, PGF_INVALID, "large border size must be 65..1024");
  if (!h->sp.active) return fail(h, PGF_NOT_READY, "pgf_sparse_set_pattern first");
  if (k >= h->n + h->m) return fail(h, PGF_INVALID, "the border must leave at least one band row");
  const auto &blk = h->sp.blk;
  if (blk.B <= 8) return fail(h, PGF_INVALID, "a large border needs a wide remainder (block size 16, 32 or 64)");
  if (!(blk.split && blk.bMr)) return fail(h, PGF_INVALID, "a large border needs the factor / solve split");
  return band_declare_border(h, k, (k + 63) / 64 * 64, /*large=*/true);
}

int pgf_debug_border_stats(pgf_handle h, int *k, int *border_factorisations, int *border_solves) {
  if (!h) return PGF_INVALID;
  if (k) *k = h->sp.bor.bk;
  if (border_factorisations) *border_factorisations = h->sp.cnt.stat_bfactor;
  if (border_solves) *border_solves = h->sp.cnt.stat_bsolve;
  return PGF_OK;
}

int pgf_debug_border_gram(pgf_handle h, double *Cout, double *Yout, double *Gout) {
  if (!h) return PGF_INVALID;
  const SparseDev &sp = h->sp;
  if (!h->sparse || !sp_border_large(sp)) return fail(h, PGF_INVALID, "pgf_debug_border_gram: no large border");
  if (!sp.bor.gram_ready) return fail(h, PGF_NOT_READY, "no factor phase has run on this border yet");
  (void)hipSetDevice(h->device);
  const size_t panel = (size_t)sp.bor.Nb * sp.bor.bkp * sizeof(double);
  int rc;
  if (Cout && (rc = down(h, Cout, sp.bor.bC, panel))) return rc;
  if (Yout && (rc = down(h, Yout, sp.bor.bY, panel))) return rc;
  if (Gout && (rc = down(h, Gout, sp.bor.bG, (size_t)sp.bor.bkp * sp.bor.bkp * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PGF_OK;
}

int pgf_debug_border_gram_plan(pgf_handle h, int *rows, int *chunks, int *tiles) {
  if (!h) return PGF_INVALID;
  const SparseDev &sp = h->sp;
  if (!h->sparse || !sp_border_large(sp)) return fail(h, PGF_INVALID, "pgf_debug_border_gram_plan: no large border");
  if (rows) *rows = sp.bor.bgrows;
  if (chunks) *chunks = sp.bor.bgchunks;
  if (tiles) *tiles = (sp.bor.bkp / 64) * (sp.bor.bkp / 64 + 1) / 2;
  return PGF_OK;
}

int pgf_debug_border_gram_time(pgf_handle h, int reps, double *ms_mfma, double *ms_fma) {
  if (!h || !ms_mfma || !ms_fma || reps < 1) return PGF_INVALID;
  const SparseDev &sp = h->sp;
  if (!h->sparse || !sp.bor.bk || sp.bor.bkp % 64)
    return fail(h, PGF_INVALID, "pgf_debug_border_gram_time: a border with kp a multiple of 64");
  if (!sp.cnt.stat_bfactor) return fail(h, PGF_NOT_READY, "no factor phase has run on this border yet");
  (void)hipSetDevice(h->device);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  HIPCHK(h, sp_borderL_gram_time(h->stream, sp, reps, ms_mfma, ms_fma));
  return PGF_OK;
}

int pgf_sparse_set_factor_split(pgf_handle h, int on) {
  if (!h) return PGF_INVALID;
  if (!h->sparse) return fail(h, PGF_INVALID, "pgf_sparse_set_factor_split: banded handles only");
  SparseDev &sp = h->sp;
  const bool want = on != 0;
  if (want == sp.blk.split) return PGF_OK;
  if (!want && sp_border_large(sp))
    return fail(h, PGF_INVALID, "a large border needs the factor / solve split");
  (void)hipSetDevice(h->device);
  HIPCHK(h, hipStreamSynchronize(h->stream));
  sp.blk.split = want;
  invalidate_factor(h);  // (a bordered band's factor phase depends on the route too)
  // the blocks anew, with or without the kept multipliers (nothing to do at B = 8: it keeps none)
  return sp.active && sp.blk.B > 8 ? sp_alloc_blocks(h, sp.blk.B) : PGF_OK;
}

int pgf_debug_band_stats(pgf_handle h, int *reductions, int *solve_phases, int *panel_solves) {
  if (!h) return PGF_INVALID;
  if (reductions) *reductions = h->sp.cnt.stat_bw_reduce;
  if (solve_phases) *solve_phases = h->sp.cnt.stat_bw_solve;
  if (panel_solves) *panel_solves = h->sp.cnt.stat_bw_panel;
  return PGF_OK;
}

int pgf_sparse_set_block_size(pgf_handle h, int B) {
  if (!h) return PGF_INVALID;
  if (!h->sparse || !h->sp.active) return fail(h, PGF_NOT_READY, "pgf_sparse_set_pattern first");
  if (B != 0 && B != 8 && B != 16 && B != 32 && B != 64)
    return fail(h, PGF_INVALID, "block size must be 0 (automatic), 8, 16, 32 or 64");
  if (B != 0 && B < h->sp.pat.bw)
    return fail(h, PGF_INVALID, "block size is smaller than the half-bandwidth");
  (void)hipSetDevice(h->device);
  const int want = B ? B : auto_block_size(h->sp.pat.bw);
  if (want == h->sp.blk.B) return PGF_OK;
  if (want == 8 && sp_border_large(h->sp))
    return fail(h, PGF_INVALID, "a large border needs a wide remainder (block size 16, 32 or 64)");
  int rc;
  if ((rc = sp_alloc_blocks(h, want))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  invalidate_factor(h);
  return PGF_OK;
}

int pgf_sparse_set_values(pgf_handle h, const double *Hval, const double *Jval) {
  if (!h) return PGF_INVALID;
  if (!h->sparse || !h->sp.active) return fail(h, PGF_NOT_READY, "pgf_sparse_set_pattern first");
  if ((h->sp.pat.nnzH && !Hval) || (h->sp.pat.nnzJ && !Jval)) return fail(h, PGF_INVALID, "null values");
  (void)hipSetDevice(h->device);
  int rc;
  if ((rc = up(h, h->sp.pat.Hval, Hval, (size_t)h->sp.pat.nnzH * sizeof(double)))) return rc;
  if ((rc = up(h, h->sp.pat.Jval, Jval, (size_t)h->sp.pat.nnzJ * sizeof(double)))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->sp.pat.values_set = true;
  h->ls.hat_fresh = false;
  h->derivs_set = true;
  invalidate_factor(h);
  return PGF_OK;
}

}  // extern "C"
