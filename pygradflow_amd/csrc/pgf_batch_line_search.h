// The Armijo line search of the Globalized policy for every instance of a device batch
// (PGF_BATCH_LINE_SEARCH; kernels in pgf_batch_line_search.hip, bodies in pgf_line_search_dev.h, host
// side in pgf_api_batch_line_search.hip).  gfx950 (MI355X / CDNA4) only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgf_line_search.h"

// One entry per instance, dense or banded: what the ladder and the finish read and write.  (x, y):
// the instance's current point, which the finish overwrites with the new one; (g, c) at (x, y);
// (v, u) the direction's images; red: LS_TERMS doubles per workgroup of 256 entries; blk: the
// instance's block.  ctl, ps: as in BInst.  bad: a word that is non-zero when the instance's
// direction failed (dense: its word of flags_out, written by kb_step_final; band: its pivot flags).
// stat / guard (band; null on a dense batch): the residual pairs of the instance's solve and
// (guard on, refine_tol) of its handle -- an instance above its tolerance sits the stage out and is
// repaired on its handle, where the dense batch's sampled guard has set bit 2 of `bad' already.
struct LsInst {
  double *x, *y;
  const double *xhat, *yhat, *dx, *dy, *g, *c, *v, *u, *slb, *sub, *lb, *ub;
  double *red, *blk;
  const int *ctl;
  const double *ps;
  const int *bad;
  const double *stat, *guard;
};
// An instance's block: the single handle's LS_COPY doubles (pgf_line_search.h), behind them [36] the
// two tickets and [37] non-zero when the instance sat the stage out (frozen, or a failed direction):
// written by every ladder launch, read by the finish and the host.
#define LSB_TICKETS LS_COPY
#define LSB_SAT_OUT 37
#define LSB_STRIDE 38

// nred: residual pairs per instance (band batches).  Both are one launch for the whole batch, grid
// (ceil((n + m) / 256), 1, B), whatever any instance decides.
void batch_launch_ls_ladder(hipStream_t s, const LsInst *tab, int B, int n, int m, int nred, double newton_tol);
void batch_launch_ls_finish(hipStream_t s, const LsInst *tab, int B, int n, int m);
