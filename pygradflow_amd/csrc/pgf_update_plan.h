// The lazy trailing-update plan of the dense LDL^T look-ahead schedule (pgf_factor2.hip): the job
// tables its launches carry, THE tile number -> tile mapping that the device workers and the host
// walk share, and the host-side planner (pgf_update_plan.hip: no kernel, no HIP call).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

// Jobs of one lazy update launch: job q brings column block [col0, col0 + 256) -- rows from
// rowstart (or the diagonal, whichever is lower) -- from "blocks < kc0 / 256 applied" to
// "blocks < (kc0 + KB) / 256 applied"; its 128 x 128 tiles are numbered tile_begin[q] ...
#define UPD_MAXJOBS 96
#define UPD_TM 64  // tile rows (x 128 columns): with the persistent tile loop the finer unit packs
                   // a launch's work into fewer idle CU-rounds (128: ~260 units of 37 us over 253 CUs = two
                   // rounds, half of the second one idle)
struct UpdJobs {
  int njobs;
  int tile_begin[UPD_MAXJOBS + 1];
  int col0[UPD_MAXJOBS], rowstart[UPD_MAXJOBS], kc0[UPD_MAXJOBS], KB[UPD_MAXJOBS];
  int ntc[UPD_MAXJOBS];  // 128-wide tile columns of the job (2 per column block; adjacent column
                         // blocks with the same K-range share a job: large N, eager plan)
  // a leading segment of the K-range in the pre-eliminated block's panel (UpdVirt): columns
  // [kc0v, kc0v + KBv) of V first, then columns [kc0, kc0 + KB) of K (either may be empty) -- ONE
  // job, one pass over the tiles: two jobs on the same tiles of a launch would race
  int kc0v[UPD_MAXJOBS], KBv[UPD_MAXJOBS];
};
// The pre-eliminated block (DenseLdlt::V): panel rows V[i][.], D-scaling vd.
struct UpdVirt {
  const double *V;
  int64_t ldv;
  const double *vd;
};

// THE tile number -> tile mapping, on the device (update_job_tile, pgf_factor2.hip) and on the
// host (pgf_debug_update_plan).  Tile t of a launch's job table belongs to job q and covers rows
// from i0 (UPD_TM of them) and columns from j0 (128): a job's tile columns in turn, the rows of
// each from max(rowstart, column start) down to row nrows - 1.  false: t is past the end.
__host__ __device__ inline bool upd_tile(const UpdJobs &jobs, int t, int N, int nrows, int &q, int &i0, int &j0) {
  if (t >= jobs.tile_begin[jobs.njobs]) return false;
  q = 0;
  while (t >= jobs.tile_begin[q + 1]) ++q;
  t -= jobs.tile_begin[q];
  const int col0 = jobs.col0[q], rs = jobs.rowstart[q];
  int jt = col0, it = rs > jt ? rs : jt;
  for (int c = 0; c < jobs.ntc[q]; ++c) {
    jt = col0 + 128 * c;
    it = rs > jt ? rs : jt;
    const int nc = (jt < N && it < nrows) ? (nrows - it + UPD_TM - 1) / UPD_TM : 0;
    if (t < nc) break;
    t -= nc;
  }
  i0 = it + UPD_TM * t;
  j0 = jt;
  return true;
}

// The trailing update beside the chain.  Launch L (chain D(L), panels of blocks < L available)
// must leave column block L complete below its diagonal block (T(L) reads it) and column block
// L + 1 complete through block L - 1 (k_update_diag / D(L + 1)); every other (column block,
// block) pair may wait.  Work is counted in tile-blocks (one 128 x 128 tile x K-depth 256 =
// one workgroup for ~45 us); what hides behind a chain of ~66 us is a little less than two
// rounds over 255 CUs.  Earliest deadline first with a per-launch budget: nearest column block
// first, an optional job takes at most `cap` pending blocks at once (its tiles run for cap x
// 45 us).  Too small a budget pushes work against the deadlines, where it comes back as a few
// very deep tiles on a few CUs; too large a one front-loads the launches as the eager schedule
// does.  The budget is therefore chosen per factorisation: the candidate with the smallest
// estimated total time (UpdPlan::cost) -- the reduced size changes from step to step.
struct UpdPlan {
  UpdJobs first;                // beside the chain of column block 0 (virtual blocks only)
  std::vector<UpdJobs> launch;  // [L - 1]: beside the chain of column block k + 1
  double cost = 0.0;            // estimated sum of launch times in units of one tile-block
  int budget = 0;               // the per-launch budget it was made with (UPD_NO_LIMIT: eager)
};
#define UPD_NO_LIMIT (1 << 30)

// the plan of one factorisation for a given budget (tile-blocks per launch) and cap; OB = LDLT_OB
void plan_updates(UpdPlan &pl, int N, int nrows, int OB, int budget, int cap, int vdepth = 0);
// The plan production factorises (N, nrows, vdepth) with: PGF_LAZY_BUDGET / PGF_LAZY_CAP where
// set, else the budget with the smallest estimated time among 60 candidates and the eager plan,
// searched once per 128-row size class.  Cached per thread: the reference is good until the
// thread's next call.  env = false (pgf_debug_update_plan): the two variables are ignored.
const UpdPlan &update_plan_for(int N, int nrows, int vdepth, bool env = true);
