// Host side of the lazy trailing-update plan (pgf_update_plan.h): the planner, its budget search
// and the per-thread caches of the look-ahead schedule of pgf_factor2.hip.  No kernel and no HIP
// call: pgf_debug_update_plan walks the same plans without a GPU.
#include "pgf_update_plan.h"

#include "pgf_env.h"
#include "pgf_ldlt.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <unordered_map>

// budget of one lazy update launch in tile-blocks (128 x 128 tile x K-depth 256; 255 CUs take
// one each per ~47 us) and the number of pending blocks an optional job may take at once;
// PGF_LAZY_BUDGET=0: no limit = the eager schedule (every launch applies block k everywhere)
static int lazy_budget() {
  static const int b = env_int("PGF_LAZY_BUDGET", 420);
  return b > 0 ? b : UPD_NO_LIMIT;
}
// pending blocks an optional job takes at once: 2 in the natural order; 4 with a pre-eliminated
// block (its virtual blocks are all pending from the start: deeper passes over the same C tiles
// re-read them less often; measured 2.03 -> 2.015 ms at config 2, 3 and 5+ are slower)
static int lazy_cap(int vdepth, bool env) {
  static const int c = getenv("PGF_LAZY_CAP") ? std::max(1, atoi(getenv("PGF_LAZY_CAP"))) : 0;
  return (env && c) ? c : (vdepth > 0 ? 4 : 2);
}
// ~66 us chain (DPP elimination) / time of one tile-block (64 x 128 x 256: ~21 us, 128 x 128: ~40 us)
static double plan_chain_units() { return 66.0 / (UPD_TM == 64 ? 21.0 : 40.0); }

// A pre-eliminated block of depth vdepth (DenseLdlt::V) counts as nv = ceil(vdepth / OB) column
// blocks that are factorised before the first one: block indices below are unified, virtual blocks
// [0, nv) first, real block k at nv + k.  Updates commute, so the only deadlines are the usual
// ones -- a column block's diagonal tile complete before its chain, its rows below before its T --
// and the virtual blocks are pending work like any other: only the first diagonal block is due
// before the first chain (k_virtual_diag: small tiles, a few microseconds, the only exposed part);
// the rows below it and column block 1 follow beside that chain (stage `first'), the rest lazily.
void plan_updates(UpdPlan &pl, int N, int nrows, int OB, int budget, int cap, int vdepth) {
  const double chain_units = plan_chain_units();
  const int nblk = (N + OB - 1) / OB;
  const int nv = (vdepth + OB - 1) / OB;
  std::vector<int> done(nblk + 2, 0);
  pl.launch.assign(std::max(0, nblk - 1), UpdJobs());
  pl.first.njobs = 0;
  pl.first.tile_begin[0] = 0;
  pl.cost = 0.0;
  pl.budget = budget;
  auto tiles = [&](int col0, int rowstart) {
    int n = 0;
    for (int c = 0; c < 2; ++c) {
      const int j0 = col0 + 128 * c;
      if (j0 >= N) continue;
      const int i0 = std::max(rowstart, j0);
      if (i0 < nrows) n += (nrows - i0 + UPD_TM - 1) / UPD_TM;
    }
    return n;
  };
  // stage -1: first, k >= 0: the launch beside the chain of column block k + 1
  for (int st = (nv > 0 ? -1 : 0); st < nblk - 1; ++st) {
    const int k = st;
    const int avail = st < 0 ? nv - 1 : nv + k;  // newest block whose panel exists
    UpdJobs jb;
    jb.njobs = 0;
    int units = 0, maxdepth = 0, cnt[UPD_MAXJOBS];
    // unified blocks [p0, p1]: the virtual part and the real part are the two segments of one job
    auto add = [&](int J, int rowstart, int p0, int p1) {
      if (p1 < p0) return;
      int kc0v = 0, KBv = 0, kc0 = 0, KB = 0;
      if (p0 < nv) {
        const int v1 = std::min(p1, nv - 1);
        kc0v = p0 * OB;
        KBv = std::min((v1 + 1) * OB, vdepth) - p0 * OB;
      }
      if (p1 >= nv) {
        const int r0 = std::max(p0, nv) - nv, r1 = p1 - nv;
        kc0 = r0 * OB;
        KB = (r1 - r0 + 1) * OB;
      }
      const int depth = p1 - p0 + 1;
      const int n = tiles(J * OB, rowstart);
      if (!n || KB + KBv <= 0) return;
      units += n * depth;
      maxdepth = std::max(maxdepth, depth);
      // a whole column block right behind the previous job's, same K-range: one job
      if (jb.njobs > 0 && rowstart == J * OB) {
        const int q = jb.njobs - 1;
        if (jb.rowstart[q] == jb.col0[q] && jb.col0[q] + 128 * jb.ntc[q] == J * OB && jb.kc0[q] == kc0 &&
            jb.KB[q] == KB && jb.kc0v[q] == kc0v && jb.KBv[q] == KBv) {
          jb.ntc[q] += OB / 128;
          cnt[q] += n;
          return;
        }
      }
      const int q = jb.njobs++;
      jb.col0[q] = J * OB;
      jb.rowstart[q] = rowstart;
      jb.kc0[q] = kc0;
      jb.KB[q] = KB;
      jb.kc0v[q] = kc0v;
      jb.KBv[q] = KBv;
      jb.ntc[q] = OB / 128;
      cnt[q] = n;
    };
    int Jopt;  // first column block whose pending work is optional at this stage
    const int lim = budget;
    if (st == -1) {
      add(0, std::min(OB, N), done[0], avail);  // (its diagonal block: k_virtual_diag)
      done[0] = avail + 1;
      if (nblk > 1) {
        add(1, OB, done[1], avail);
        done[1] = avail + 1;
      }
      Jopt = 2;
    } else {
      const int c1 = (k + 1) * OB, nb1 = std::min(OB, N - c1), row0 = c1 + nb1;
      if (done[k + 1] <= avail) add(k + 1, row0, done[k + 1], avail);
      done[k + 1] = avail + 1;
      if (k + 2 < nblk && done[k + 2] <= avail) {
        add(k + 2, (k + 2) * OB, done[k + 2], avail);
        done[k + 2] = avail + 1;
      }
      Jopt = k + 3;
    }
    for (int J = Jopt; J < nblk; ++J) {
      const int pend = avail + 1 - done[J];
      if (pend <= 0) continue;
      // (room is kept for the jobs that must run; what is skipped here stays pending)
      if (units >= lim || jb.njobs >= UPD_MAXJOBS - 2) break;
      const int take = std::min(pend, cap);
      add(J, J * OB, done[J], done[J] + take - 1);
      done[J] += take;
    }
    // deepest jobs first: their tiles take longest
    int order[UPD_MAXJOBS];
    for (int q = 0; q < jb.njobs; ++q) order[q] = q;
    std::stable_sort(order, order + jb.njobs,
                     [&](int a, int b) { return jb.KB[a] + jb.KBv[a] > jb.KB[b] + jb.KBv[b]; });
    UpdJobs &js = st == -1 ? pl.first : pl.launch[k];
    js.njobs = jb.njobs;
    js.tile_begin[0] = 0;
    for (int q = 0; q < jb.njobs; ++q) {
      const int o = order[q];
      js.col0[q] = jb.col0[o];
      js.rowstart[q] = jb.rowstart[o];
      js.kc0[q] = jb.kc0[o];
      js.KB[q] = jb.KB[o];
      js.ntc[q] = jb.ntc[o];
      js.kc0v[q] = jb.kc0v[o];
      js.KBv[q] = jb.KBv[o];
      js.tile_begin[q + 1] = js.tile_begin[q] + cnt[o];
    }
    // list-scheduling estimate of the launch: work / 253 CUs, at least the deepest tile, in
    // whole tile times; and never less than the chain
    const double t = std::max((double)maxdepth, std::ceil(units / 253.0));
    pl.cost += std::max(chain_units, t);
  }
}

// The search (about 60 candidate plans): the eager plan, then every budget of the range that
// beats the best so far.  Leaves the winner in `best'.
static void search_budget(UpdPlan &best, int N, int nrows, int OB, int cap, int vdepth) {
  plan_updates(best, N, nrows, OB, UPD_NO_LIMIT, cap, vdepth);  // eager
  for (int b = 200 * (128 / UPD_TM); b <= 1400 * (128 / UPD_TM); b += 20 * (128 / UPD_TM)) {
    UpdPlan cand;
    plan_updates(cand, N, nrows, OB, b, cap, vdepth);
    if (cand.cost < best.cost - 1e-9) best = std::move(cand);
  }
}

const UpdPlan &update_plan_for(int N, int nrows, int vdepth, bool env) {
  // cached per (N, nrows, depth of the pre-eliminated block): a Newton iteration refactorises
  // the same size many times.  The search once per 128-row size class: the winning budget
  // depends on the tile counts, and the reduced size moves by a few rows from step to step when
  // the active set churns (config 5b: a new N every step).  [1]: the environment honoured.
  struct Cache {
    int N = -1, R = -1, V = -1;
    UpdPlan plan;
    std::unordered_map<int, int> budget_of;
  };
  static thread_local Cache caches[2];
  Cache &c = caches[env ? 1 : 0];
  if (c.N == N && c.R == nrows && c.V == vdepth) return c.plan;
  constexpr int OB = LDLT_OB;
  const int cap = lazy_cap(vdepth, env);
  if (env && getenv("PGF_LAZY_BUDGET")) {
    plan_updates(c.plan, N, nrows, OB, lazy_budget(), cap, vdepth);
  } else {
    const int key = (nrows + 127) / 128 + 4096 * ((vdepth + 127) / 128);
    auto it = c.budget_of.find(key);
    if (it == c.budget_of.end()) {
      search_budget(c.plan, N, nrows, OB, cap, vdepth);
      c.budget_of.emplace(key, c.plan.budget);
    } else {
      plan_updates(c.plan, N, nrows, OB, it->second, cap, vdepth);
    }
  }
  c.N = N;
  c.R = nrows;
  c.V = vdepth;
  return c.plan;
}
