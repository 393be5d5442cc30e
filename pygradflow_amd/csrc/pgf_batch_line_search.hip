// Batched twins of k_ls_ladder / k_ls_finish (pgf_line_search.hip): the Armijo line search of every
// instance of a device batch in two launches, the instance in blockIdx.z as in the kb_* kernels.
// Each instance has its own partial-sum slice, its own two tickets and its own block; the last
// workgroup of an instance sums its partials in the single handle's order (pgf_line_search_dev.h) and
// decides its k.  lamb is the instance's own (BPS_LAMB): instances have their own dt.  A frozen
// instance and one whose direction failed return at once, in both launches.  Compiled with
// -ffp-contract=off.
#include "pgf_batch_line_search.h"

#include "pgf_batch.h"
#include "pgf_line_search_dev.h"

// Whether the instance sits the stage out; the same for every thread of the workgroup.  The band
// batch's guard: band_residual_rel_of (pgf_api_band.hip) over the instance's pairs -- max |r| over
// max (|K| |x| + |rhs|), +inf for a NaN or overflowed numerator, denominator 1 when it is 0 -- above
// the handle's refine_tol; a max is order-free, so the host comes to the same verdict.
__device__ __forceinline__ bool ls_sits_out(const LsInst &L, int nred) {
  if (L.ctl[3] || L.bad[0]) return true;
  if (!L.stat || L.guard[0] == 0.0) return false;
  __shared__ double pr[4], pd[4];
  __shared__ int pb[4];
  const int tid = threadIdx.x;
  double r = 0.0, den = 0.0;
  int broken = 0;
  for (int k = tid; k < nred; k += 256) {
    const double rk = L.stat[2 * k];
    if (!(rk == rk) || !(rk <= 1.79e308))
      broken = 1;
    else
      r = fmax(r, rk);
    den = fmax(den, L.stat[2 * k + 1]);
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    r = fmax(r, __shfl_xor(r, off));
    den = fmax(den, __shfl_xor(den, off));
    broken |= __shfl_xor(broken, off);
  }
  if ((tid & 63) == 0) {
    pr[tid >> 6] = r;
    pd[tid >> 6] = den;
    pb[tid >> 6] = broken;
  }
  __syncthreads();
  r = fmax(fmax(pr[0], pr[1]), fmax(pr[2], pr[3]));
  den = fmax(fmax(pd[0], pd[1]), fmax(pd[2], pd[3]));
  broken = pb[0] | pb[1] | pb[2] | pb[3];
  const double rel = broken ? __builtin_huge_val() : r / (den > 0.0 ? den : 1.0);
  return !(rel <= L.guard[1]);
}

__global__ __launch_bounds__(256) void kb_ls_ladder(const LsInst *__restrict__ tab, int n, int m, int nred,
                                                    double newton_tol) {
  const LsInst &L = tab[blockIdx.z];
  const bool out = ls_sits_out(L, nred);
  if (blockIdx.x == 0 && threadIdx.x == 0) L.blk[LSB_SAT_OUT] = out ? 1.0 : 0.0;
  if (out) return;
  b_ls_ladder(blockIdx.x, gridDim.x, n, m, L.ps[BPS_LAMB], newton_tol, L.x, L.y, L.xhat, L.yhat, L.dx, L.dy, L.g,
              L.c, L.v, L.u, L.slb, L.sub, L.red, L.blk, reinterpret_cast<unsigned *>(L.blk + LSB_TICKETS));
}

// the new point replaces the instance's current one in place
__global__ __launch_bounds__(256) void kb_ls_finish(const LsInst *__restrict__ tab, int n, int m) {
  const LsInst &L = tab[blockIdx.z];
  if (L.blk[LSB_SAT_OUT] != 0.0) return;
  b_ls_finish(blockIdx.x, gridDim.x, n, m, L.xhat, L.yhat, L.dx, L.dy, L.lb, L.ub, L.x, L.y, L.red, L.blk,
              reinterpret_cast<unsigned *>(L.blk + LSB_TICKETS) + 1);
}

void batch_launch_ls_ladder(hipStream_t s, const LsInst *tab, int B, int n, int m, int nred, double newton_tol) {
  const int nb = (n + m + 255) / 256;
  if (!nb) return;
  hipLaunchKernelGGL(kb_ls_ladder, dim3(nb, 1, B), dim3(256), 0, s, tab, n, m, nred, newton_tol);
}

void batch_launch_ls_finish(hipStream_t s, const LsInst *tab, int B, int n, int m) {
  const int nb = (n + m + 255) / 256;
  if (!nb) return;
  hipLaunchKernelGGL(kb_ls_finish, dim3(nb, 1, B), dim3(256), 0, s, tab, n, m);
}
