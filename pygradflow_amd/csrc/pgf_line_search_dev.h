// Device bodies of the Armijo line search (reference newton.py:244-299) for a linear-quadratic
// problem: the per-entry terms, the summation order and the decision, shared by the single
// handle's kernels (pgf_line_search.hip) and their batched twins (pgf_batch_line_search.hip), so that
// both give the same bits.  nblk workgroups of 256 threads cover the n + m entries of ONE problem;
// bid is the workgroup's index among them (the single handle: blockIdx.x of gridDim.x; a batch:
// blockIdx.x of gridDim.x with the instance in blockIdx.z).  Every includer is compiled with
// -ffp-contract=off: the trial masks are the expressions of k_active_set.  No atomics on doubles:
// per-workgroup partial sums, summed in a fixed order by the last workgroup to arrive (the ticket of
// k_unscaled_res_norm).
#pragma once

#include "pgf_line_search.h"
#include "pgf_reduce_dev.h"

#define LS_ACTIVE_EPS 1e-8  // reference implicit_func.py:44

// lamb x - P(p), p = lamb xhat - g clipped where it leaves [slb - eps, sub + eps]: an x row of
// ScaledImplicitFunc.value_at with the mask of its own point (implicit_func.py:219-231, 246)
__device__ __forceinline__ double ls_fx(double lamb, double lxh, double x, double g, double lo, double hi,
                                        bool *act) {
  double p = lxh - g;
  *act = (p < lo - LS_ACTIVE_EPS) || (p > hi + LS_ACTIVE_EPS);
  if (*act) p = fmin(fmax(p, lo), hi);
  return lamb * x - p;
}
__device__ __forceinline__ double ls_fy(double lamb, double lyh, double y, double c) {
  const double t = lyh + c;
  return -(lamb * y - t);
}

// whether this workgroup is the last of the problem's nblk to arrive (its partials are published first)
__device__ __forceinline__ bool ls_last_block(unsigned *ticket, unsigned nblk) {
  __shared__ bool last;
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == nblk - 1u;
  __syncthreads();
  if (last) __threadfence();
  return last;
}

// The ladder: every trial merit, merit0, the slope and the decision into blk (layout: pgf_line_search.h).
// red: LS_TERMS doubles per workgroup.  The ticket is re-zeroed by its last arriver.
__device__ __forceinline__ void b_ls_ladder(int bid, unsigned nblk, int n, int m, double lamb, double newton_tol,
    const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ xhat,
    const double *__restrict__ yhat, const double *__restrict__ dx, const double *__restrict__ dy,
    const double *__restrict__ g, const double *__restrict__ c, const double *__restrict__ v,
    const double *__restrict__ u, const double *__restrict__ slb, const double *__restrict__ sub,
    double *red, double *blk, unsigned *ticket) {
  __shared__ double part[4][LS_TERMS];
  __shared__ double fin[8][LS_TERMS];
  __shared__ double tot[LS_TERMS];
  const int tid = threadIdx.x;
  const int i = bid * 256 + tid;
  double t[LS_TERMS];
#pragma unroll
  for (int k = 0; k < LS_TERMS; ++k) t[k] = 0.0;
  if (i < n) {
    const double xi = x[i], d = dx[i], gi = g[i], vi = v[i], lo = slb[i], hi = sub[i];
    const double lxh = lamb * xhat[i];
    bool act;
    const double f0 = ls_fx(lamb, lxh, xi, gi, lo, hi, &act);
    t[LS_TRIALS] = f0 * f0;
    t[LS_TRIALS + 1] = f0 * (lamb * d + (act ? 0.0 : vi));
    double a = 1.0;
#pragma unroll
    for (int k = 0; k < LS_TRIALS; ++k) {
      const double f = ls_fx(lamb, lxh, xi - a * d, gi - a * vi, lo, hi, &act);
      t[k] = f * f;
      a *= 0.5;
    }
  } else if (i < n + m) {
    const int r = i - n;
    const double yr = y[r], d = dy[r], cr = c[r], ur = u[r];
    const double lyh = lamb * yhat[r];
    const double f0 = ls_fy(lamb, lyh, yr, cr);
    t[LS_TRIALS] = f0 * f0;
    t[LS_TRIALS + 1] = f0 * (lamb * d - ur);
    double a = 1.0;
#pragma unroll
    for (int k = 0; k < LS_TRIALS; ++k) {
      const double f = ls_fy(lamb, lyh, yr - a * d, cr - a * ur);
      t[k] = f * f;
      a *= 0.5;
    }
  }
#pragma unroll
  for (int k = 0; k < LS_TERMS; ++k) {
    const double s = wave_sum(t[k]);
    if ((tid & 63) == 0) part[tid >> 6][k] = s;
  }
  __syncthreads();
  if (tid < LS_TERMS)
    red[(size_t)bid * LS_TERMS + tid] = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
  if (!ls_last_block(ticket, nblk)) return;
  // term q of every workgroup: eight lanes take every eighth workgroup, then the eight in order
  const int q = tid & (LS_TERMS - 1), j = tid >> 5;
  double s = 0.0;
  for (unsigned b = j; b < nblk; b += 8) s += red[(size_t)b * LS_TERMS + q];
  fin[j][q] = s;
  __syncthreads();
  if (tid < LS_TERMS) {
    double w = 0.0;
    for (int p = 0; p < 8; ++p) w += fin[p][tid];
    tot[tid] = w;
  }
  __syncthreads();
  if (tid < LS_TRIALS) blk[LS_MERITS + tid] = 0.5 * tot[tid];
  if (tid != 0) return;
  const double merit0 = 0.5 * tot[LS_TRIALS], slope = tot[LS_TRIALS + 1];
  double alpha = 1.0, status = 0.0;
  int trials = 0;
  if (!(merit0 <= newton_tol)) {  // (newton.py:254: at or below it, the full step without a trial)
    status = 1.0;
    trials = LS_TRIALS;
    double a = 1.0;
    for (int k = 0; k < LS_TRIALS; ++k) {
      const double tm = 0.5 * tot[k];
      // the reference's sign and constant (newton.py:281-285)
      if (tm <= newton_tol || tm <= merit0 + 1e-4 * a * slope) {
        alpha = a;
        trials = k + 1;
        status = 0.0;
        break;
      }
      a *= 0.5;
    }
  }
  blk[LS_ALPHA] = alpha;
  blk[LS_NTRIALS] = (double)trials;
  blk[LS_MERIT0] = merit0;
  blk[LS_SLOPE] = slope;
  blk[LS_STATUS] = status;
  *ticket = 0u;
}

// StepResult(orig_iterate, alpha dx, alpha dy) (newton.py:296, step_solver.py:25-48): measured from
// the outer point, clipped as k_step_update clips, the length as k_final_reduce sums it.  Nothing
// when the block's status says failed.  (xn, yn) may be the current point's own vectors: each lane
// writes its own entry, and none is read here.
__device__ __forceinline__ void b_ls_finish(int bid, unsigned nblk, int n, int m, const double *__restrict__ xhat,
    const double *__restrict__ yhat, const double *__restrict__ dx, const double *__restrict__ dy,
    const double *__restrict__ lb, const double *__restrict__ ub, double *__restrict__ xn,
    double *__restrict__ yn, double *red, double *blk, unsigned *ticket) {
  __shared__ double part[4];
  if (blk[LS_STATUS] != 0.0) return;  // no trial accepted: the point stays
  const double alpha = blk[LS_ALPHA];
  const int tid = threadIdx.x;
  const int i = bid * 256 + tid;
  double sq = 0.0;
  if (i < n) {
    double d = alpha * dx[i];
    const double xi = xhat[i];
    double w = xi - d;
    const double lo = lb[i], hi = ub[i];
    if (w < lo) {
      w = lo;
      d = xi - lo;
    }
    if (w > hi) {
      w = hi;
      d = xi - hi;
    }
    xn[i] = w;
    sq = d * d;
  } else if (i < n + m) {
    const int r = i - n;
    const double d = alpha * dy[r];
    yn[r] = yhat[r] - d;
    sq = d * d;
  }
  sq = wave_sum(sq);
  if ((tid & 63) == 0) part[tid >> 6] = sq;
  __syncthreads();
  if (tid == 0) red[bid] = (part[0] + part[1]) + (part[2] + part[3]);
  if (!ls_last_block(ticket, nblk)) return;
  double s = 0.0;
  for (unsigned b = tid; b < nblk; b += 256) s += red[b];
  s = wave_sum(s);
  __syncthreads();  // (part is read above by lane 0 of this same workgroup)
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    blk[LS_DIFF] = sqrt((part[0] + part[1]) + (part[2] + part[3]));
    *ticket = 0u;
  }
}
