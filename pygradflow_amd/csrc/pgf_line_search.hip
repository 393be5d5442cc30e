// The Armijo line search of the Globalized policy (reference newton.py:244-299) for a
// linear-quadratic problem, in two launches whatever the number of trials.  With the direction's
// images u = A dx and v = Q dx + A'(rho u + dy), the trial point (x - a dx, y - a dy) has
// c - a u and g - a v: the 30 trial merits of the ladder a = 2^-k are 30 sums over the same n + m
// entries, loaded once.  Compiled with -ffp-contract=off like the other step kernels: the trial
// masks are the expressions of k_active_set.  No atomics on doubles: per-workgroup partial sums,
// summed in a fixed order by the last workgroup to arrive (the ticket of k_unscaled_res_norm).
#include "pgf_line_search.h"

#include "pgf_reduce_dev.h"

#define ACTIVE_EPS 1e-8  // reference implicit_func.py:44

// lamb x - P(p), p = lamb xhat - g clipped where it leaves [slb - eps, sub + eps]: an x row of
// ScaledImplicitFunc.value_at with the mask of its own point (implicit_func.py:219-231, 246)
__device__ __forceinline__ double ls_fx(double lamb, double lxh, double x, double g, double lo, double hi,
                                        bool *act) {
  double p = lxh - g;
  *act = (p < lo - ACTIVE_EPS) || (p > hi + ACTIVE_EPS);
  if (*act) p = fmin(fmax(p, lo), hi);
  return lamb * x - p;
}
__device__ __forceinline__ double ls_fy(double lamb, double lyh, double y, double c) {
  const double t = lyh + c;
  return -(lamb * y - t);
}

// whether this workgroup is the last of the launch to arrive (its partials are published first)
__device__ __forceinline__ bool ls_last_block(unsigned *ticket) {
  __shared__ bool last;
  __threadfence();
  __syncthreads();
  if (threadIdx.x == 0) last = atomicAdd(ticket, 1u) == gridDim.x - 1u;
  __syncthreads();
  if (last) __threadfence();
  return last;
}

__global__ __launch_bounds__(256) void k_ls_ladder(int n, int m, double lamb, double newton_tol,
    const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ xhat,
    const double *__restrict__ yhat, const double *__restrict__ dx, const double *__restrict__ dy,
    const double *__restrict__ g, const double *__restrict__ c, const double *__restrict__ v,
    const double *__restrict__ u, const double *__restrict__ slb, const double *__restrict__ sub,
    double *red, double *blk, unsigned *ticket) {
  __shared__ double part[4][LS_TERMS];
  __shared__ double fin[8][LS_TERMS];
  __shared__ double tot[LS_TERMS];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * 256 + tid;
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
    red[(size_t)blockIdx.x * LS_TERMS + tid] = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
  if (!ls_last_block(ticket)) return;
  // term q of every workgroup: eight lanes take every eighth workgroup, then the eight in order
  const int q = tid & (LS_TERMS - 1), j = tid >> 5;
  double s = 0.0;
  for (unsigned b = j; b < gridDim.x; b += 8) s += red[(size_t)b * LS_TERMS + q];
  fin[j][q] = s;
  __syncthreads();
  if (tid < LS_TERMS) {
    double w = 0.0;
    for (int p = 0; p < 8; ++p) w += fin[p][tid];
    tot[tid] = w;
  }
  __syncthreads();
  if (tid < LS_TRIALS) blk[4 + tid] = 0.5 * tot[tid];
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
  blk[0] = alpha;
  blk[1] = (double)trials;
  blk[2] = merit0;
  blk[3] = slope;
  blk[34] = status;
  *ticket = 0u;
}

// StepResult(orig_iterate, alpha dx, alpha dy) (newton.py:296, step_solver.py:25-48): measured from
// the outer point, clipped as k_step_update clips, the length as k_final_reduce sums it
__global__ __launch_bounds__(256) void k_ls_finish(int n, int m, const double *__restrict__ xhat,
    const double *__restrict__ yhat, const double *__restrict__ dx, const double *__restrict__ dy,
    const double *__restrict__ lb, const double *__restrict__ ub, double *__restrict__ xn,
    double *__restrict__ yn, double *red, double *blk, unsigned *ticket) {
  __shared__ double part[4];
  if (blk[34] != 0.0) return;  // no trial accepted: the point stays
  const double alpha = blk[0];
  const int tid = threadIdx.x;
  const int i = blockIdx.x * 256 + tid;
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
  if (tid == 0) red[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
  if (!ls_last_block(ticket)) return;
  double s = 0.0;
  for (unsigned b = tid; b < gridDim.x; b += 256) s += red[b];
  s = wave_sum(s);
  __syncthreads();  // (part is read above by lane 0 of this same workgroup)
  if ((tid & 63) == 0) part[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    blk[35] = sqrt((part[0] + part[1]) + (part[2] + part[3]));
    *ticket = 0u;
  }
}

void launch_ls_ladder(hipStream_t s, int n, int m, double lamb, double newton_tol, const double *x,
                      const double *y, const double *xhat, const double *yhat, const double *dx,
                      const double *dy, const double *g, const double *c, const double *v, const double *u,
                      const double *slb, const double *sub, double *red, double *blk) {
  const int nb = (n + m + 255) / 256;
  if (!nb) return;
  unsigned *ticket = reinterpret_cast<unsigned *>(blk + LS_COPY);
  hipLaunchKernelGGL(k_ls_ladder, dim3(nb), dim3(256), 0, s, n, m, lamb, newton_tol, x, y, xhat, yhat, dx, dy,
                     g, c, v, u, slb, sub, red, blk, ticket);
}

void launch_ls_finish(hipStream_t s, int n, int m, const double *xhat, const double *yhat, const double *dx,
                      const double *dy, const double *lb, const double *ub, double *xn, double *yn,
                      double *red, double *blk) {
  const int nb = (n + m + 255) / 256;
  if (!nb) return;
  unsigned *ticket = reinterpret_cast<unsigned *>(blk + LS_COPY) + 1;
  hipLaunchKernelGGL(k_ls_finish, dim3(nb), dim3(256), 0, s, n, m, xhat, yhat, dx, dy, lb, ub, xn, yn, red,
                     blk, ticket);
}
