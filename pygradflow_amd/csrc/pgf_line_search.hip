// The Armijo line search of the Globalized policy (reference newton.py:244-299) for a
// linear-quadratic problem, in two launches whatever the number of trials.  With the direction's
// images u = A dx and v = Q dx + A'(rho u + dy), the trial point (x - a dx, y - a dy) has
// c - a u and g - a v: the 30 trial merits of the ladder a = 2^-k are 30 sums over the same n + m
// entries, loaded once.  Compiled with -ffp-contract=off like the other step kernels: the trial
// masks are the expressions of k_active_set.  No atomics on doubles: per-workgroup partial sums,
// summed in a fixed order by the last workgroup to arrive (the ticket of k_unscaled_res_norm).
// The kernels' bodies live in pgf_line_search_dev.h.
#include "pgf_line_search.h"

#include "pgf_line_search_dev.h"

// (bodies: pgf_line_search_dev.h, shared with the batched twins of pgf_batch_line_search.hip)
__global__ __launch_bounds__(256) void k_ls_ladder(int n, int m, double lamb, double newton_tol,
    const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ xhat,
    const double *__restrict__ yhat, const double *__restrict__ dx, const double *__restrict__ dy,
    const double *__restrict__ g, const double *__restrict__ c, const double *__restrict__ v,
    const double *__restrict__ u, const double *__restrict__ slb, const double *__restrict__ sub,
    double *red, double *blk, unsigned *ticket) {
  b_ls_ladder(blockIdx.x, gridDim.x, n, m, lamb, newton_tol, x, y, xhat, yhat, dx, dy, g, c, v, u, slb, sub, red,
              blk, ticket);
}

__global__ __launch_bounds__(256) void k_ls_finish(int n, int m, const double *__restrict__ xhat,
    const double *__restrict__ yhat, const double *__restrict__ dx, const double *__restrict__ dy,
    const double *__restrict__ lb, const double *__restrict__ ub, double *__restrict__ xn,
    double *__restrict__ yn, double *red, double *blk, unsigned *ticket) {
  b_ls_finish(blockIdx.x, gridDim.x, n, m, xhat, yhat, dx, dy, lb, ub, xn, yn, red, blk, ticket);
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
