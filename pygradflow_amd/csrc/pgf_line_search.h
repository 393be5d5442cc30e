// Launch wrappers of pgf_line_search.hip: the Armijo line search of the Globalized policy
// (reference newton.py:244-299) for a linear-quadratic problem, all asynchronous on the stream.
#pragma once

#include <hip/hip_runtime.h>

#define LS_TRIALS 30  // the reference's max_it (newton.py:270)
#define LS_TERMS 32   // sums of one ladder launch: the 30 trials, merit0, the slope
// The line search's device block (doubles): [0] alpha, [1] trials evaluated (0: merit0 <= newton_tol,
// the full step without a trial), [2] merit0, [3] slope, [4, 34) the trial merits, [34] status
// (0 accepted, 1 no trial accepted), [35] ||(dx, alpha dy)|| of the step taken (k_ls_finish);
// behind what the host reads: [36] the two tickets of the last-workgroup reductions.
#define LS_ALPHA 0
#define LS_NTRIALS 1
#define LS_MERIT0 2
#define LS_SLOPE 3
#define LS_MERITS 4  // LS_TRIALS doubles
#define LS_STATUS 34
#define LS_DIFF 35
#define LS_COPY 36
#define LS_ALLOC 37

// Every trial merit 1/2 ||F||^2 at (x - a_k dx, y - a_k dy), a_k = 2^-k, with g - a_k v and
// c - a_k u and the trial's own tau-less mask; merit0 and the slope F . [lamb dx + keep v; lamb dy - u]
// at (x, y); the decision.  red: 32 doubles per workgroup of 256 entries.
void launch_ls_ladder(hipStream_t s, int n, int m, double lamb, double newton_tol, const double *x,
                      const double *y, const double *xhat, const double *yhat, const double *dx,
                      const double *dy, const double *g, const double *c, const double *v, const double *u,
                      const double *slb, const double *sub, double *red, double *blk);
// xn = clip(xhat - alpha dx), yn = yhat - alpha dy, blk[35] = ||(dx rewritten where clipped, alpha dy)||;
// nothing when the block's status says failed
void launch_ls_finish(hipStream_t s, int n, int m, const double *xhat, const double *yhat, const double *dx,
                      const double *dy, const double *lb, const double *ub, double *xn, double *yn,
                      double *red, double *blk);
