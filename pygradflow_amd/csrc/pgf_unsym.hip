// The reference's three UNSYMMETRIC step-solver formulations on the device (pgf_hip.h,
// pgf_set_formulation): assembly of the (n + m) x (n + m) Newton matrix straight into the pivoted
// LU's array, the right-hand side in the formulation's row order, the unscaled residual / mask of
// the Standard formulation and the step update from the full-length solution.
// Compiled with -ffp-contract=off: every matrix entry and every mask is meant to be bit-identical
// to the reference's numpy expression, so no multiply-add may be fused here.
//
// With A = active set, I = inactive set (ascending), Hl = H + lamb I_n, delta = lamb / (1 + lamb rho):
//   Standard   (standard_step_solver.py:40-92, ImplicitFunc.deriv), natural order:
//              row i in I: [e_i + dt H[i,:], dt J[:,i]^T]; row i in A: e_i; rows n + k: [-dt J, I_m]
//   Extended   (extended_step_solver.py:39-112), rows reordered, columns natural:
//              |A| unit rows e_a, then [Hl[I,:], J[:,I]^T], then [J, -delta I_m]
//   Asymmetric (asymmetric_step_solver.py:38-173): [[Hl, J^T], [J, -delta I_m]], natural order,
//              every active row overwritten by e_a
#include "pgf_unsym.h"

#include "../../include/pgf_hip.h"
#include "pgf_reduce_dev.h"

#define ACTIVE_EPS 1e-8  // reference implicit_func.py:44
#define UT 64            // tile edge of the assembly

// ---------------------------------------------------------------- assembly
// One 64 x 64 tile of M per workgroup of 64 x 4 lanes; every entry of the (n + m) x ld array is
// written exactly once (zeros and the padding columns included: no memset in front).  Only the
// lower triangle of H (and of the Gram matrix G = J^T J) is valid: an entry above the diagonal is
// H[j][i], and the J^T block is J[k][i] -- both are read ALONG the rows of H / J (lane = row index
// of the tile, coalesced while the tile's variables are contiguous) into an LDS tile and taken out
// of it transposed, so that the stores run along the rows of M.  Entries on and below the diagonal
// and the constraint rows are read in place.  Every source entry is loaded once.
// G != nullptr (device-resident Standard): the Hessian is H + rhoG * G, the rho J^T J term of
// aug_lag_deriv_xx(rho).
enum { ROW_NONE = 0, ROW_VAR = 1, ROW_UNIT = 2, ROW_CONS = 3 };

template <int FORM>
__global__ __launch_bounds__(256) void k_assemble_unsym(
    double *__restrict__ M, int64_t ld, int n, int m, const double *__restrict__ H, int64_t ldh,
    const double *__restrict__ J, int64_t ldj, const double *__restrict__ G, int64_t ldg, double rhoG,
    const uint8_t *__restrict__ mask, const int *__restrict__ idxI, const int *__restrict__ idxA,
    const int *__restrict__ counts, double dt, double lamb, double delta) {
  __shared__ double tile[UT][UT + 1];
  __shared__ int rkind[UT], ridx[UT];
  const int N = n + m;
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int r0 = blockIdx.y * UT, c0 = blockIdx.x * UT;
  if (ty == 0) {
    const int r = r0 + tx;
    int kind = ROW_NONE, idx = 0;
    if (r < n) {
      if (FORM == PGF_FORM_EXTENDED) {
        const int nA = counts[1];
        if (r < nA) {
          kind = ROW_UNIT;
          idx = idxA[r];
        } else {
          kind = ROW_VAR;
          idx = idxI[r - nA];
        }
      } else {
        kind = mask[r] ? ROW_UNIT : ROW_VAR;
        idx = r;
      }
    } else if (r < N) {
      kind = ROW_CONS;
      idx = r - n;
    }
    rkind[tx] = kind;
    ridx[tx] = idx;
  }
  __syncthreads();
  // transposed sources: lane tx = the tile row's variable i, ty + 4 u = the tile column j
  if (rkind[tx] == ROW_VAR) {
    const int i = ridx[tx];
#pragma unroll 4
    for (int u = 0; u < UT / 4; ++u) {
      const int jj = ty + 4 * u;
      const int j = c0 + jj;
      if (j < n) {
        if (j > i) {
          double v = H[(int64_t)j * ldh + i];
          if (G) v = v + rhoG * G[(int64_t)j * ldg + i];
          tile[jj][tx] = v;
        }
      } else if (j < N) {
        tile[jj][tx] = J[(int64_t)(j - n) * ldj + i];
      }
    }
  }
  __syncthreads();
  const int j = c0 + tx;
  if (j >= ld) return;
#pragma unroll 4
  for (int u = 0; u < UT / 4; ++u) {
    const int rr = ty + 4 * u;
    const int r = r0 + rr;
    if (r >= N) break;
    const int kind = rkind[rr], i = ridx[rr];
    double v = 0.0;
    if (kind == ROW_VAR) {
      if (j < n) {
        double hv;
        if (j <= i) {
          hv = H[(int64_t)i * ldh + j];
          if (G) hv = hv + rhoG * G[(int64_t)i * ldg + j];
        } else {
          hv = tile[tx][rr];
        }
        if (FORM == PGF_FORM_STANDARD) {
          v = dt * hv;
          if (j == i) v = 1.0 + v;
        } else {
          v = (j == i) ? hv + lamb : hv;
        }
      } else if (j < N) {
        const double t = tile[tx][rr];
        v = (FORM == PGF_FORM_STANDARD) ? dt * t : t;
      }
    } else if (kind == ROW_UNIT) {
      v = (j == i) ? 1.0 : 0.0;
    } else if (kind == ROW_CONS) {
      if (j < n) {
        const double t = J[(int64_t)i * ldj + j];
        v = (FORM == PGF_FORM_STANDARD) ? -dt * t : t;
      } else if (j - n == i) {
        v = (FORM == PGF_FORM_STANDARD) ? 1.0 : -delta;
      }
    }
    M[(int64_t)r * ld + j] = v;
  }
}

void launch_assemble_unsym(hipStream_t s, int form, double *M, int64_t ld, int n, int m, const double *H,
                           int64_t ldh, const double *J, int64_t ldj, const double *G, int64_t ldg,
                           double rhoG, const uint8_t *mask, const int *idxI, const int *idxA,
                           const int *counts, double dt, double lamb, double delta) {
  const int N = n + m;
  if (N == 0) return;
  const dim3 grid((unsigned)((ld + UT - 1) / UT), (unsigned)((N + UT - 1) / UT)), block(UT, 4);
#define LAUNCH_(F)                                                                                      \
  hipLaunchKernelGGL(k_assemble_unsym<F>, grid, block, 0, s, M, ld, n, m, H, ldh, J, ldj, G, ldg, rhoG, \
                     mask, idxI, idxA, counts, dt, lamb, delta)
  if (form == PGF_FORM_STANDARD)
    LAUNCH_(PGF_FORM_STANDARD);
  else if (form == PGF_FORM_EXTENDED)
    LAUNCH_(PGF_FORM_EXTENDED);
  else
    LAUNCH_(PGF_FORM_ASYMMETRIC);
#undef LAUNCH_
}

// ---------------------------------------------------------------- unscaled mask (Standard)
// p = x^ - dt g; with tau: ((1 - tau lamb) x + (tau lamb) x^) - tau g, left to right as numpy
// (UnscaledStepFunc.projection_initial); mask = p < lb - 1e-8 or p > ub + 1e-8
__global__ void k_unscaled_active_set(int n, int use_tau, double dt, double f_x, double f_x0, double tau,
                                      const double *__restrict__ xhat, const double *__restrict__ x,
                                      const double *__restrict__ g, const double *__restrict__ lb,
                                      const double *__restrict__ ub, uint8_t *__restrict__ mask) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double p;
  if (use_tau) {
    const double a = f_x * x[i];
    const double b = f_x0 * xhat[i];
    const double c = tau * g[i];
    p = (a + b) - c;
  } else {
    p = xhat[i] - dt * g[i];
  }
  const double lo = lb[i] - ACTIVE_EPS;
  const double hi = ub[i] + ACTIVE_EPS;
  mask[i] = (p < lo || p > hi) ? 1 : 0;
}

void launch_unscaled_active_set(hipStream_t s, int n, int use_tau, double dt, double f_x, double f_x0,
                                double tau, const double *xhat, const double *x, const double *g,
                                const double *lb, const double *ub, uint8_t *mask) {
  if (n)
    hipLaunchKernelGGL(k_unscaled_active_set, dim3((n + 255) / 256), dim3(256), 0, s, n, use_tau, dt, f_x,
                       f_x0, tau, xhat, x, g, lb, ub, mask);
}

// ---------------------------------------------------------------- residual + right-hand side
// F: the formulation's residual in natural order (Standard: the UNSCALED one,
// [x - P(x^ - dt g); y - (y^ + dt c)], implicit_func.py:102-199; Extended / Asymmetric: the scaled
// one of k_residual, [lamb x - P(lamb x^ - g); -(lamb y - (lamb y^ + c))]), P clipping only masked
// entries.  rhs (optional): the same in the formulation's row order --
//   Standard:   F;   Asymmetric: dt F_x on active rows, F_x on inactive ones, fact F_y;
//   Extended:   [dt F_x[A]; F_x[I]; fact F_y]  (pos = rank inside the own list, counts[1] = |A|)
template <int FORM>
__global__ void k_unsym_residual_rhs(int n, int m, double lamb, double dt, double fact,
                                     const double *__restrict__ xhat, const double *__restrict__ yhat,
                                     const double *__restrict__ x, const double *__restrict__ y,
                                     const double *__restrict__ g, const double *__restrict__ c,
                                     const double *__restrict__ lo, const double *__restrict__ hi,
                                     const uint8_t *__restrict__ mask, const int *__restrict__ pos,
                                     const int *__restrict__ counts, double *__restrict__ F,
                                     double *__restrict__ rhs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const bool act = mask[i] != 0;
    double f;
    if (FORM == PGF_FORM_STANDARD) {
      double p = xhat[i] - dt * g[i];
      if (act) p = fmin(fmax(p, lo[i]), hi[i]);
      f = x[i] - p;
    } else {
      double p = lamb * xhat[i] - g[i];
      if (act) p = fmin(fmax(p, lo[i]), hi[i]);
      f = lamb * x[i] - p;
    }
    F[i] = f;
    if (!rhs) return;
    if (FORM == PGF_FORM_STANDARD) {
      rhs[i] = f;
    } else if (FORM == PGF_FORM_ASYMMETRIC) {
      rhs[i] = act ? dt * f : f;
    } else {
      if (act)
        rhs[pos[i]] = dt * f;
      else
        rhs[counts[1] + pos[i]] = f;
    }
  } else if (i < n + m) {
    const int r = i - n;
    double f;
    if (FORM == PGF_FORM_STANDARD) {
      f = y[r] - (yhat[r] + dt * c[r]);
    } else {
      const double t = lamb * yhat[r] + c[r];
      f = -(lamb * y[r] - t);
    }
    F[i] = f;
    if (rhs) rhs[i] = (FORM == PGF_FORM_STANDARD) ? f : fact * f;
  }
}

void launch_unsym_residual_rhs(hipStream_t s, int form, int n, int m, double lamb, double dt, double fact,
                               const double *xhat, const double *yhat, const double *x, const double *y,
                               const double *g, const double *c, const double *lo, const double *hi,
                               const uint8_t *mask, const int *pos, const int *counts, double *F,
                               double *rhs) {
  const int N = n + m;
  if (N == 0) return;
  const dim3 grid((N + 255) / 256), block(256);
#define LAUNCH_(Fm)                                                                                    \
  hipLaunchKernelGGL(k_unsym_residual_rhs<Fm>, grid, block, 0, s, n, m, lamb, dt, fact, xhat, yhat, x, \
                     y, g, c, lo, hi, mask, pos, counts, F, rhs)
  if (form == PGF_FORM_STANDARD)
    LAUNCH_(PGF_FORM_STANDARD);
  else if (form == PGF_FORM_EXTENDED)
    LAUNCH_(PGF_FORM_EXTENDED);
  else
    LAUNCH_(PGF_FORM_ASYMMETRIC);
#undef LAUNCH_
}

// ---------------------------------------------------------------- step update
// From the full-length solution s (columns are in natural order in all three formulations):
// dx = s[:n]; dy = s[n:] (Standard) or fact (s[n:] - rho F_y) (Extended / Asymmetric);
// xn = clip(x - dx, lb, ub) with dx rewritten where clipped, yn = y - dy; per-block partial sums
// of dx^2 + dy^2 in fixed order -> red[blockIdx.x] (as k_step_update for the reduced system).
__global__ __launch_bounds__(256) void k_unsym_step_update(
    int n, int m, int scaled, double fact, double rho, const double *__restrict__ x,
    const double *__restrict__ y, const double *__restrict__ lb, const double *__restrict__ ub,
    const double *__restrict__ F, const double *__restrict__ sol, double *__restrict__ dx,
    double *__restrict__ dy, double *__restrict__ xn, double *__restrict__ yn, double *__restrict__ red) {
  __shared__ double part[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double sq = 0.0;
  if (i < n) {
    double d = sol[i];
    const double xi = x[i];
    double v = xi - d;
    const double lo = lb[i], hi = ub[i];
    if (v < lo) {
      v = lo;
      d = xi - lo;
    }
    if (v > hi) {
      v = hi;
      d = xi - hi;
    }
    dx[i] = d;
    xn[i] = v;
    sq = d * d;
  } else if (i < n + m) {
    const int r = i - n;
    double d = sol[i];
    if (scaled) {
      const double t = rho * F[i];
      d = fact * (d - t);
    }
    dy[r] = d;
    yn[r] = y[r] - d;
    sq = d * d;
  }
  sq = wave_sum(sq);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) red[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

void launch_unsym_step_update(hipStream_t s, int form, int n, int m, double fact, double rho,
                              const double *x, const double *y, const double *lb, const double *ub,
                              const double *F, const double *sol, double *dx, double *dy, double *xn,
                              double *yn, double *red) {
  const int nb = (n + m + 255) / 256;
  if (nb)
    hipLaunchKernelGGL(k_unsym_step_update, dim3(nb), dim3(256), 0, s, n, m,
                       form == PGF_FORM_STANDARD ? 0 : 1, fact, rho, x, y, lb, ub, F, sol, dx, dy, xn, yn,
                       red);
}
