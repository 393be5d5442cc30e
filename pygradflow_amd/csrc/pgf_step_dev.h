// Device bodies of the Newton step's elementwise, compaction, right-hand-side, step-update and
// measure kernels.  pgf_kernels.hip wraps each in the kernel of a single handle, pgf_batch_kernels.hip
// in its batched twin (instance = blockIdx.z, pointers from the instance's BInst): the same function
// with the same arguments, so that both routes compute the same bits.
//
// Contraction rule: every includer is compiled with -ffp-contract=off.  The active-set mask must be
// bit-exact with the reference's numpy expressions, so no multiply-add may be fused here unless
// written as an explicit fma() (only inside dot products, whose summation order differs from
// scipy's anyway and is covered by the 1e-10 iterate tolerance).  build.py keeps the includers in
// one group; tests/test_build_sources.py checks it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pgf_reduce_dev.h"

#define ACTIVE_EPS 1e-8  // reference implicit_func.py:44

// ---------------------------------------------------------------- bounds (a2)
__device__ __forceinline__ void b_scale_bounds(int n, double lamb, const double *__restrict__ lb,
                               const double *__restrict__ ub, double *__restrict__ slb,
                               double *__restrict__ sub) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    slb[i] = lamb * lb[i];
    sub[i] = lamb * ub[i];
  }
}

// ---------------------------------------------------------------- p and mask (a3, a4)
// tau form: (f_x * x + f_x0 * x_hat) - f_d * g, evaluated left to right as numpy does
// (implicit_func.py:237-244); plain form: lamb * x_hat - g (:246).
__device__ __forceinline__ uint8_t active_flag(int i, int use_tau, double lamb, double f_x,
                                               double f_x0, double f_d,
                                               const double *__restrict__ xhat,
                                               const double *__restrict__ x,
                                               const double *__restrict__ g,
                                               const double *__restrict__ slb,
                                               const double *__restrict__ sub) {
  double p;
  if (use_tau) {
    const double a = f_x * x[i];
    const double b = f_x0 * xhat[i];
    const double c = f_d * g[i];
    p = (a + b) - c;
  } else {
    p = lamb * xhat[i] - g[i];
  }
  const double lo = slb[i] - ACTIVE_EPS;
  const double hi = sub[i] + ACTIVE_EPS;
  return (p < lo || p > hi) ? 1 : 0;
}
__device__ __forceinline__ void b_active_set(int n, int use_tau, double lamb, double f_x,
    double f_x0, double f_d,
                             const double *__restrict__ xhat, const double *__restrict__ x,
                             const double *__restrict__ g, const double *__restrict__ slb,
                             const double *__restrict__ sub, uint8_t *__restrict__ mask) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  mask[i] = active_flag(i, use_tau, lamb, f_x, f_x0, f_d, xhat, x, g, slb, sub);
}

// ---------------------------------------------------------------- compaction (k2)
// One workgroup of 1024 lanes walks the mask in chunks; wavefront ballots + a scan of the
// 16 wave totals give stable (ascending) index lists of the inactive and active sets.
// pos[j] = rank of j inside its own list.  counts[0, 1] <- |I|, |A|; counts[3] <- 1 when |I|
// differs from `expect' (the count a speculatively enqueued step runs with; -1: none).
// ActiveArgs::xhat != nullptr: the mask is evaluated here (b_active_set's predicate) and stored
// to `mask' on the way -- the active set, its copy and the compaction in one launch.
struct ActiveArgs {
  int use_tau;
  double lamb, f_x, f_x0, f_d;
  const double *xhat, *x, *g, *slb, *sub;
};
// FrontArgs (with ActiveArgs): the variable rows of k_residual_rhs on the way, for a step enqueued
// with |A| = 0 -- every lane has its entry's mask flag and rank in hand: F, b0full (b_residual's
// expressions) and rhs[rank] = F - 0.0 for the inactive entries (what the row idxI[rank] = j of
// k_residual_rhs computes; a step whose enqueued sizes turn out stale is discarded, as ever).
struct FrontArgs {
  double dt;
  double *F, *b0full, *rhs;
};
__device__ __forceinline__ double residual_x_m(int i, double lamb, const double *__restrict__ xhat,
                                              const double *__restrict__ x, const double *__restrict__ g,
                                              const double *__restrict__ slb, const double *__restrict__ sub,
                                              bool active);
__device__ __forceinline__ void b_compact(int n, const uint8_t *__restrict__ mask,
                                                  int *__restrict__ idxI, int *__restrict__ idxA,
                                                  int *__restrict__ pos, int *__restrict__ counts,
                                                  int expect = -1, const ActiveArgs *eval = nullptr,
                                                  uint8_t *__restrict__ mask_out = nullptr,
                                                  const FrontArgs *front = nullptr) {
  __shared__ int wtot[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int baseI = 0;
  for (int start = 0; start < n; start += 1024) {
    const int j = start + tid;
    const bool valid = j < n;
    bool inact;
    if (eval) {
      const uint8_t mk = valid ? active_flag(j, eval->use_tau, eval->lamb, eval->f_x, eval->f_x0,
                                             eval->f_d, eval->xhat, eval->x, eval->g, eval->slb,
                                             eval->sub)
                               : 1;
      if (valid) mask_out[j] = mk;
      inact = valid && mk == 0;
    } else {
      inact = valid && (mask[j] == 0);
    }
    const unsigned long long bal = __ballot(inact);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    int woff = 0, tot = 0;
    for (int w = 0; w < 16; ++w) {
      const int t = wtot[w];
      if (w < wave) woff += t;
      tot += t;
    }
    if (valid) {
      if (inact) {
        const int r = baseI + woff + before;
        idxI[r] = j;
        pos[j] = r;
      } else {
        const int r = j - (baseI + woff + before);  // active rank = j - #inactive before j
        idxA[r] = j;
        pos[j] = r;
      }
      if (front) {
        const double f = residual_x_m(j, eval->lamb, eval->xhat, eval->x, eval->g, eval->slb, eval->sub, !inact);
        front->F[j] = f;
        front->b0full[j] = !inact ? front->dt * f : 0.0;
        if (inact) front->rhs[baseI + woff + before] = f - 0.0;
      }
    }
    baseI += tot;
    __syncthreads();
  }
  if (tid == 0) {
    counts[0] = baseI;
    counts[1] = n - baseI;
    counts[3] = (expect >= 0 && baseI != expect) ? 1 : 0;
  }
}

// ---------------------------------------------------------------- residual (a5, a6)
// F = [lamb x - P(p) ; -(lamb y - (lamb y_hat + c))], P clips only masked entries
// (np.clip == min(max(p, lo), hi)).  Also emits b0full = mask ? dt * F_x : 0 (a8).
__device__ __forceinline__ double residual_x(int i, double lamb, const double *__restrict__ xhat,
                                            const double *__restrict__ x, const double *__restrict__ g,
                                            const double *__restrict__ slb, const double *__restrict__ sub,
                                            const uint8_t *__restrict__ mask) {
  return residual_x_m(i, lamb, xhat, x, g, slb, sub, mask[i] != 0);
}
__device__ __forceinline__ double residual_x_m(int i, double lamb, const double *__restrict__ xhat,
                                              const double *__restrict__ x, const double *__restrict__ g,
                                              const double *__restrict__ slb, const double *__restrict__ sub,
                                              bool active) {
  double p = lamb * xhat[i] - g[i];
  if (active) p = fmin(fmax(p, slb[i]), sub[i]);
  return lamb * x[i] - p;
}
__device__ __forceinline__ double residual_y(int r, double lamb, const double *__restrict__ yhat,
                                            const double *__restrict__ y, const double *__restrict__ c) {
  const double t = lamb * yhat[r] + c[r];
  return -(lamb * y[r] - t);
}
__device__ __forceinline__ void b_residual(int n, int m, double lamb, double dt,
    const double *__restrict__ xhat,
                           const double *__restrict__ yhat, const double *__restrict__ x,
                           const double *__restrict__ y, const double *__restrict__ g,
                           const double *__restrict__ c, const double *__restrict__ slb,
                           const double *__restrict__ sub, const uint8_t *__restrict__ mask,
                           double *__restrict__ F, double *__restrict__ b0full,
                           int i) {
  if (i < n) {
    const double f = residual_x(i, lamb, xhat, x, g, slb, sub, mask);
    F[i] = f;
    if (b0full) b0full[i] = mask[i] != 0 ? dt * f : 0.0;
  } else if (i < n + m) {
    F[i] = residual_y(i - n, lamb, yhat, y, c);
  }
}

// reduced right-hand side (a9 part, a11):
//   i <  nI : rhs[i] = F[I[i]]            - H[I[i], :] . b0full
//   i >= nI : rhs[i] = fact * F[n + r]    - J[r, :]    . b0full      (r = i - nI)
// b0full is zero on the inactive set, so the full-row dot equals the reference's
// H_lamb[I, A] b0 / J[:, A] b0 (symmetric_step_solver.py:87-91); skipped when |A| = 0.
// The H part reads the ACTIVE rows instead of the inactive ones (H is symmetric:
// H[I, A] b0 = (H[A, I])^T b0): |A| n instead of |I| n entries -- b_active_rows_partial leaves
// partial[p][j] = sum over the active rows a of chunk p of H[a][j] b0[a], fixed chunks, and the
// rows i < nI pick their column out of it.  (One row-dot per inactive row read 90 % of every
// instance's H in a batch with 10 % active variables: 53 us of a 1.3 ms batched step.)
__device__ __forceinline__ void b_active_rows_partial(int n, int nA, const int *__restrict__ idxA,
                                                      const double *__restrict__ H, int64_t ldh,
                                                      const double *__restrict__ b0full, int nparts,
                                                      double *__restrict__ partial) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n || nA <= 0) return;
  const int chunk = (nA + nparts - 1) / nparts;
  const int a0 = blockIdx.y * chunk, a1 = min(nA, a0 + chunk);
  double acc = 0.0;
  for (int a = a0; a < a1; ++a) {
    const int ga = idxA[a];
    acc = fma(H[(int64_t)ga * ldh + j], b0full[ga], acc);
  }
  partial[(int64_t)blockIdx.y * n + j] = acc;
}
__device__ __forceinline__ void b_reduced_rhs(int n, int m, int nI, int nA, double fact,
                                                     const double *__restrict__ F,
                                                     const int *__restrict__ idxI,
                                                     const double *__restrict__ J, int64_t ldj,
                                                     const double *__restrict__ b0full,
                                                     const double *__restrict__ partial, int nparts,
                                                     double *__restrict__ rhs) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nI + m) return;
  if (i < nI) {
    const int gi = idxI[i];
    double corr = 0.0;
    if (nA > 0) {  // lane p takes chunk p (nparts <= 64), summed over the wavefront in a fixed order
      corr = lane < nparts ? partial[(int64_t)lane * n + gi] : 0.0;
      corr = wave_sum(corr);
    }
    if (lane == 0) rhs[i] = F[gi] - corr;
    return;
  }
  const int r = i - nI;
  double corr = 0.0;
  if (nA > 0) corr = row_dot(J + (int64_t)r * ldj, b0full, n, lane);
  if (lane == 0) rhs[i] = fact * F[n + r] - corr;
}

// ---------------------------------------------------------------- K assembly (a10, a12)
// (b_assemble_kkt: pgf_head_dev.h)

__device__ __forceinline__ void b_copy(double *__restrict__ dst, const double *__restrict__ src,
    int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

__device__ __forceinline__ void b_copy_u8(uint8_t *__restrict__ dst,
    const uint8_t *__restrict__ src, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// count positions where two masks differ (ActiveSet policy, newton.py:210)
__device__ __forceinline__ void b_mask_diff(int n, const uint8_t *__restrict__ a,
    const uint8_t *__restrict__ b,
                            int *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const bool d = (i < n) && (a[i] != b[i]);
  const unsigned long long bal = __ballot(d);
  if ((threadIdx.x & 63) == 0 && bal) atomicAdd(out, __popcll(bal));
}

// ---------------------------------------------------------------- step update (a9, a15, a16)
// dx[I] = s[:nI], dx[A] = b0;  dy = fact * (s[nI:] - rho * b2)
// xn = clip(x - dx, lb, ub) with dx rewritten where clipped; yn = y - dy
// per-block partial sums of dx^2 + dy^2 in fixed order -> red[blockIdx.x]
__device__ __forceinline__ void b_step_update(
    int n, int m, int nI, double fact, double rho, const double *__restrict__ x,
    const double *__restrict__ y, const double *__restrict__ lb, const double *__restrict__ ub,
    const uint8_t *__restrict__ mask, const int *__restrict__ pos,
    const double *__restrict__ b0full, const double *__restrict__ F,
    const double *__restrict__ sol, double *__restrict__ dx, double *__restrict__ dy,
    double *__restrict__ xn, double *__restrict__ yn, double *__restrict__ red,
    bool own_sy = false, double sy = 0.0) {  // (own_sy: this row's sol[nI + r] is sy, formed by the caller)
  __shared__ double part[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double sq = 0.0;
  if (i < n) {
    double d = mask[i] ? b0full[i] : sol[pos[i]];
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
    const double t = rho * F[n + r];
    const double d = fact * ((own_sy ? sy : sol[nI + r]) - t);
    dy[r] = d;
    yn[r] = y[r] - d;
    sq = d * d;
  }
  sq = wave_sum(sq);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) red[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}

// out[0] = sqrt(sum red[0..cnt)) (or the plain sum when take_sqrt == 0), fixed order
__device__ __forceinline__ void b_final_reduce(const double *__restrict__ red, int cnt,
                                                      double *__restrict__ out, int take_sqrt) {
  __shared__ double part[4];
  double s = 0.0;
  for (int i = threadIdx.x; i < cnt; i += 256) s += red[i];
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    const double t = (part[0] + part[1]) + (part[2] + part[3]);
    out[0] = take_sqrt ? sqrt(t) : t;
  }
}

// The last workgroup to finish (atomic ticket) sums the per-block partials of red[0, nb) in
// b_final_reduce's fixed order, every workgroup's partial having been published by a release
// fence before its ticket; the ticket word is reset for the next launch.  Returns true in the
// workgroup that did it.
__device__ __forceinline__ bool last_block_reduce(const double *red, int nb, double *out,
                                                  unsigned *ticket) {
  __shared__ bool last;
  __syncthreads();  // (red[blockIdx.x] is stored by lane 0 after the block's own barrier)
  if (threadIdx.x == 0) {
    __threadfence();
    last = atomicAdd(ticket, 1u) == (unsigned)(nb - 1);
  }
  __syncthreads();
  if (!last) return false;
  __threadfence();
  b_final_reduce(red, nb, out, 1);
  if (threadIdx.x == 0) *ticket = 0u;
  return true;
}

// ---------------------------------------------------------------- linear-quadratic evaluation
// out[r] = M[r, :] . v + sgn * add[r]     (c = A x - b ;  g = Q x + (q + A'(rho c + y)))
__device__ __forceinline__ void b_gemv_rows(int rows, int cols,
                                                   const double *__restrict__ M, int64_t ld,
                                                   const double *__restrict__ v,
                                                   const double *__restrict__ add, double sgn,
                                                   double *__restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const double d = row_dot(M + (int64_t)r * ld, v, cols, lane);
  if (lane == 0) out[r] = d + sgn * add[r];
}

// partial[rb][j] = sum_{r in chunk rb} M[r][j] * w[r]   (transposed product, fixed order)
__device__ __forceinline__ void b_gemvT_partial(int rows, int cols,
                                                       const double *__restrict__ M, int64_t ld,
                                                       const double *__restrict__ w, int chunk,
                                                       double *__restrict__ partial) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= cols) return;
  const int r0 = blockIdx.y * chunk;
  const int r1 = min(rows, r0 + chunk);
  double acc = 0.0;
  for (int r = r0; r < r1; ++r) acc = fma(M[(int64_t)r * ld + j], w[r], acc);
  partial[(int64_t)blockIdx.y * cols + j] = acc;
}

// out[j] = base[j] + sum_rb partial[rb][j]
__device__ __forceinline__ void b_sum_partials(int cols, int nparts,
    const double *__restrict__ partial,
                               const double *__restrict__ base, double *__restrict__ out) {
  const int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= cols) return;
  double s = 0.0;
  for (int p = 0; p < nparts; ++p) s += partial[(int64_t)p * cols + j];
  out[j] = base[j] + s;
}

// w = rho * c + y
__device__ __forceinline__ void b_mult_vec(int m, double rho, const double *__restrict__ c,
                           const double *__restrict__ y, double *__restrict__ w) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) w[i] = rho * c[i] + y[i];
}

// squared entries of the UNSCALED residual with its own mask (ImplicitFunc.value_at,
// implicit_func.py:131-161): per-block partial sums -> red.  (The entry expressions and the block's
// sum on their own: k_tail_combine forms the same partials from the g it has just computed.)
__device__ __forceinline__ double unscaled_sq_x(double dt, double xhat, double x, double g, double lb,
                                                double ub) {
  double p = xhat - dt * g;
  const bool act = (p < lb - ACTIVE_EPS) || (p > ub + ACTIVE_EPS);
  if (act) p = fmin(fmax(p, lb), ub);
  const double f = x - p;
  return f * f;
}
__device__ __forceinline__ double unscaled_sq_y(double dt, double yhat, double y, double c) {
  const double f = y - (yhat + dt * c);
  return f * f;
}
__device__ __forceinline__ void block_sq_partial(double sq, double *__restrict__ red) {  // 256 lanes
  __shared__ double part[4];
  sq = wave_sum(sq);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sq;
  __syncthreads();
  if (threadIdx.x == 0) red[blockIdx.x] = (part[0] + part[1]) + (part[2] + part[3]);
}
__device__ __forceinline__ void b_unscaled_res_sq(
    int n, int m, double dt, const double *__restrict__ xhat, const double *__restrict__ yhat,
    const double *__restrict__ x, const double *__restrict__ y, const double *__restrict__ g,
    const double *__restrict__ c, const double *__restrict__ lb, const double *__restrict__ ub,
    double *__restrict__ red) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  double sq = 0.0;
  if (i < n) {
    sq = unscaled_sq_x(dt, xhat[i], x[i], g[i], lb[i], ub[i]);
  } else if (i < n + m) {
    const int r = i - n;
    sq = unscaled_sq_y(dt, yhat[r], y[r], c[r]);
  }
  block_sq_partial(sq, red);
}

// ---------------------------------------------------------------- termination measures
// Iterate-level residuals the outer loop tests between Newton calls (SURVEY.md 8f rank 4;
// reference iterate.py:136-181, active_set.py:4-29), per-block maxima of
//   [0] | r + d |   r = obj_grad + J'y (given), d = bounds_dual        -> stat_res
//   [1] | c |                                                         -> cons_violation
//   [2] max(lb - x, 0), max(x - ub, 0)                                -> bound_violation
//   [3] | y |                                                         -> DualNormUpdate
// written to red[4 * blockIdx.x + k].  np.maximum / np.linalg.norm(inf) propagate NaN;
// fmax does not, so a NaN entry is forwarded explicitly.
__device__ __forceinline__ void b_measures(int n, int m, double active_tol,
                                           const double *__restrict__ x,
                                           const double *__restrict__ y,
                                           const double *__restrict__ r,
                                           const double *__restrict__ c,
                                           const double *__restrict__ lb,
                                           const double *__restrict__ ub,
                                           double *__restrict__ red) {
  __shared__ double part[4][4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  double v0 = 0.0, v1 = 0.0, v2 = 0.0, v3 = 0.0;
  if (i < n) {
    const double xi = x[i], lo = lb[i], hi = ub[i], ri = r[i];
    const bool al = fabs(xi - lo) <= active_tol;
    const bool au = fabs(hi - xi) <= active_tol;
    const double nr = -ri;
    double d = 0.0;
    if (al && au)
      d = nr;
    else if (au)
      d = (nr != nr) ? nr : fmax(nr, 0.0);
    else if (al)
      d = (nr != nr) ? nr : fmin(nr, 0.0);
    v0 = fabs(ri + d);
    const double bl = lo - xi, bu = xi - hi;
    v2 = nan_max((bl != bl) ? bl : fmax(bl, 0.0), (bu != bu) ? bu : fmax(bu, 0.0));
  } else if (i < n + m) {
    v1 = fabs(c[i - n]);
    v3 = fabs(y[i - n]);
  }
  v0 = wave_max(v0);
  v1 = wave_max(v1);
  v2 = wave_max(v2);
  v3 = wave_max(v3);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[w][0] = v0;
    part[w][1] = v1;
    part[w][2] = v2;
    part[w][3] = v3;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    red[4 * blockIdx.x + k] =
        nan_max(nan_max(part[0][k], part[1][k]), nan_max(part[2][k], part[3][k]));
  }
}

// out[k] = max over blocks of red[4 b + k]
__device__ __forceinline__ void b_measures_final(const double *__restrict__ red, int nb,
                                                 double *__restrict__ out) {
  __shared__ double part[4][4];
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int b = threadIdx.x; b < nb; b += 256)
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = nan_max(v[k], red[4 * b + k]);
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = wave_max(v[k]);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0)
#pragma unroll
    for (int k = 0; k < 4; ++k) part[w][k] = v[k];
  __syncthreads();
  if (threadIdx.x < 4) {
    const int k = threadIdx.x;
    out[k] = nan_max(nan_max(part[0][k], part[1][k]), nan_max(part[2][k], part[3][k]));
  }
}
