// Kernels and launchers of the dense batch: the batched twins of the step kernels (device bodies in
// pgf_step_dev.h), the sampled accuracy guard, the device-resident step controller and the condensed
// order.  Launch declarations: pgf_batch.h.  The vector kernels serve the banded batch too
// (pgf_api_band_batch.hip).  Compiled with -ffp-contract=off (the contraction rule: pgf_step_dev.h).
#include "pgf_batch.h"

#include <algorithm>

#include "pgf_head_dev.h"
#include "pgf_kernels.h"
#include "pgf_step_dev.h"

// ================================================================ batched kernels
// Same bodies as above, one instance per blockIdx.z, sizes read on the device (BInst in
// pgf_batch.h).  Nothing here needs a host round trip.
__global__ void kb_advance(const BInst *__restrict__ tab, int n, int m,
                           const uint8_t *__restrict__ accept) {
  const BInst &I = tab[blockIdx.z];
  const double lamb = I.ps[BPS_LAMB];
  const bool acc = accept[blockIdx.z] != 0;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    if (acc)
      I.xhat[i] = I.x[i];
    else
      I.x[i] = I.xhat[i];
    I.slb[i] = lamb * I.lb[i];
    I.sub[i] = lamb * I.ub[i];
  } else if (i < n + m) {
    if (acc)
      I.yhat[i - n] = I.y[i - n];
    else
      I.y[i - n] = I.yhat[i - n];
  }
  if (i == 0) {
    I.ctl[0] = 0;
    I.ctl[1] = 0;
    I.ctl[2] = 0;
    I.ctl[3] = 0;
  }
}

__global__ void kb_set_frozen(const BInst *__restrict__ tab, int B,
                              const uint8_t *__restrict__ frozen) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < B) tab[i].ctl[3] = frozen[i] ? 1 : 0;
}

// which 0: c = J x - b ; which 1: g = H x + tmpn
__global__ __launch_bounds__(256) void kb_gemv_rows(const BInst *__restrict__ tab, int which,
                                                    int n, int m) {
  const BInst &I = tab[blockIdx.z];
  if (which == 0)
    b_gemv_rows(m, n, I.J, I.ldj, I.x, I.b, -1.0, I.c);
  else
    b_gemv_rows(n, n, I.H, I.ldh, I.x, I.tmpn, 1.0, I.g);
}

__global__ void kb_mult_vec(const BInst *__restrict__ tab, int m) {
  const BInst &I = tab[blockIdx.z];
  b_mult_vec(m, I.ps[BPS_RHO], I.c, I.y, I.w);
}

__global__ __launch_bounds__(256) void kb_gemvT_partial(const BInst *__restrict__ tab, int n, int m,
                                                        int chunk) {
  const BInst &I = tab[blockIdx.z];
  b_gemvT_partial(m, n, I.J, I.ldj, I.w, chunk, I.partial);
}

__global__ void kb_sum_partials(const BInst *__restrict__ tab, int n, int used) {
  const BInst &I = tab[blockIdx.z];
  b_sum_partials(n, used, I.partial, I.q, I.tmpn);
}

// tau NaN = None; the factors of the tau form exactly as the host computes them for a single
// instance (implicit_func.py:237-244)
__global__ void kb_active_set(const BInst *__restrict__ tab, int n, double tau) {
  const BInst &I = tab[blockIdx.z];
  if (I.ctl[3]) return;
  const double lamb = I.ps[BPS_LAMB];
  const int use_tau = (tau != tau) ? 0 : 1;
  const double f_x = use_tau ? lamb * (1 - tau * lamb) : 0.0;
  const double f_x0 = use_tau ? tau * lamb * lamb : 0.0;
  const double f_d = use_tau ? tau * lamb : 0.0;
  b_active_set(n, use_tau, lamb, f_x, f_x0, f_d, I.xhat, I.x, I.g, I.slb, I.sub, I.mask_new);
}

// Adopt mask_new (mode 2: always; mode 1: when it differs elementwise from the current mask
// or there is none yet -- newton.py:203-215; mode 0: keep), rebuild the index lists when
// adopted, and decide whether this step factorises: ctl[0] = !factor_valid.
__global__ __launch_bounds__(1024) void kb_mask_adopt(const BInst *__restrict__ tab, int n,
                                                      int mode) {
  const BInst &I = tab[blockIdx.z];
  const int tid = threadIdx.x;
  if (I.ctl[3]) {  // frozen: nothing of this instance moves in this step
    if (tid == 0) I.ctl[0] = 0;
    return;
  }
  int diff = 0;
  if (mode == 2 || (mode == 1 && I.ctl[2] == 0)) {
    diff = 1;
  } else if (mode == 1) {
    for (int j = tid; j < n; j += 1024) diff |= (I.mask[j] != I.mask_new[j]) ? 1 : 0;
  }
  const int changed = __syncthreads_or(diff);
  if (changed) {
    for (int j = tid; j < n; j += 1024) I.mask[j] = I.mask_new[j];
    b_compact(n, I.mask_new, I.idxI, I.idxA, I.pos, I.counts);
  }
  if (tid == 0) {
    if (changed) {
      I.ctl[2] = 1;
      I.ctl[1] = 0;
    }
    I.ctl[0] = (changed || I.ctl[1] == 0) ? 1 : 0;
  }
}

__global__ void kb_residual(const BInst *__restrict__ tab, int n, int m) {
  const BInst &I = tab[blockIdx.z];
  if (I.ctl[3]) return;
  const double lamb = I.ps[BPS_LAMB], dt = I.ps[BPS_DT];
  b_residual(n, m, lamb, dt, I.xhat, I.yhat, I.x, I.y, I.g, I.c, I.slb, I.sub, I.mask, I.F,
             I.b0full, blockIdx.x * blockDim.x + threadIdx.x);
}

__global__ __launch_bounds__(256) void kb_active_rows_partial(const BInst *__restrict__ tab, int n,
                                                              int nparts) {
  const BInst &I = tab[blockIdx.z];
  if (I.ctl[3]) return;
  b_active_rows_partial(n, I.counts[1], I.idxA, I.H, I.ldh, I.b0full, nparts, I.partial);
}
__global__ __launch_bounds__(256) void kb_reduced_rhs(const BInst *__restrict__ tab, int n,
                                                      int m, int nparts) {
  const BInst &I = tab[blockIdx.z];
  if (I.ctl[3]) return;
  b_reduced_rhs(n, m, I.counts[0], I.counts[1], I.ps[BPS_FACT], I.F, I.idxI, I.J, I.ldj, I.b0full,
                I.partial, nparts, I.rhs);
}

// K (lower triangle) + the right-hand side in row N, only for instances that factorise
// (KB_ASM_ROWS rows per workgroup: with 8, a batch of 256 instances of N = 1280 is 206 000
// workgroups and the launch is bound by their dispatch)
#define KB_ASM_ROWS 32
__global__ __launch_bounds__(256) void kb_assemble(const BInst *__restrict__ tab, int m) {
  const BInst &I = tab[blockIdx.z];
  if (I.ctl[0] == 0) return;
  const double lamb = I.ps[BPS_LAMB], delta = I.ps[BPS_DELTA];
  const int nI = I.counts[0], N = nI + m;
  const int i0 = blockIdx.y * KB_ASM_ROWS;
  if (i0 > N) return;
  if (i0 == 0 && blockIdx.x == 0 && threadIdx.x < 4) I.flags[threadIdx.x] = 0;
  if (i0 <= N && N < i0 + KB_ASM_ROWS) {  // this row block also holds row N: the rhs
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < N) I.K[(int64_t)N * I.ldk + j] = I.rhs[j];
  }
  b_assemble_kkt<KB_ASM_ROWS>(blockIdx.x, blockIdx.y, threadIdx.x, I.K, I.ldk, I.H, I.ldh, I.J, I.ldj, I.idxI, nI, m, lamb, delta);
}

__global__ __launch_bounds__(256) void kb_step_update(const BInst *__restrict__ tab, int n,
                                                      int m, int move) {
  const BInst &I = tab[blockIdx.z];
  if (I.ctl[3]) return;
  b_step_update(n, m, I.counts[0], I.ps[BPS_FACT], I.ps[BPS_RHO], I.x, I.y, I.lb, I.ub, I.mask, I.pos, I.b0full, I.F,
                I.sol, I.dx, I.dy, I.xn, I.yn, I.red);
  // the new point replaces the current one in place (each lane re-reads its own entry) -- unless
  // the sampled residual of the solve failed: the host repairs such an instance from the point it
  // started at (batch_repair_instance, pgf_api_batch.hip).  move == 0 (a Globalized step, whose
  // table names the outer point): only the clipped direction is wanted, kb_ls_finish moves the point
  if (I.flags[3] || !move) return;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n)
    I.x[i] = I.xn[i];
  else if (i < n + m)
    I.y[i - n] = I.yn[i - n];
}

// Accuracy guard of the batched path.  The factor has overwritten the assembled matrix and a
// full residual would read H and J of every instance again (3 GB for 256 instances, 7 % of the
// step); element growth in an unpivoted LDL^T spoils the whole solution vector, so a SAMPLE of
// the rows of r = rhs - K s tells just as well: KB_NSAMPLE rows spread over the reduced system,
// K applied from H, J, the index list and the instance's lambda / delta, one wavefront per row.
// The measure is the normwise backward error of the single-instance guard (residual_rel,
// pgf_api.hip): max |r_sampled| > KB_RES_TOL (max |rhs| + ||K||_inf max |s|) sets flags[3], with
// ||K||_inf <= max(||H||_inf + lambda + ||J||_1, ||J||_inf + delta) and KB_RES_TOL its default
// refine_tol.  A tolerance of 1e-8 against max |rhs| passed solves spoilt by a pivot of 1e-9
// (forward error 1.2e-9); at one tight enough for those, max |rhs| alone would flag backward-
// stable solves of ill-conditioned systems (|r| ~ eps cond(K) |rhs|).  A flagged step is
// repaired on the instance's handle by pgf_batch_sync; under the device-resident controller it
// is reported as failed (kb_step_final), which the controller answers with a rejected step and
// a doubled lambda -- the reference's own recovery path (step_control.py:80-107) and what makes
// the matrix quasi-definite again.
#define KB_NSAMPLE 32
#define KB_RES_TOL 1e-11
__global__ __launch_bounds__(256) void kb_sample_residual(const BInst *__restrict__ tab, int m) {
  // grid (KB_NSAMPLE / 4, 1, B): one sampled row per wavefront (a row is a chain of dependent
  // gathers: 32 rows one after the other in one workgroup cost 0.1 ms per batched step)
  const BInst &I = tab[blockIdx.z];
  if (I.ctl[3]) return;
  __shared__ double bmax[4], smax[4];
  const int nI = I.counts[0], N = nI + m;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const double lamb = I.ps[BPS_LAMB], delta = I.ps[BPS_DELTA];
  double rb = 0.0, sb = 0.0;
  for (int j = tid; j < N; j += 256) {
    rb = fmax(rb, fabs(I.rhs[j]));
    sb = fmax(sb, fabs(I.sol[j]));
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    rb = fmax(rb, __shfl_down(rb, off));
    sb = fmax(sb, __shfl_down(sb, off));
  }
  if (lane == 0) {
    bmax[wave] = rb;
    smax[wave] = sb;
  }
  __syncthreads();
  const double b = fmax(fmax(bmax[0], bmax[1]), fmax(bmax[2], bmax[3]));
  const double sn = fmax(fmax(smax[0], smax[1]), fmax(smax[2], smax[3]));
  const double nK = fmax(I.ps[BPS_NORM_H] + lamb + I.ps[BPS_NORM_J1], I.ps[BPS_NORM_JINF] + delta);
  double den = b;
  if (sn <= 1.79e308) den += nK * sn;  // (a non-finite solution is measured against max |rhs|)
  const int ns = min(KB_NSAMPLE, N);
  const int k = blockIdx.x * 4 + wave;
  if (k >= ns) return;
  const int i = (int)(((long long)k * N) / ns);
  double acc = 0.0;
  if (i < nI) {
    const double *hrow = I.H + (int64_t)I.idxI[i] * I.ldh;
    for (int j = lane; j < nI; j += 64) acc = fma(hrow[I.idxI[j]], I.sol[j], acc);
    const double *jcol = I.J + I.idxI[i];
    for (int r = lane; r < m; r += 64) acc = fma(jcol[(int64_t)r * I.ldj], I.sol[nI + r], acc);
    if (lane == 0) acc = fma(lamb, I.sol[i], acc);
  } else {
    const double *jrow = I.J + (int64_t)(i - nI) * I.ldj;
    for (int j = lane; j < nI; j += 64) acc = fma(jrow[I.idxI[j]], I.sol[j], acc);
    if (lane == 0) acc = fma(-delta, I.sol[i], acc);
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    const double r = fabs(I.rhs[i] - acc);
    // (flags[3] was cleared by kb_solve_prep_bwd of this step; set only on failure: no
    // contention in the normal case)
    if (!(r <= KB_RES_TOL * (den > 0.0 ? den : 1.0))) atomicOr(&I.flags[3], 1);
  }
}

__global__ __launch_bounds__(256) void kb_step_final(const BInst *__restrict__ tab, int nb,
                                                     double *__restrict__ diff_out,
                                                     int *__restrict__ flags_out) {
  const BInst &I = tab[blockIdx.z];
  if (I.ctl[3]) {  // frozen: no step was taken
    if (threadIdx.x == 0) {
      diff_out[blockIdx.z] = 0.0;
      flags_out[3 * blockIdx.z] = 0;
      flags_out[3 * blockIdx.z + 1] = I.flags[1];
      flags_out[3 * blockIdx.z + 2] = I.counts[0];
    }
    return;
  }
  b_final_reduce(I.red, nb, diff_out + blockIdx.z, 1);
  if (threadIdx.x == 0) {
    // bit 0: zero / non-finite pivot; bit 1: the chain's helper workgroups failed a check
    // (a chained solve of the instance that failed its own checks counts like the helpers)
    // bit 2: the sampled residual of the solve is too large (kb_sample_residual)
    const int bad = (I.flags[0] ? 1 : 0) | ((I.flags[2] || I.cctl[1]) ? 2 : 0) | (I.flags[3] ? 4 : 0);
    I.cctl[1] = 0;
    // (sticky, behind the per-instance triples: a device-resident controller loop overwrites the
    // triples step after step; pgf_batch_ctl_read must still learn that a hand-over failed)
    if (bad & 2) atomicOr(flags_out + 3 * gridDim.z, 1);
    flags_out[3 * blockIdx.z] = bad;
    flags_out[3 * blockIdx.z + 1] = I.flags[1];
    flags_out[3 * blockIdx.z + 2] = I.counts[0];
    if (I.ctl[0]) I.ctl[1] = (bad == 0) ? 1 : 0;
  }
}

__global__ __launch_bounds__(256) void kb_unscaled_res_sq(const BInst *__restrict__ tab, int n,
                                                          int m) {
  const BInst &I = tab[blockIdx.z];
  b_unscaled_res_sq(n, m, I.ps[BPS_DT], I.xhat, I.yhat, I.x, I.y, I.g, I.c, I.lb, I.ub, I.red);
}

__global__ __launch_bounds__(256) void kb_norm_final(const BInst *__restrict__ tab, int nb,
                                                     double *__restrict__ norm_out) {
  const BInst &I = tab[blockIdx.z];
  b_final_reduce(I.red, nb, norm_out + blockIdx.z, 1);
}

static inline dim3 gb(int cnt, int per, int B) { return dim3((cnt + per - 1) / per, 1, B); }

// ---------------------------------------------------------------- device-resident step controller
// The reference's default DistanceRatioController (step/distance_ratio_control.py:12-78, PI law of
// controller.py:54-77) for every instance of a batch WITHOUT host round trips: three tiny kernels
// around the two batched Newton steps of an outer iteration keep lambda, the PI integral, the
// accept flag and the early exits on the device.  cs: DCS_STRIDE doubles per instance; cp: the
// controller's constants; log: 3 doubles per (iteration, instance).
__global__ void kb_dctl_begin(int B, const double *__restrict__ cs, const double *__restrict__ cp,
                              double *__restrict__ ps, uint8_t *__restrict__ accept) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  const double *c = cs + (size_t)DCS_STRIDE * i;
  // the host controller hands over dt = 1 / lambda and the library recomputes lambda = 1 / dt
  // (pgf_batch_advance_outer_each): same two roundings here
  const double dt = 1.0 / c[DCS_LAMB];
  const double lamb = 1.0 / dt, rho = cp[DCP_RHO];
  double *p = ps + (size_t)BPS_STRIDE * i;
  p[BPS_DT] = dt;
  p[BPS_LAMB] = lamb;
  p[BPS_RHO] = rho;
  p[BPS_FACT] = 1.0 / (1.0 + lamb * rho);
  p[BPS_DELTA] = lamb / (1.0 + lamb * rho);
  accept[i] = c[DCS_ACCEPTED] != 0.0 ? 1 : 0;
}

// after the first Newton step: failed factorisation -> reject, 2 lambda; converged residual ->
// accept, lambda * lamb_red; zero step -> accept; all three freeze the instance for step two
__global__ void kb_dctl_mid(const BInst *__restrict__ tab, int B, double *__restrict__ cs,
                            const double *__restrict__ cp, const double *__restrict__ diff,
                            const int *__restrict__ flags, const double *__restrict__ norm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  double *c = cs + (size_t)DCS_STRIDE * i;
  const double lamb = c[DCS_LAMB];
  c[DCS_USED] = lamb;
  double next = lamb, acc = 1.0, done = 1.0;
  if (flags[3 * i] != 0) {
    next = 2.0 * lamb;
    acc = 0.0;
  } else if (norm[i] <= cp[DCP_NEWTON_TOL]) {
    next = fmax(lamb * cp[DCP_LAMB_RED], cp[DCP_LAMB_MIN]);
  } else if (diff[i] == 0.0) {
    next = lamb;
  } else {
    done = 0.0;
  }
  c[DCS_NEXT] = next;
  c[DCS_ACCEPTED] = acc;
  c[DCS_DONE] = done;
  c[DCS_FIRST] = diff[i];
  tab[i].ctl[3] = done != 0.0 ? 1 : 0;
}

// after the second step: theta test + PI update on the log scale for the instances still in play
__global__ void kb_dctl_end(int B, double *__restrict__ cs, const double *__restrict__ cp,
                            const double *__restrict__ diff, const int *__restrict__ flags,
                            double *__restrict__ log3) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B) return;
  double *c = cs + (size_t)DCS_STRIDE * i;
  const double lamb = c[DCS_LAMB];
  double next = c[DCS_NEXT], acc = c[DCS_ACCEPTED];
  if (c[DCS_DONE] == 0.0) {
    const double second = diff[i];
    if (flags[3 * i] != 0) {
      next = 2.0 * lamb;
      acc = 0.0;
    } else if (second == 0.0) {
      next = lamb;
      acc = 1.0;
    } else {
      const double theta = second / c[DCS_FIRST];
      if (theta <= cp[DCP_THETA_MAX]) {
        const double e = cp[DCP_LOG_THETA_REF] - log(theta);
        const double integral = c[DCS_INTEGRAL] + e;
        c[DCS_INTEGRAL] = integral;
        const double u = cp[DCP_K_P] * e + cp[DCP_K_I] * integral;
        next = fmax(cp[DCP_LAMB_MIN], lamb / exp(u));
        acc = 1.0;
      } else {
        next = lamb * cp[DCP_LAMB_INC];
        acc = 0.0;
      }
    }
  }
  c[DCS_LAMB] = next;
  c[DCS_ACCEPTED] = acc;
  if (log3) {
    log3[3 * i] = lamb;
    log3[3 * i + 1] = next;
    log3[3 * i + 2] = acc;
  }
}

void batch_launch_dctl_begin(hipStream_t s, int B, const double *cs, const double *cp, double *ps,
                             uint8_t *accept) {
  hipLaunchKernelGGL(kb_dctl_begin, dim3((B + 255) / 256), dim3(256), 0, s, B, cs, cp, ps, accept);
}
void batch_launch_dctl_mid(hipStream_t s, const BInst *tab, int B, double *cs, const double *cp,
                           const double *diff, const int *flags, const double *norm) {
  hipLaunchKernelGGL(kb_dctl_mid, dim3((B + 255) / 256), dim3(256), 0, s, tab, B, cs, cp, diff, flags,
                     norm);
}
void batch_launch_dctl_end(hipStream_t s, int B, double *cs, const double *cp, const double *diff,
                           const int *flags, double *log3) {
  hipLaunchKernelGGL(kb_dctl_end, dim3((B + 255) / 256), dim3(256), 0, s, B, cs, cp, diff, flags, log3);
}

void batch_launch_advance(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc,
                          const uint8_t *accept) {
  hipLaunchKernelGGL(kb_advance, gb(std::max(1, sc.n + sc.m), 256, B), dim3(256), 0, s, tab, sc.n,
                     sc.m, accept);
}

void batch_launch_set_frozen(hipStream_t s, const BInst *tab, int B, const uint8_t *frozen) {
  hipLaunchKernelGGL(kb_set_frozen, dim3((B + 255) / 256), dim3(256), 0, s, tab, B, frozen);
}

// c = A x - b ; w = rho c + y ; tmpn = q + A' w ; g = Q x + tmpn   for every instance
void batch_launch_eval(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc, int nparts) {
  const int n = sc.n, m = sc.m;
  if (!n) return;
  int used = 0;
  if (m) {
    hipLaunchKernelGGL(kb_gemv_rows, gb(m, 4, B), dim3(256), 0, s, tab, 0, n, m);
    hipLaunchKernelGGL(kb_mult_vec, gb(m, 256, B), dim3(256), 0, s, tab, m);
    const int chunk = (m + nparts - 1) / nparts;
    used = (m + chunk - 1) / chunk;
    hipLaunchKernelGGL(kb_gemvT_partial, dim3((n + 255) / 256, used, B), dim3(256), 0, s, tab, n, m,
                       chunk);
  }
  hipLaunchKernelGGL(kb_sum_partials, gb(n, 256, B), dim3(256), 0, s, tab, n, used);
  hipLaunchKernelGGL(kb_gemv_rows, gb(n, 4, B), dim3(256), 0, s, tab, 1, n, m);
}

void batch_launch_mask(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc, int mode,
                       double tau) {
  if (mode != 0 && sc.n)
    hipLaunchKernelGGL(kb_active_set, gb(sc.n, 256, B), dim3(256), 0, s, tab, sc.n, tau);
  hipLaunchKernelGGL(kb_mask_adopt, dim3(1, 1, B), dim3(1024), 0, s, tab, sc.n, mode);
}

// ---- condensed order, batched (single-instance twins: k_cond_* in pgf_kernels.hip) -------
// V[i][r] = J[r][idxI[i]], zero beyond m; instances that factorise this step only
__global__ __launch_bounds__(256) void kb_cond_panel(const BInst *__restrict__ tab, int m, int mp) {
  const BInst &I = tab[blockIdx.z];
  if (I.ctl[0] == 0) return;
  const int nI = I.counts[0];
  const int i0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  if (i0 >= nI) return;
  __shared__ double tile[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int i = i0 + tx;
  const int col = i < nI ? I.idxI[i] : 0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int r = r0 + ty + 8 * p;
    tile[ty + 8 * p][tx] = (r < m && i < nI) ? I.J[(int64_t)r * I.ldj + col] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int ii = i0 + ty + 8 * p, r = r0 + tx;
    if (ii < nI && r < mp) I.V[(int64_t)ii * I.ldv + r] = tile[tx][ty + 8 * p];
  }
}
// row nI of V <- b_y, vd <- -1 / delta
__global__ void kb_cond_tail(const BInst *__restrict__ tab, int m, int mp) {
  const BInst &I = tab[blockIdx.z];
  if (I.ctl[0] == 0) return;
  const int nI = I.counts[0];
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= mp) return;
  I.V[(int64_t)nI * I.ldv + r] = (r < m) ? I.rhs[nI + r] : 0.0;
  I.vd[r] = -1.0 / I.ps[BPS_DELTA];
}
// zwork[i] = b_x[i] + dot(V[i][0:m], b_y) / delta: the forward solve's input when the factor is reused
__global__ __launch_bounds__(256) void kb_cond_prep_fwd(const BInst *__restrict__ tab, int m) {
  const BInst &I = tab[blockIdx.z];
  if (I.ctl[0] != 0 || I.ctl[3]) return;
  const int nI = I.counts[0];
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (i >= nI) return;
  const double d = row_dot(I.V + (int64_t)i * I.ldv, I.rhs + nI, m, lane);
  if (lane == 0) I.zwork[i] = I.rhs[i] + d / I.ps[BPS_DELTA];
}
// sol_y[r] = (sum_i V[i][r] sol_x[i] - b_y[r]) / delta: 64 columns per workgroup, sixteen lane
// groups take the rows i = g, g + 16, ... (four loads in flight each) and are summed in a fixed order
__global__ __launch_bounds__(1024) void kb_cond_y(const BInst *__restrict__ tab, int m) {
  const BInst &I = tab[blockIdx.z];
  if (I.ctl[3]) return;
  __shared__ double part[16][64];
  const int nI = I.counts[0];
  const int c = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int r = blockIdx.x * 64 + c;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  if (r < m) {
    const double *__restrict__ v = I.V + r;
    const double *__restrict__ x = I.sol;
    const int64_t ld = I.ldv;
    int i = g;
    for (; i + 48 < nI; i += 64) {
      s0 = fma(v[(int64_t)i * ld], x[i], s0);
      s1 = fma(v[(int64_t)(i + 16) * ld], x[i + 16], s1);
      s2 = fma(v[(int64_t)(i + 32) * ld], x[i + 32], s2);
      s3 = fma(v[(int64_t)(i + 48) * ld], x[i + 48], s3);
    }
    for (; i < nI; i += 16) s0 = fma(v[(int64_t)i * ld], x[i], s0);
  }
  part[g][c] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (g == 0 && r < m) {
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += part[k][c];
    I.sol[nI + r] = (s - I.rhs[nI + r]) / I.ps[BPS_DELTA];
  }
}

// F and b0full of every instance that is not frozen (the banded batch assembles its own system)
void batch_launch_residual(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc) {
  const int Nmax = sc.n + sc.m;
  if (Nmax) hipLaunchKernelGGL(kb_residual, gb(Nmax, 256, B), dim3(256), 0, s, tab, sc.n, sc.m);
}

void batch_launch_rhs_assemble(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc, int cond_mp) {
  const int n = sc.n, m = sc.m, Nmax = n + m;
  if (!Nmax) return;
  batch_launch_residual(s, tab, B, sc);
  // (the scratch `partial' holds 32 n doubles per instance: PGF_GEMVT_PARTS in pgf_api_internal.h)
  if (n) hipLaunchKernelGGL(kb_active_rows_partial, dim3((n + 255) / 256, 32, B), dim3(256), 0, s, tab, n, 32);
  hipLaunchKernelGGL(kb_reduced_rhs, gb(Nmax, 4, B), dim3(256), 0, s, tab, n, m, 32);
  if (cond_mp > 0) {
    // A and b_x (the assembly kernel with no constraint rows), V, b_y
    hipLaunchKernelGGL(kb_assemble, dim3((n + 255) / 256, n / KB_ASM_ROWS + 1, B), dim3(256), 0, s, tab, 0);
    hipLaunchKernelGGL(kb_cond_panel, dim3((n + 31) / 32, cond_mp / 32, B), dim3(256), 0, s, tab, m, cond_mp);
    hipLaunchKernelGGL(kb_cond_tail, gb(cond_mp, 256, B), dim3(256), 0, s, tab, m, cond_mp);
    return;
  }
  hipLaunchKernelGGL(kb_assemble, dim3((Nmax + 255) / 256, Nmax / KB_ASM_ROWS + 1, B), dim3(256), 0,
                     s, tab, m);
}
void batch_launch_cond_prep_fwd(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc) {
  if (sc.n) hipLaunchKernelGGL(kb_cond_prep_fwd, gb(sc.n, 4, B), dim3(256), 0, s, tab, sc.m);
}
void batch_launch_cond_y(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc) {
  if (sc.m) hipLaunchKernelGGL(kb_cond_y, dim3((sc.m + 63) / 64, 1, B), dim3(1024), 0, s, tab, sc.m);
}

void batch_launch_step_update(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc,
                              double *diff_out, int *flags_out, bool move) {
  const int nb = step_update_blocks(sc.n, sc.m);
  hipLaunchKernelGGL(kb_sample_residual, dim3(KB_NSAMPLE / 4, 1, B), dim3(256), 0, s, tab, sc.m);
  if (nb)
    hipLaunchKernelGGL(kb_step_update, dim3(nb, 1, B), dim3(256), 0, s, tab, sc.n, sc.m, move ? 1 : 0);
  hipLaunchKernelGGL(kb_step_final, dim3(1, 1, B), dim3(256), 0, s, tab, nb, diff_out, flags_out);
}

void batch_launch_res_norm(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc,
                           double *norm_out) {
  const int nb = (sc.n + sc.m + 255) / 256;
  if (nb)
    hipLaunchKernelGGL(kb_unscaled_res_sq, dim3(nb, 1, B), dim3(256), 0, s, tab, sc.n, sc.m);
  hipLaunchKernelGGL(kb_norm_final, dim3(1, 1, B), dim3(256), 0, s, tab, nb, norm_out);
}

// r = Q x + (q + A'y) into tmpn / g is NOT touched: the measures use their own vector (F is
// free between steps).  which 2: F[0:n] = H x + tmpn (after kb_sum_partials with w = y)
__global__ void kb_copy_y_to_w(const BInst *__restrict__ tab, int m) {
  const BInst &I = tab[blockIdx.z];
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) I.w[i] = I.y[i];
}

__global__ __launch_bounds__(256) void kb_gemv_stat(const BInst *__restrict__ tab, int n) {
  const BInst &I = tab[blockIdx.z];
  b_gemv_rows(n, n, I.H, I.ldh, I.x, I.tmpn, 1.0, I.F);
}

__global__ __launch_bounds__(256) void kb_measures(const BInst *__restrict__ tab, int n, int m,
                                                   double active_tol, double *__restrict__ red4,
                                                   int nb) {
  const BInst &I = tab[blockIdx.z];
  b_measures(n, m, active_tol, I.x, I.y, I.F, I.c, I.lb, I.ub, red4 + (size_t)blockIdx.z * 4 * nb);
}

__global__ __launch_bounds__(256) void kb_measures_final(const double *__restrict__ red4, int nb,
                                                         double *__restrict__ out) {
  b_measures_final(red4 + (size_t)blockIdx.z * 4 * nb, nb, out + 4 * blockIdx.z);
}

// c must be fresh (batch_launch_eval).  Leaves tmpn / w overwritten: the caller marks the
// evaluation stale.
void batch_launch_measures(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc,
                           int nparts, double active_tol, double *red4, double *out) {
  const int n = sc.n, m = sc.m;
  if (n) {
    int used = 0;
    if (m) {
      hipLaunchKernelGGL(kb_copy_y_to_w, gb(m, 256, B), dim3(256), 0, s, tab, m);
      const int chunk = (m + nparts - 1) / nparts;
      used = (m + chunk - 1) / chunk;
      hipLaunchKernelGGL(kb_gemvT_partial, dim3((n + 255) / 256, used, B), dim3(256), 0, s, tab, n,
                         m, chunk);
    }
    hipLaunchKernelGGL(kb_sum_partials, gb(n, 256, B), dim3(256), 0, s, tab, n, used);
    hipLaunchKernelGGL(kb_gemv_stat, gb(n, 4, B), dim3(256), 0, s, tab, n);
  }
  batch_launch_measures_final(s, tab, B, sc, active_tol, red4, out);
}

// the four measures of every instance from x, y, c and the stationarity residual in F[0:n]
void batch_launch_measures_final(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc,
                                 double active_tol, double *red4, double *out) {
  const int n = sc.n, m = sc.m;
  const int nb = (n + m + 255) / 256;
  if (nb)
    hipLaunchKernelGGL(kb_measures, dim3(nb, 1, B), dim3(256), 0, s, tab, n, m, active_tol, red4,
                       nb);
  hipLaunchKernelGGL(kb_measures_final, dim3(1, 1, B), dim3(256), 0, s, red4, nb, out);
}
