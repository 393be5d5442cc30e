// The dense batch: the per-instance table (BInst), the step scalars, the device-resident step
// controller's state and the launchers of pgf_batch_kernels.hip.  gfx950 (MI355X / CDNA4) only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- batched mode ----------------------------------------------------------
// One entry per instance of a batch (all instances share n, m): the device addresses of an
// ordinary solver handle.  Batched kernels pick their instance with blockIdx.z and read the
// instance's own reduced size N = counts[0] + m on the device, so a whole batched Newton
// step is enqueued without a host round trip.  ctl: [0] factor this step, [1] factor
// valid, [2] mask valid, [3] frozen (the instance sits this Newton step out).
// ps: the instance's own outer-step scalars [dt, lambda, rho, fact, delta] -- every instance
// has its own step-size controller.
struct BInst {
  const double *H, *J;
  int64_t ldh, ldj;
  const double *lb, *ub, *q, *b;
  double *slb, *sub, *xhat, *yhat, *x, *y, *xn, *yn, *g, *c, *F, *b0full, *rhs, *sol, *dx, *dy;
  double *w, *tmpn, *partial, *red;
  uint8_t *mask, *mask_new;
  int *idxI, *idxA, *pos, *counts, *ctl;
  const double *ps;
  double *K;
  int64_t ldk;
  double *W;
  int64_t wstride;
  double *dvec, *dinv, *zwork, *Linv, *LinvT;
  int *flags;
  int *hctl;  // stamps between the instance's chain and its helper workgroups (small batches)
  // chained triangular solves: both publication halves (capblk * 64 entries each) and the
  // control words [0] XCC slot, [1] status, [2] solve counter of the instance's handle
  double *xpub;
  int *cctl;
  int capblk;
  // condensed order (pgf_api_batch.hip, pgf_batch_s::cond): the instance's panel V = J_I^T
  // ((n + 1) x ldv, row nI = the constraint part of the right-hand side) and its scaling -1 / delta
  double *V;
  int64_t ldv;
  double *vd;
};

struct BatchScalars {
  int n, m;
};
#define BPS_DT 0
#define BPS_LAMB 1
#define BPS_RHO 2
#define BPS_FACT 3
#define BPS_DELTA 4
// ||H||_inf, ||J||_1, ||J||_inf of the instance (residual_norms): the normwise measure of
// kb_sample_residual bounds ||K||_inf with them and the current lambda, delta
#define BPS_NORM_H 5
#define BPS_NORM_J1 6
#define BPS_NORM_JINF 7
#define BPS_STRIDE 8
// ctl: BCTL_STRIDE ints per instance (the words above).  flags_out of the step update and its pinned
// mirror: BFL_STRIDE ints per instance; on the device one sticky word behind the last instance's
// (a chain helper or a chained solve failed its hand-over in some step since it was cleared)
#define BCTL_STRIDE 4
#define BFL_BAD 0  // bit 0 zero pivot, bit 1 failed hand-over, bit 2 sampled residual too large
#define BFL_NEG 1  // negative pivots
#define BFL_NI 2   // |I|
#define BFL_STRIDE 3

// device-resident step controller: per-instance state (cs) and constants (cp)
#define DCS_LAMB 0      // lambda of the next outer iteration
#define DCS_INTEGRAL 1  // integral of the PI law (log scale)
#define DCS_FIRST 2     // step length of the first Newton step
#define DCS_ACCEPTED 3  // 1: the last outer step was accepted
#define DCS_DONE 4      // 1: decided after the first Newton step
#define DCS_NEXT 5      // lambda decided so far
#define DCS_USED 6      // lambda the current iteration ran with
#define DCS_STRIDE 8
#define DCP_RHO 0
#define DCP_NEWTON_TOL 1
#define DCP_LAMB_RED 2
#define DCP_LAMB_MIN 3
#define DCP_LAMB_INC 4
#define DCP_THETA_MAX 5
#define DCP_K_P 6
#define DCP_K_I 7
#define DCP_LOG_THETA_REF 8
#define DCP_COUNT 16

// ---- launchers (pgf_batch_kernels.hip) --------------------------------------
void batch_launch_dctl_begin(hipStream_t s, int B, const double *cs, const double *cp, double *ps,
                             uint8_t *accept);
void batch_launch_dctl_mid(hipStream_t s, const BInst *tab, int B, double *cs, const double *cp,
                           const double *diff, const int *flags, const double *norm);
void batch_launch_dctl_end(hipStream_t s, int B, double *cs, const double *cp, const double *diff,
                           const int *flags, double *log3);
// accept[i] != 0: (x^, y^) <- (x, y); == 0: (x, y) <- (x^, y^) (a rejected step goes back)
void batch_launch_advance(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc,
                          const uint8_t *accept);
void batch_launch_set_frozen(hipStream_t s, const BInst *tab, int B, const uint8_t *frozen);
void batch_launch_eval(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc, int nparts);
// mode 1: adopt mask_new where it differs (or no mask yet); 2: always adopt; 0: keep
void batch_launch_mask(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc, int mode,
                       double tau);
// cond_mp > 0: the condensed order -- only A = H[I,I] + lamb I is assembled (+ b_x in row nI), the
// constraint block goes into the instances' panels V (cond_mp columns, zero-padded)
void batch_launch_rhs_assemble(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc,
                               int cond_mp = 0);
// condensed order: zwork <- b_x + V b_y / delta before a forward solve (instances that reuse their
// factor), sol_y <- (V^T sol_x - b_y) / delta after the backward solve (all instances)
void batch_launch_residual(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc);
void batch_launch_cond_prep_fwd(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc);
void batch_launch_cond_y(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc);
// flags_out: [3 i] zero-pivot flag, [3 i + 1] negative pivots, [3 i + 2] |I| of instance i
// move == false: (xn, yn), dx, dy and the length only; the current point stays (a Globalized step on
// the table that names the outer point: the line search's finish moves the point)
void batch_launch_step_update(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc,
                              double *diff_out, int *flags_out, bool move = true);
void batch_launch_res_norm(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc,
                           double *norm_out);
void batch_launch_measures(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc,
                           int nparts, double active_tol, double *red4, double *out);
void batch_launch_measures_final(hipStream_t s, const BInst *tab, int B, const BatchScalars &sc,
                                 double active_tol, double *red4, double *out);
