// Launch wrappers of pgf_unsym.hip: the Standard / Extended / Asymmetric formulations on the
// device (all asynchronous on the given stream).  form: PGF_FORM_STANDARD / _EXTENDED / _ASYMMETRIC.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// M ((n + m) x ld, row-major) <- the formulation's Newton matrix, every entry written once (the
// padding columns too).  Only the lower triangles of H and G are read; G != nullptr adds rhoG * G
// to H (device-resident Standard).  counts[1] = |A| is read on the device (Extended).
void launch_assemble_unsym(hipStream_t s, int form, double *M, int64_t ld, int n, int m, const double *H,
                           int64_t ldh, const double *J, int64_t ldj, const double *G, int64_t ldg,
                           double rhoG, const uint8_t *mask, const int *idxI, const int *idxA,
                           const int *counts, double dt, double lamb, double delta);
// Standard's mask from the UNSCALED projection; f_x = 1 - tau lamb, f_x0 = tau lamb
void launch_unscaled_active_set(hipStream_t s, int n, int use_tau, double dt, double f_x, double f_x0,
                                double tau, const double *xhat, const double *x, const double *g,
                                const double *lb, const double *ub, uint8_t *mask);
// F <- the formulation's residual (natural order), rhs (may be null) <- the same in the
// formulation's row order.  lo, hi: the bounds the projection clips to (Standard: lb, ub; else the
// scaled ones).
void launch_unsym_residual_rhs(hipStream_t s, int form, int n, int m, double lamb, double dt, double fact,
                               const double *xhat, const double *yhat, const double *x, const double *y,
                               const double *g, const double *c, const double *lo, const double *hi,
                               const uint8_t *mask, const int *pos, const int *counts, double *F,
                               double *rhs);
// dx, dy, xn, yn from the full-length solution; red[0, (n + m + 255) / 256) <- partial sums of
// the squared step
void launch_unsym_step_update(hipStream_t s, int form, int n, int m, double fact, double rho,
                              const double *x, const double *y, const double *lb, const double *ub,
                              const double *F, const double *sol, double *dx, double *dy, double *xn,
                              double *yn, double *red);
