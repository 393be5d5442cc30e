// The dense LU with partial pivoting (pgf_lu.hip).  gfx950 (MI355X / CDNA4) only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- dense LU with partial pivoting (pgf_lu.hip): P A = L U, row-major, in place ----------
struct DenseLu {
  int N = 0;
  int64_t ld = 0;
  double *A = nullptr;     // N x ld: unit-lower L below the diagonal, U on and above it
  int *piv = nullptr;      // row interchanged with row i at step i (LAPACK convention)
  int *perm = nullptr;     // the interchanges as one permutation: (P b)[i] = b[perm[i]]
  double *work = nullptr;  // N
  double *PT = nullptr;    // the current panel, column-major (32 x ldp): pivot search and rank-1
  int64_t ldp = 0;         // updates run along rows, coalesced
  int *flags = nullptr;    // [0] zero / non-finite pivot
  hipStream_t stream = nullptr;
  bool factored = false;
  int reg_panels = 0, streamed_panels = 0;  // of the last factorisation: k_lu_panel_reg / k_lu_panel
};
hipError_t lu_alloc(DenseLu &f, int N, hipStream_t stream);
void lu_free(DenseLu &f);
int lu_factor(DenseLu &f, hipError_t *err);  // 0 ok / 1 singular / -1 HIP error
hipError_t lu_solve_async(DenseLu &f, const double *rhs, double *sol, int trans);
