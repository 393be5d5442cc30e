// Wavefront reductions and the fixed-order row dot product: the one copy for every translation unit
// that sums across lanes (the step, guard and batch kernels, the unsymmetric step, the line search).
// The order of the additions is part of the results -- two kernels that sum the same values this way
// give the same bits.
//
// Contraction rule: include only from files compiled with -ffp-contract=off (explicit fma() only,
// inside dot products).  build.py keeps those files in one group and tests/test_build_sources.py
// checks that every includer is in it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  return v;
}

// Fixed-order dot product of one matrix row with a vector by one wavefront.
__device__ __forceinline__ double row_dot(const double *__restrict__ row,
                                          const double *__restrict__ v, int cols, int lane) {
  double acc = 0.0;
  int j = lane * 2;
  if ((((uintptr_t)row) & 15) == 0) {
    for (; j + 1 < cols; j += 128) {
      const double2 a = *reinterpret_cast<const double2 *>(row + j);
      const double2 b = *reinterpret_cast<const double2 *>(v + j);
      acc = fma(a.x, b.x, acc);
      acc = fma(a.y, b.y, acc);
    }
    if (j < cols) acc = fma(row[j], v[j], acc);
  } else {
    for (j = lane; j < cols; j += 64) acc = fma(row[j], v[j], acc);
  }
  return wave_sum(acc);
}

// max that forwards a NaN operand as np.maximum does (fmax would drop it)
__device__ __forceinline__ double nan_max(double a, double b) {
  return (a != a || b != b) ? (a + b) : fmax(a, b);
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = nan_max(v, __shfl_down(v, off));
  return v;
}
