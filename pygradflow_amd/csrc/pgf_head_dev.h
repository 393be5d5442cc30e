// Device bodies of the K assembly and of the condensed system's panel, shared by their own
// kernels (pgf_kernels.hip) and by the head workers of the first chain's launch (k_chain_head,
// pgf_factor2.hip).  A body takes its (column block, row group, thread-in-group) indices as
// arguments: a unit is 256 lanes, a workgroup of their own or a quarter of a larger one.
// The entries are bit-exact with numpy expressions wherever they are written from, so the bodies
// switch contraction off themselves (pgf_factor2.hip is compiled with it on).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

// ---------------------------------------------------------------- K assembly (a10, a12)
// Lower triangle of K = [[H[I,I] + lamb I, .],[J[:,I], -delta I]] gathered from the
// device-resident H, J.  A unit covers ASM_ROWS rows x 256 columns (lanes run along
// columns: coalesced stores, loads coalesced whenever I is contiguous); the column's index
// in H / J is looked up once per lane.  One row per workgroup was dispatch-bound in the
// batched step (1.6 M workgroups).
// GRAM (the condensed system with the resident Gram matrix G = J^T J, pgf_api.hip): the H block
// becomes H[I,I] + G[I,I] * ginv (ginv = 1 / delta), gathered in the same pass with the same
// indices; the instantiations without it do not see the operand at all.
// cb: column block, rg: row group, t: lane of the unit (0 .. 255)
#define ASM_ROWS 8
template <int ROWS = ASM_ROWS, bool GRAM = false>
__device__ __forceinline__ void b_assemble_kkt(int cb, int rg, int t, double *__restrict__ K, int64_t ldk,
                                               const double *__restrict__ H, int64_t ldh,
                                               const double *__restrict__ J, int64_t ldj,
                                               const int *__restrict__ idxI, int nI, int m,
                                               double lamb, double delta,
                                               const double *__restrict__ G = nullptr, int64_t ldg = 0,
                                               double ginv = 0.0) {
#pragma clang fp contract(off)
  const int N = nI + m;
  const int i0 = rg * ROWS;
  const int j = cb * 256 + t;
  if (cb * 256 >= N || cb * 256 > i0 + ROWS - 1) return;  // (whole units only:
                                                             // every lane may be asked for its row index)
  const int gj = (j < nI) ? idxI[j] : 0;
  // The rows' indices in H come from ONE vector load (lane u holds row i0 + u's) and reach the
  // scalar unit through v_readlane: looked up row by row (`idxI[i]', a scalar load and its wait in
  // front of every row's global load) the rows ran one after the other -- 0.9 ms for a batch of
  // 256 x 1024^2, 2.4 TB/s.  Eight rows at a time: all loads of the group, then the stores.
  static_assert(ROWS <= 64, "one lane per row of the unit");
  const int lane = t & 63;
  const int rowidx = (lane < ROWS && i0 + lane < nI) ? idxI[i0 + lane] : 0;
  constexpr int GR = ROWS < 8 ? ROWS : 8;
#pragma unroll
  for (int r0 = 0; r0 < ROWS; r0 += GR) {
    double v[GR], vg[GR];
#pragma unroll
    for (int u = 0; u < GR; ++u) {
      const int i = i0 + r0 + u;
      const int gi = __builtin_amdgcn_readlane(rowidx, r0 + u);
      v[u] = 0.0;
      if (GRAM) vg[u] = 0.0;
      if (i < N && j <= i && j < N) {
        if (i < nI) {
          v[u] = H[(int64_t)gi * ldh + gj];
          // (only G's lower triangle is ever written: ldlt_gram_async)
          if (GRAM) vg[u] = G[(int64_t)max(gi, gj) * ldg + min(gi, gj)];
        } else if (j < nI) {
          v[u] = J[(int64_t)(i - nI) * ldj + gj];
        }
      }
    }
#pragma unroll
    for (int u = 0; u < GR; ++u) {
      const int i = i0 + r0 + u;
      if (i < N && j <= i && j < N) {
        double w = v[u];
        if (GRAM && i < nI) w += vg[u] * ginv;
        if (i == j) w = (i < nI) ? w + lamb : -delta;
        K[(int64_t)i * ldk + j] = w;
      }
    }
  }
}

// ---------------------------------------------------------------- condensed system: the panel
// V[i][r] = J[r][idxI[i]] (r < m), 0 for the padding columns: 32 x 32 tiles through LDS, reads
// run along i (contiguous whenever I is), writes along r
__device__ __forceinline__ void b_cond_tail(double *__restrict__ Vrow, double *__restrict__ vd, int r,
                                            int mp, int m, const double *__restrict__ rhs_y, double delta) {
  if (r >= mp) return;
  Vrow[r] = (rhs_y && r < m) ? rhs_y[r] : 0.0;
  vd[r] = -1.0 / delta;
}
// Tile (bx, by) in two halves with a barrier of the caller's between them; t: lane of the unit
// (0 .. 255).  (The units of the first row of tiles also write b_cond_tail's 32 entries of their
// columns.)
typedef double CondTile[32][33];
__device__ __forceinline__ void b_cond_panel_load(CondTile &tile, int bx, int by, int t, double *__restrict__ V,
                                                  int64_t ldv, int mp, const double *__restrict__ J, int64_t ldj,
                                                  const int *__restrict__ idxI, int nI, int m,
                                                  double *__restrict__ vd, const double *__restrict__ rhs_y,
                                                  double delta) {
  const int tx = t & 31, ty = t >> 5;
  const int i0 = bx * 32, r0 = by * 32;
  if (bx == 0 && ty == 0) b_cond_tail(V + (int64_t)nI * ldv, vd, r0 + tx, mp, m, rhs_y, delta);
  const int i = i0 + tx;
  const int col = i < nI ? idxI[i] : 0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int r = r0 + ty + 8 * p;
    tile[ty + 8 * p][tx] = (r < m && i < nI) ? J[(int64_t)r * ldj + col] : 0.0;
  }
}
__device__ __forceinline__ void b_cond_panel_store(const CondTile &tile, int bx, int by, int t,
                                                   double *__restrict__ V, int64_t ldv, int mp, int nI) {
  const int tx = t & 31, ty = t >> 5;
  const int i0 = bx * 32, r0 = by * 32;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int ii = i0 + ty + 8 * p, r = r0 + tx;
    if (ii < nI && r < mp) V[(int64_t)ii * ldv + r] = tile[tx][ty + 8 * p];
  }
}
