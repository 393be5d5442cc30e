// Large border: the bordered band of pgf_border.hip for 65 <= k <= 1024 border nodes.  The block
// elimination, the storage and the phases are the same; kp is k rounded up to 64, and what
// pgf_border.hip does for kp <= 64 with one workgroup or one wavefront is done here by kernels
// without a width limit:
//   factor:  B = kept factors of the wide reduction (block 16, 32, 64; the split is on),
//            Y = inv(B) C as ONE panel solve whose launches carry kp / 64 slices (pgf_band_wide.hip),
//            C' Y on v_mfma_f64_16x16x4_f64 (k_borderL_gram), S = D - C' Y into a dense L D L' of
//            size kp (pgf_ldlt.h), whose status is awaited here, once per assembled matrix
//   solve:   v = inv(B) ra, C' v by Dot2 per 64-column slice, z = inv(S) (rb - C' v) with the dense
//            factor's per-block triangular solves, xa = v - Y z: no host wait
//   guard:   r = rhs - K x over all Nb + k rows, the border rows with error-free sums
// The negative pivots of K are those of B plus those of S, the flags of B parked in bsflags[2, 4)
// as on the small route.  Compiled with -ffp-contract=off (explicit fma() only).
#include <algorithm>

#include "pgf_border_dev.h"
#include "pgf_ldlt.h"
#include "pgf_sparse.h"

typedef double bl_double4 __attribute__((ext_vector_type(4)));
typedef double bl_double2 __attribute__((ext_vector_type(2)));

#define BL_T 64        // tile of C' Y: 64 x 64, one workgroup of four wavefronts (2 x 2, 32 x 32 each)
#define BL_RS 16       // rows of C and Y staged per barrier pair
#define BL_LD 80       // LDS row stride in doubles: 64 + 16, so that the 2 x 16 doubles a lane group
                       // of ds_read_b64 reads (two consecutive rows) fall into different banks

// ---------------------------------------------------------------- G = C' Y
// Workgroup (tile, chunk): the 64 x 64 tile (ti, tj), tj <= ti, of the lower triangle of C' Y summed
// over the chunk's rows [chunk * rows, ...).  The reduction dimension is the row index, and both
// operands are row-major with the tile's 64 columns contiguous: a slab of four rows of C is the A
// operand of v_mfma_f64_16x16x4_f64 (lane l: A[l & 15][l >> 4] = C[row + (l >> 4)][a0 + (l & 15)])
// and the same four rows of Y the B operand (B[l >> 4][l & 15]) -- no transpose.  16 rows of both
// go through LDS per barrier pair, the next 16 already in registers.  Rows past the chunk's end
// are staged as zeros.  The tile leaves as a partial sum, part[(chunk * ntiles + tile)][64][64];
// k_borderL_schur adds the chunks in index order: deterministic, no same-address atomics.
__global__ __launch_bounds__(256) void k_borderL_gram(const double *__restrict__ C, const double *__restrict__ Y,
                                                      int Nb, int kp, int rows, double *__restrict__ part) {
  __shared__ double Cs[BL_RS * BL_LD], Ys[BL_RS * BL_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wr = wave >> 1, wc = wave & 1, l15 = lane & 15, l4 = lane >> 4;
  // tile index -> (ti, tj): tile = ti (ti + 1) / 2 + tj
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= (int)blockIdx.x) ++ti;
  const int tj = (int)blockIdx.x - ti * (ti + 1) / 2;
  const int a0 = ti * BL_T, b0 = tj * BL_T;
  const int i0 = (int)blockIdx.y * rows, i1 = min(Nb, i0 + rows);
  bl_double4 acc[2][2];
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 2; ++nj) acc[mi][nj] = (bl_double4){0.0, 0.0, 0.0, 0.0};
  // staging map: piece p = q * 256 + tid -> row p / 32, two doubles at column (p % 32) * 2
  bl_double2 pc[2], py[2];
  auto fetch = [&](int base) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int p = q * 256 + tid, r = base + p / 32, c = (p % 32) * 2;
      if (r < i1) {
        pc[q] = *reinterpret_cast<const bl_double2 *>(C + (int64_t)r * kp + a0 + c);
        py[q] = *reinterpret_cast<const bl_double2 *>(Y + (int64_t)r * kp + b0 + c);
      } else {
        pc[q] = (bl_double2){0.0, 0.0};
        py[q] = (bl_double2){0.0, 0.0};
      }
    }
  };
  fetch(i0);
  for (int base = i0; base < i1; base += BL_RS) {
    __syncthreads();  // the previous slab's fragment reads are done
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int p = q * 256 + tid;
      *reinterpret_cast<bl_double2 *>(&Cs[(p / 32) * BL_LD + (p % 32) * 2]) = pc[q];
      *reinterpret_cast<bl_double2 *>(&Ys[(p / 32) * BL_LD + (p % 32) * 2]) = py[q];
    }
    __syncthreads();
    if (base + BL_RS < i1) fetch(base + BL_RS);
#pragma unroll
    for (int ks = 0; ks < BL_RS; ks += 4) {
      double a[2], b[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        a[t] = Cs[(ks + l4) * BL_LD + wr * 32 + t * 16 + l15];
        b[t] = Ys[(ks + l4) * BL_LD + wc * 32 + t * 16 + l15];
      }
#pragma unroll
      for (int mi = 0; mi < 2; ++mi)
#pragma unroll
        for (int nj = 0; nj < 2; ++nj)
          acc[mi][nj] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[mi], b[nj], acc[mi][nj], 0, 0, 0);
    }
  }
  // C / D layout: row (l >> 4) + 4 reg, column l & 15
  double *out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (BL_T * BL_T);
#pragma unroll
  for (int mi = 0; mi < 2; ++mi)
#pragma unroll
    for (int nj = 0; nj < 2; ++nj)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[(wr * 32 + mi * 16 + l4 + 4 * r) * BL_T + wc * 32 + nj * 16 + l15] = acc[mi][nj][r];
}

// G[a][b] = sum over the chunks, in index order, of the partial tiles (a >= b; zero above the
// diagonal).  Kf != null: also S = D - G, both triangles, into the dense factor's K (row stride
// ldk); the padding of D is the identity and that of C' Y zero, so S carries the identity there.
__global__ __launch_bounds__(256) void k_borderL_schur(const double *__restrict__ part, int chunks, int kp,
                                                       const double *__restrict__ Dd, double *__restrict__ G,
                                                       double *__restrict__ Kf, int64_t ldk) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (int64_t)kp * kp) return;
  const int a = (int)(idx / kp), b = (int)(idx % kp);
  if (a < b) {
    G[idx] = 0.0;
    return;
  }
  const int nt = kp / BL_T, ntiles = nt * (nt + 1) / 2;
  const int ti = a / BL_T, tj = b / BL_T, tile = ti * (ti + 1) / 2 + tj;
  const double *p = part + (int64_t)tile * (BL_T * BL_T) + (a % BL_T) * BL_T + b % BL_T;
  double g = 0.0;
  for (int c = 0; c < chunks; ++c) g += p[(int64_t)c * ntiles * (BL_T * BL_T)];
  G[idx] = g;
  if (Kf) {
    const double sv = Dd[idx] - g;
    Kf[(int64_t)a * ldk + b] = sv;
    Kf[(int64_t)b * ldk + a] = sv;
  }
}

void sp_borderL_gram_plan(int Nb, int kp, int *rows, int *chunks) {
  const int nt = kp / BL_T, ntiles = nt * (nt + 1) / 2;
  // two workgroups per compute unit of a 256-CU device, no chunk below 64 rows, the partial sums
  // (32 KB per tile and chunk) below 256 MB
  const int want = std::max(1, 512 / ntiles);
  const int cap = std::max(1, (int)(((size_t)256 << 20) / ((size_t)ntiles * BL_T * BL_T * sizeof(double))));
  int r = (Nb + want - 1) / want;
  r = std::max(64, (r + BL_RS - 1) / BL_RS * BL_RS);
  int c = (Nb + r - 1) / r;
  if (c > cap) {
    r = ((Nb + cap - 1) / cap + BL_RS - 1) / BL_RS * BL_RS;
    c = (Nb + r - 1) / r;
  }
  *rows = r;
  *chunks = std::max(1, c);
}

// Device time of the Gram launch alone, the mean over reps launches between two events, on
// the C and Y of the handle's last factor phase (tools/time_border.py): the MFMA kernel into a
// scratch buffer of its own, and for kp <= 64 the small border's FMA kernel (k_border_gram) into
// sp.bor.bpart, which the factor phase has consumed.  kp must be a multiple of 64.
hipError_t sp_borderL_gram_time(hipStream_t s, const SparseDev &sp, int reps, double *ms_mfma, double *ms_fma) {
  const int Nb = sp.bor.Nb, kp = sp.bor.bkp, nt = kp / BL_T, ntiles = nt * (nt + 1) / 2;
  int rows, chunks;
  sp_borderL_gram_plan(Nb, kp, &rows, &chunks);
  double *part = nullptr;
  hipError_t e = hipMalloc((void **)&part, (size_t)chunks * ntiles * BL_T * BL_T * sizeof(double));
  if (e != hipSuccess) return e;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  float ms = 0.f;
  for (int variant = 0; variant < 2; ++variant) {
    if (variant == 1 && kp > 64) {
      *ms_fma = -1.0;
      break;
    }
    for (int it = -2; it < reps; ++it) {  // two warm-up launches
      if (it == 0) (void)hipEventRecord(e0, s);
      if (variant == 0)
        hipLaunchKernelGGL(k_borderL_gram, dim3(ntiles, chunks), dim3(256), 0, s, sp.bor.bC, sp.bor.bY, Nb, kp, rows, part);
      else
        sp_border_gram_fma(s, sp);
    }
    (void)hipEventRecord(e1, s);
    e = hipEventSynchronize(e1);
    if (e != hipSuccess) break;
    (void)hipEventElapsedTime(&ms, e0, e1);
    *(variant == 0 ? ms_mfma : ms_fma) = (double)ms / reps;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
  (void)hipFree(part);
  return e;
}

// ---------------------------------------------------------------- C' v, 64 columns per workgroup
// b_border_ctv (pgf_border_dev.h) on the column slice blockIdx.y of a chunk of SP_BORDER_CHUNK rows:
// the same Dot2 accumulation, the same (head, |C|' |v|, tail) triple per column and chunk.
__global__ __launch_bounds__(256) void k_borderL_ctv(const double *__restrict__ C, const double *__restrict__ v,
                                                     int Nb, int kp, double *__restrict__ partv) {
  __shared__ double red[256], redc[256], reda[256];
  const int t = threadIdx.x, j = t & 63, rg = t >> 6, col = (int)blockIdx.y * 64 + j;
  const int i0 = (int)blockIdx.x * SP_BORDER_CHUNK, i1 = min(Nb, i0 + SP_BORDER_CHUNK);
  double acc = 0.0, comp = 0.0, aa = 0.0;
  for (int i = i0 + rg; i < i1; i += 4) {
    const double cv = C[(int64_t)i * kp + col], x = v[i];
    const double p = cv * x, pe = fma(cv, x, -p);
    double e;
    two_sum(acc, p, acc, e);
    comp += e + pe;
    aa += fabs(p);
  }
  red[t] = acc;
  redc[t] = comp;
  reda[t] = aa;
  __syncthreads();
  if (t < 64) {
    double sv = 0.0, sc = 0.0, sa = 0.0;
    for (int g = 0; g < 4; ++g) {
      double e;
      two_sum(sv, red[g * 64 + t], sv, e);
      sc += e + redc[g * 64 + t];
      sa += reda[g * 64 + t];
    }
    partv[(int64_t)blockIdx.x * 3 * kp + col] = sv;
    partv[(int64_t)blockIdx.x * 3 * kp + kp + col] = sa;
    partv[(int64_t)blockIdx.x * 3 * kp + 2 * kp + col] = sc;
  }
}

// t = rb - sum of the chunks' C' v (head + tail, in chunk order), kp entries (padding: 0 - 0)
__global__ __launch_bounds__(256) void k_borderL_rhs(int kp, const double *__restrict__ rb,
                                                     const double *__restrict__ partv, int nchunk,
                                                     double *__restrict__ t) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= kp) return;
  double v = rb[j];
  for (int c = 0; c < nchunk; ++c) v -= partv[(int64_t)c * 3 * kp + j] + partv[(int64_t)c * 3 * kp + 2 * kp + j];
  t[j] = v;
}

// xa = v - Y z, 64 rows per workgroup: z in LDS, a wavefront per row with its lanes across the
// columns (coalesced reads of Y), the lanes' sums combined by a fixed butterfly.  Workgroup 0 also
// hands z to x[Nb, Nb + k) and merges the pivot flags of S into those of B (b_border_small_solve).
__global__ __launch_bounds__(256) void k_borderL_update(int Nb, int k, int kp, const double *__restrict__ Y,
                                                        const double *__restrict__ z, double *__restrict__ x,
                                                        const int *__restrict__ sflags,
                                                        int *__restrict__ flags) {
  __shared__ double zs[1024];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int j = t; j < kp; j += 256) zs[j] = (j < k) ? z[j] : 0.0;
  __syncthreads();
  const int r0 = (int)blockIdx.x * 64;
  for (int rr = wave; rr < 64; rr += 4) {
    const int i = r0 + rr;
    if (i >= Nb) break;  // (uniform over the wavefront)
    const double *row = Y + (int64_t)i * kp;
    double acc = 0.0;
    for (int j = lane; j < kp; j += 64) acc = fma(row[j], zs[j], acc);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) x[i] = x[i] - acc;
  }
  if (blockIdx.x == 0) {
    for (int j = t; j < k; j += 256) x[Nb + j] = zs[j];
    if (t == 0) {
      flags[0] |= sflags[0];
      flags[1] += sflags[1];
    }
  }
}

// ---------------------------------------------------------------- accuracy guard
// b_border_residual for any k: workgroup b < ceil(Nb / 256) takes 256 band rows (B x_a by the row's
// thread, C z by a wavefront per row), the next ceil(k / 256) workgroups the border rows, C' x_a
// from the chunk sums of k_borderL_ctv and D z with error-free products and sums; any further pair
// is zero.  The pairs and the flags behind them are those of b_border_residual.
__global__ __launch_bounds__(256) void k_borderL_residual(
    const double *__restrict__ band, int ldb, int bw, int Nb, int k, int kp, const double *__restrict__ C,
    const double *__restrict__ Dd, const double *__restrict__ partv, int nchunk,
    const double *__restrict__ x, const double *__restrict__ rhs0, double *__restrict__ r,
    double *__restrict__ rsmax, const int *__restrict__ flags, int nred) {
  if (blockIdx.x == 0 && threadIdx.x < 4) rsmax[3 * nred + threadIdx.x] = (double)flags[threadIdx.x];
  __shared__ double zs[1024];
  __shared__ double cz[256], caz[256];
  __shared__ double pr[4], pb[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  for (int j = t; j < kp; j += 256) zs[j] = (j < k) ? x[Nb + j] : 0.0;
  __syncthreads();
  const int nbB = (Nb + 255) / 256, nbK = (k + 255) / 256;
  double ar = 0.0, ab = 0.0;
  if ((int)blockIdx.x < nbB) {
    const int r0 = (int)blockIdx.x * 256;
    for (int rr = wave; rr < 256; rr += 4) {
      const int i = r0 + rr;
      if (i >= Nb) break;
      const double *row = C + (int64_t)i * kp;
      double s1 = 0.0, s2 = 0.0;
      for (int j = lane; j < kp; j += 64) {
        s1 = fma(row[j], zs[j], s1);
        s2 += fabs(row[j] * zs[j]);
      }
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_xor(s1, off);
        s2 += __shfl_xor(s2, off);
      }
      if (lane == 0) {
        cz[rr] = s1;
        caz[rr] = s2;
      }
    }
    __syncthreads();
    const int i = r0 + t;
    if (i < Nb) {
      double acc = rhs0[i];
      ab = fabs(acc);
      const double *row = band + (int64_t)i * ldb;
      for (int d = 0; d <= bw && d <= i; ++d) {
        acc = fma(-row[d], x[i - d], acc);
        ab += fabs(row[d] * x[i - d]);
      }
      for (int d = 1; d <= bw && i + d < Nb; ++d) {
        const double kv = band[(int64_t)(i + d) * ldb + d];
        acc = fma(-kv, x[i + d], acc);
        ab += fabs(kv * x[i + d]);
      }
      acc -= cz[t];
      ab += caz[t];
      r[i] = acc;
      ar = (acc == acc) ? fabs(acc) : __builtin_huge_val();
    }
  } else if ((int)blockIdx.x < nbB + nbK) {
    const int q = ((int)blockIdx.x - nbB) * 256 + t;
    if (q < k) {
      double acc = rhs0[Nb + q];
      ab = fabs(acc);
      // head + tail of rhs - C' x_a - D z, every sum and product error-free
      double comp = 0.0, e;
      for (int c = 0; c < nchunk; ++c) {
        two_sum(acc, -partv[(int64_t)c * 3 * kp + q], acc, e);
        comp += e - partv[(int64_t)c * 3 * kp + 2 * kp + q];
        ab += partv[(int64_t)c * 3 * kp + kp + q];
      }
      for (int l = 0; l < k; ++l) {
        const double dv = Dd[(int64_t)max(q, l) * kp + min(q, l)];
        const double p = dv * zs[l], pe = fma(dv, zs[l], -p);
        two_sum(acc, -p, acc, e);
        comp += e - pe;
        ab += fabs(p);
      }
      acc += comp;
      r[Nb + q] = acc;
      ar = (acc == acc) ? fabs(acc) : __builtin_huge_val();
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    ar = fmax(ar, __shfl_down(ar, off));
    ab = fmax(ab, __shfl_down(ab, off));
  }
  if ((t & 63) == 0) {
    pr[t >> 6] = ar;
    pb[t >> 6] = ab;
  }
  __syncthreads();
  if (t == 0) {
    rsmax[2 * blockIdx.x] = fmax(fmax(pr[0], pr[1]), fmax(pr[2], pr[3]));
    rsmax[2 * blockIdx.x + 1] = fmax(fmax(pb[0], pb[1]), fmax(pb[2], pb[3]));
  }
}

// the status of S, as the host read it from the dense factorisation, where the solve phase looks
// for it (bsflags[0] bad pivot, [1] negative pivots)
__global__ void k_borderL_sflags(int *__restrict__ sflags, int bad, int neg) {
  if (threadIdx.x == 0) {
    sflags[0] = bad;
    sflags[1] = neg;
  }
}

// ---------------------------------------------------------------- phases
void sp_borderL_factor(hipStream_t s, const SparseDev &sp, int *flags) {
  const int Nb = sp.bor.Nb, kp = sp.bor.bkp;
  DenseLdlt &f = *sp.bor.blf;
  sp_border_wide_Y(s, sp, flags);  // the factors of B, its flags parked, Y = inv(B) C
  const int nt = kp / BL_T, ntiles = nt * (nt + 1) / 2;
  hipLaunchKernelGGL(k_borderL_gram, dim3(ntiles, sp.bor.bgchunks), dim3(256), 0, s, sp.bor.bC, sp.bor.bY, Nb, kp, sp.bor.bgrows,
                     sp.bor.bpart);
  // S into the dense factor and its L D L'; the status is awaited here, once per assembled matrix
  // (a solve phase never waits).  Status 2 -- the diagonal chain's helper workgroups failed their
  // checks and are off now -- means nothing of that factor is to be trusted: S is formed again from
  // the partial sums, which are still there, and factorised without them.
  int st = -1;
  for (int attempt = 0; attempt < 2; ++attempt) {
    hipLaunchKernelGGL(k_borderL_schur, dim3((unsigned)(((int64_t)kp * kp + 255) / 256)), dim3(256), 0, s,
                       sp.bor.bpart, sp.bor.bgchunks, kp, sp.bor.bDd, sp.bor.bG, f.K, f.ldk);
    hipError_t e = ldlt_factor_async(f, kp, kp);
    st = e == hipSuccess ? ldlt_finish(f, &e) : -1;
    if (st != 2) break;
  }
  sp.bor.gram_ready = true;
  // Anything but a clean factor reaches the caller as a bad pivot at its next look at the flags --
  // intended also for a HIP error (st < 0) and for helpers that failed twice (st == 2), which
  // pgf_ls_create_dense reports as PGF_HIP_ERROR: this function has no return path of its own (the
  // four entry points are void and enqueue), the step is rejected either way, and a HIP error on the
  // stream comes back as such from the caller's own synchronisation right behind.
  hipLaunchKernelGGL(k_borderL_sflags, dim3(1), dim3(64), 0, s, sp.bor.bsflags, st == 0 ? 0 : 1, st == 0 ? f.n_neg : 0);
}

void sp_borderL_residual(hipStream_t s, const SparseDev &sp, const int *flags) {
  hipLaunchKernelGGL(k_borderL_ctv, dim3(sp.bor.bnchunk, sp.bor.bkp / 64), dim3(256), 0, s, sp.bor.bC, sp.vec.brhs, sp.bor.Nb, sp.bor.bkp,
                     sp.bor.bpartv);
  hipLaunchKernelGGL(k_borderL_residual, dim3(sp.vec.nred), dim3(256), 0, s, sp.pat.band, sp.pat.ldb, sp.pat.bw, sp.bor.Nb, sp.bor.bk,
                     sp.bor.bkp, sp.bor.bC, sp.bor.bDd, sp.bor.bpartv, sp.bor.bnchunk, sp.vec.brhs, sp.vec.brhs0, sp.vec.bres, sp.vec.bred, flags,
                     sp.vec.nred);
}

void sp_borderL_solve(hipStream_t s, const SparseDev &sp, int *flags, bool guard) {
  const int Nb = sp.bor.Nb, k = sp.bor.bk, kp = sp.bor.bkp;
  DenseLdlt &f = *sp.bor.blf;
  // (the band solve writes whole blocks: the border entries behind Nb do not survive it)
  (void)hipMemcpyAsync(sp.bor.brb, sp.vec.brhs + Nb, (size_t)k * sizeof(double), hipMemcpyDeviceToDevice, s);
  if (guard)
    (void)hipMemcpyAsync(sp.vec.brhs0, sp.vec.brhs, (size_t)(Nb + k) * sizeof(double), hipMemcpyDeviceToDevice, s);
  sp_border_wide_v(s, sp, flags);  // v = inv(B) ra against the kept factors; flags <- pivots of B as kept
  hipLaunchKernelGGL(k_borderL_ctv, dim3(sp.bor.bnchunk, kp / 64), dim3(256), 0, s, sp.bor.bC, sp.vec.brhs, Nb, kp, sp.bor.bpartv);
  hipLaunchKernelGGL(k_borderL_rhs, dim3((kp + 255) / 256), dim3(256), 0, s, kp, sp.bor.brb, sp.bor.bpartv, sp.bor.bnchunk,
                     sp.bor.bS);
  // (a factor that failed is reported through the flags; the solve then runs on whatever is there,
  // as the small route's does, and its result is discarded with the step)
  (void)ldlt_solve_async(f, sp.bor.bS, sp.bor.bz);
  hipLaunchKernelGGL(k_borderL_update, dim3((Nb + 63) / 64), dim3(256), 0, s, Nb, k, kp, sp.bor.bY, sp.bor.bz, sp.vec.brhs,
                     sp.bor.bsflags, flags);
  if (guard) sp_borderL_residual(s, sp, flags);
}
