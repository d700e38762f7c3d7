// Samples from N(mean, J^-1) off a stored factor: x = mean + H^T eps, H = L^-1 T the forward half of the solve
// (halfsolve), so that J^-1 = H^T H and H^T = backhalfsolve.  eps is standard-normal noise in CRR layout, DEFINED as
// the array cgps_normal_fill(rows = N d, cols = nrhs, seed, stream) would write (cgps_rng.h) -- and never written:
// this is the backward sweep of cgps_solve_tile_m.h (same Panel, PassLevels, Chol, load_block and tile sizes) in which
// the lane that eliminates CRR block c makes its d x (its columns) panel of eps in registers where
// backsolve_tile_m_kernel loads the right-hand side.  The vector ALUs idle in that latency-bound sweep; the noise
// costs no memory traffic at all.
//
// All column chunks of a pass run in one launch: blockIdx.y is the chunk (columns [col0 + y MC, ... + MC)), each with
// its own slice of the coarse-solution buffers (sample_ws in cgps_plan.h).  The pass that produces level 0 adds the
// mean in its store to the caller's x [n][d][nrhs].
#pragma once
#include "cgps_rng.h"
#include "cgps_solve_tile_m.h"

namespace cgps {

// the panel of eps of CRR block row `crr`, columns [col, col + MS) (col a multiple of MS); columns >= ncols: zero
template <typename T, int D, int MS, int MC>
__device__ __forceinline__ void noise_panel(Panel<T, D, MS, MC>& r, uint64_t seed, uint32_t stream, int64_t crr, int64_t col,
                                            int64_t ncols) {
  constexpr int GC = RngGroup<T>::COLS;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    const uint64_t re = (uint64_t)crr * D + i;
    if constexpr (MS >= GC) {
#pragma unroll
      for (int q = 0; q < MS / GC; ++q) {
        T z[GC];
#pragma unroll
        for (int u = 0; u < GC; ++u) z[u] = T(0);
        if (col + q * GC < ncols) normal_group(seed, stream, re, (uint32_t)((col + q * GC) / GC), z);
#pragma unroll
        for (int u = 0; u < GC; ++u) r.v[i][q * GC + u] = z[u];
      }
    } else {                                               // fp32, two-column panel: half a group
      static_assert(MS == 2 && GC == 4, "sub-panels are 2 or 4 columns wide");
      float z[2] = {0.0f, 0.0f};
      if (col < ncols) normal_half_group(seed, stream, re, (uint64_t)col, z);
      r.v[i][0] = z[0];
      r.v[i][1] = z[1];
    }
  }
}

// x_coarse / x_out: chunk y's data starts coarse_stride / out_stride elements after chunk y - 1's.  Workspace passes:
// x_out [n][D][MC] dense (ld_o = MC, mean = nullptr); the last pass: x_out = x + col0, out_stride = MC, ld_o = ncols.
template <typename T, int D, int MC>
__global__ __launch_bounds__((1 << solve_m_tile_log2<MC>()) / 2 * solve_m_col_splits<MC>()) void sample_tile_m_kernel(
    const T* __restrict__ Dp, const T* __restrict__ Fp, const T* __restrict__ Gp, PassLevels lv, uint64_t seed, uint32_t stream,
    int64_t col0, int64_t ncols, const T* __restrict__ x_coarse, size_t coarse_stride, int64_t n, T* __restrict__ x_out,
    size_t out_stride, int64_t ld_o, const T* __restrict__ mean) {
  constexpr int DD = D * D, TS = 1 << solve_m_tile_log2<MC>(), NT = TS / 2, PW = D * MC;
  constexpr int CS = solve_m_col_splits<MC>(), MS = MC / CS;
  using P = Panel<T, D, MS, MC>;
  extern __shared__ __attribute__((aligned(16))) char solve_smem[];
  T* xs = reinterpret_cast<T*>(solve_smem);                                   // [TS][D][MC]
  const int tid = threadIdx.x % NT, c0 = (threadIdx.x / NT) * MS;
  const int64_t row0 = (int64_t)blockIdx.x * TS;
  const int n0 = (int)((n - row0) < TS ? (n - row0) : TS);
  const int64_t col = col0 + (int64_t)blockIdx.y * MC + c0;                   // this lane's first column of x
  xs += c0;
  P xleft;                                               // x of the previous tile's last row
  xleft.zero();
  if (x_coarse != nullptr) {                             // solution of the rows that survived this pass's levels
    const T* xc = x_coarse + (size_t)blockIdx.y * coarse_stride;
    const int spt = TS >> lv.nlev;
    if (blockIdx.x > 0) xleft.load_dense(xc + ((size_t)blockIdx.x * spt - 1) * PW + c0);
    for (int r = tid; r < (n0 >> lv.nlev); r += NT) {
      P v;
      v.load_dense(xc + ((size_t)blockIdx.x * spt + r) * PW + c0);
      v.lds_store(xs + (size_t)(((r + 1) << lv.nlev) - 1) * PW);
    }
  }
  __syncthreads();
#pragma unroll 1
  for (int j = lv.nlev - 1; j >= 0; --j) {
    const int nj = n0 >> j;
    if (nj >= 1) {
      const int ne = (nj + 1) >> 1;
      const int64_t g0 = row0 >> (j + 1);
#pragma unroll 1
      for (int k = tid; k < ne; k += NT) {
        T M[D][D];
        P r, xo;
        noise_panel<T, D, MS, MC>(r, seed, stream, lv.offD[j] + g0 + k, col, ncols);
        if (2 * k + 1 < nj) {
          load_block<T, D>(Fp + (lv.offF[j] + g0 + k) * DD, M);
          xo.lds_load(xs + (size_t)(((2 * k + 2) << j) - 1) * PW);
          r.gemmT_sub(M, xo);
        }
        if (k >= 1) {
          load_block<T, D>(Gp + (lv.offG[j] + g0 + k - 1) * DD, M);
          xo.lds_load(xs + (size_t)(((2 * k) << j) - 1) * PW);
          r.gemmT_sub(M, xo);
        } else if (g0 >= 1) {                            // left neighbour = previous tile's last row
          load_block<T, D>(Gp + (lv.offG[j] + g0 - 1) * DD, M);
          r.gemmT_sub(M, xleft);
        }
        T L[D][D];
        Chol<T, D> c;
        load_block<T, D>(Dp + (lv.offD[j] + g0 + k) * DD, L);
        chol_from_dense<T, D>(L, c);
        r.bwd(c);
        r.lds_store(xs + (size_t)(((2 * k + 1) << j) - 1) * PW);
      }
    }
    __syncthreads();
  }
  T* xo_base = x_out + (size_t)blockIdx.y * out_stride;
  const int64_t wcols = ncols - col;                     // this lane's real columns (<= 0: none)
  for (int r = tid; r < n0; r += NT) {
    P v;
    v.lds_load(xs + (size_t)r * PW);
    if (mean == nullptr && ld_o == MC) {
      v.store_dense(xo_base + (size_t)(row0 + r) * PW + c0);
    } else {
      T* p = xo_base + (size_t)(row0 + r) * D * ld_o + c0;
#pragma unroll
      for (int i = 0; i < D; ++i) {
        const T mu = mean != nullptr ? mean[(size_t)(row0 + r) * D + i] : T(0);
#pragma unroll
        for (int c = 0; c < MS; ++c)
          if (c < wcols) p[(size_t)i * ld_o + c] = v.v[i][c] + mu;
      }
    }
  }
}

}  // namespace cgps
