// Perturb and solve: the right-hand sides  v + w,  w ~ N(0, K),  of the draws  x = K^-1 (v + w)  from
// the posterior N(K^-1 v, K^-1) of B concatenated LEG series (K = cgps_leg_posterior_blocks_seg's system), all rows,
// all series and all columns in one launch.  K is a sum of local positive semi-definite pieces -- the stationary
// start of a series, one Markov transition per time gap, one observation per row -- so w is a sum of local pieces of
// noise.  With E_r = exp(-1/2 (t_{r+1} - t_r) G), Q_r = I - E_r E_r^T = L_r L_r^T and u_r = L_r^-T eps_{r+1}:
//     w_r = (r == 0 ? eps_0 : u_{r-1}) - (r + 1 < n ? E_r^T u_r : 0) + H_r eps'_r
// (gap r contributes (-E_r^T u_r, u_r) to rows (r, r + 1): covariance [[E^T Q^-1 E, -E^T Q^-1], [-Q^-1 E, Q^-1]], the
// gap's share of the PEG precision since b = Q^-1 E and I + E a = Q^-1; H_r H_r^T = B^T Li_r B is the row's term).
// eps_r[i] is element (id 2^40 + r d + i, column s) of the generator of cgps_rng.h under the caller's stream word,
// eps'_r[c] element (id 2^40 + r obs + c, s) under stream + 1; r is the row's index INSIDE its series and id the
// series' caller-visible number, so a row's w is bitwise independent of where the series sits in the batch, of what
// else is in the batch and of nrhs.
//
// One lane per row of the concatenated batch (peg_precision_kernel's layout): it finds its series by binary search in
// row_offsets (leg_intercast_seg_kernel's search), evaluates its own gap and the gap before it through gap_expm1 /
// gap_gram<OUTER> / chol_lower -- Q is never formed from two matrices of size 1 -- and regenerates the noise of both
// neighbouring rows from the counter: two lanes make the u of a shared gap, each for itself, and nothing is
// communicated.  A gap is never evaluated across a series boundary.  The noise lives in registers only.
//
// Columns: blockIdx.y names a chunk of PERT_CHUNK_GROUPS generator groups (32 fp64 / 64 fp32 columns); the lanes of a
// chunk redo the gap work (two exponentials, two factors) and loop over the chunk's groups.  The chunk width is fixed,
// every column's arithmetic is the same whatever chunk it lies in, so neither the grid nor nrhs changes a value.
#pragma once
#include "cgps_leg.h"
#include "cgps_rng.h"

namespace cgps {

// where H_r comes from: nothing (the prior), one block [d][obs], a table [entries][d][obs] indexed by the row's
// pattern byte (clamped as leg_obs_block clamps it), or one block per row [R][d][obs]
constexpr int PERT_H_NONE = 0, PERT_H_PLAIN = 1, PERT_H_TABLE = 2, PERT_H_ROWS = 3;
constexpr int PERT_CHUNK_GROUPS = 16;

// L of Q = I - E E^T of one gap; with WANT_E, F becomes E itself
template <typename T, int D, bool WANT_E>
__device__ __forceinline__ bool perturb_gap(T dt, const T (&G)[D][D], Chol<T, D>& L, T (&F)[D][D]) {
  T Q[D][D];
  gap_expm1<T, D>(dt, [&](int i, int j) { return G[i][j]; }, F);
  gap_gram<T, D, true>(F, Q);
  bool f = false;
  chol_lower<T, D>(Q, L, f);
  if constexpr (WANT_E) add_identity<T, D>(F);
  return !f;
}

// the row arithmetic of both kernels below: lane `row` of column chunk `chunk` of `nchunks`; info_row0 is the number of
// the operands' first row in the system info speaks of (0, or k R for model k of a concatenated system)
template <typename T, int D, int HSRC>
__device__ __forceinline__ void leg_perturbation_row(
    int64_t row, unsigned chunk, unsigned nchunks, const T* __restrict__ ts, int64_t R, const T* __restrict__ Gg,
    const int64_t* __restrict__ roff, const int64_t* __restrict__ ids, int64_t B, const T* __restrict__ hterm, int entries,
    int obs, const unsigned char* __restrict__ pattern, const T* __restrict__ v, int64_t nrhs, int64_t groups,
    uint64_t seed, uint32_t stream, T* __restrict__ out, int* __restrict__ info, int64_t info_row0) {
  constexpr int GC = RngGroup<T>::COLS;
  if (row >= R) return;
  int64_t lo = 0, hi = B;                          // first b with roff[b + 1] > row
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (roff[mid + 1] <= row) lo = mid + 1; else hi = mid;
  }
  if (lo >= B) return;                             // (offsets that do not cover R rows: nothing is written)
  const int64_t r = row - roff[lo], n = roff[lo + 1] - roff[lo];
  const uint64_t base = (uint64_t)ids[lo] << 40;
  const bool has_prev = r > 0, has_next = r + 1 < n && row + 1 < R;

  T G[D][D];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) G[a][b] = Gg[a * D + b];
  Chol<T, D> Lp, Lc;                               // factors of Q of the gap before the row and of the gap after it
  T E[D][D];                                       // E of the gap after it
  bool ok = true;
  if (has_prev) {
    T F[D][D];
    ok = perturb_gap<T, D, false>(ts[row] - ts[row - 1], G, Lp, F) && ok;
  }
  if (has_next) ok = perturb_gap<T, D, true>(ts[row + 1] - ts[row], G, Lc, E) && ok;
  if (!ok && chunk == 0) report_fail(info, info_row0 + row);

  const T* __restrict__ H = hterm;
  if constexpr (HSRC == PERT_H_TABLE) {
    const int p = (int)pattern[row];
    H = hterm + (size_t)(p < entries - 1 ? p : entries - 1) * D * obs;
  } else if constexpr (HSRC == PERT_H_ROWS) {
    H = hterm + (size_t)row * D * obs;
  }
  T vr[D];
#pragma unroll
  for (int i = 0; i < D; ++i) vr[i] = v != nullptr ? v[row * D + i] : T(0);

  T* __restrict__ orow = out + row * D * nrhs;
  for (int64_t c0 = (int64_t)chunk * PERT_CHUNK_GROUPS; c0 < groups; c0 += (int64_t)nchunks * PERT_CHUNK_GROUPS) {
    const int64_t c1 = c0 + PERT_CHUNK_GROUPS < groups ? c0 + PERT_CHUNK_GROUPS : groups;
#pragma unroll 1
    for (int64_t g = c0; g < c1; ++g) {
      T w[GC][D];                                  // w[u]: column g GC + u of the row
#pragma unroll
      for (int i = 0; i < D; ++i) {                // eps_r
        T z[GC];
        normal_group(seed, stream, base + (uint64_t)(r * D + i), (uint32_t)g, z);
#pragma unroll
        for (int u = 0; u < GC; ++u) w[u][i] = z[u];
      }
      if (has_prev) {                              // u_{r-1} = L_{r-1}^-T eps_r
#pragma unroll
        for (int u = 0; u < GC; ++u) bwd_subst<T, D>(Lp, w[u]);
      }
      if (has_next) {                              // - E_r^T u_r,  u_r = L_r^-T eps_{r+1}
        T e[GC][D];
#pragma unroll
        for (int i = 0; i < D; ++i) {
          T z[GC];
          normal_group(seed, stream, base + (uint64_t)((r + 1) * D + i), (uint32_t)g, z);
#pragma unroll
          for (int u = 0; u < GC; ++u) e[u][i] = z[u];
        }
#pragma unroll
        for (int u = 0; u < GC; ++u) {
          bwd_subst<T, D>(Lc, e[u]);
          gemvT_sub<T, D>(w[u], E, e[u]);
        }
      }
      if constexpr (HSRC != PERT_H_NONE) {         // + H_r eps'_r
#pragma unroll 1
        for (int c = 0; c < obs; ++c) {
          T z[GC];
          normal_group(seed, stream + 1u, base + (uint64_t)(r * obs + c), (uint32_t)g, z);
#pragma unroll
          for (int i = 0; i < D; ++i) {
            const T h = H[i * obs + c];
#pragma unroll
            for (int u = 0; u < GC; ++u) w[u][i] = fmaT(h, z[u], w[u][i]);
          }
        }
      }
#pragma unroll
      for (int i = 0; i < D; ++i)
#pragma unroll
        for (int u = 0; u < GC; ++u)
          if (g * GC + u < nrhs) orow[i * nrhs + g * GC + u] = w[u][i] + vr[i];
    }
  }
}

template <typename T, int D, int HSRC>
__global__ __launch_bounds__(LEG_THREADS) void leg_perturbation_kernel(
    const T* __restrict__ ts, int64_t R, const T* __restrict__ Gg, const int64_t* __restrict__ roff,
    const int64_t* __restrict__ ids, int64_t B, const T* __restrict__ hterm, int entries, int obs,
    const unsigned char* __restrict__ pattern, const T* __restrict__ v, int64_t nrhs, int64_t groups, uint64_t seed,
    uint32_t stream, T* __restrict__ out, int* __restrict__ info) {
  leg_perturbation_row<T, D, HSRC>((int64_t)blockIdx.x * LEG_THREADS + threadIdx.x, blockIdx.y, gridDim.y, ts, R, Gg, roff, ids,
                                   B, hterm, entries, obs, pattern, v, nrhs, groups, seed, stream, out, info, 0);
}

// MODELS (cgps_leg_perturbation_models): the same R rows under gridDim.z models, the right-hand sides of the system
// "model 0's batch, then model 1's batch, ...".  blockIdx.z = k names the model: it brings G[k], v[k] of v[M][R][d],
// its factors hterm + k hstride (hstride = d obs, entries d obs or R d obs values by source) and its own stream word
// stream_ids[k]; ts, roff, ids and the pattern bytes belong to the data and are shared.  Every lane runs
// leg_perturbation_row on its model's slices, so rows k R .. (k + 1) R - 1 of out are leg_perturbation_kernel's for
// model k's operands bit for bit.
template <typename T, int D, int HSRC>
__global__ __launch_bounds__(LEG_THREADS) void leg_perturbation_models_kernel(
    const T* __restrict__ ts, int64_t R, const T* __restrict__ Gg, const int64_t* __restrict__ roff,
    const int64_t* __restrict__ ids, int64_t B, const T* __restrict__ hterm, size_t hstride, int entries, int obs,
    const unsigned char* __restrict__ pattern, const T* __restrict__ v, int64_t nrhs, int64_t groups, uint64_t seed,
    const int64_t* __restrict__ stream_ids, T* __restrict__ out, int* __restrict__ info) {
  const int64_t k = blockIdx.z;
  leg_perturbation_row<T, D, HSRC>((int64_t)blockIdx.x * LEG_THREADS + threadIdx.x, blockIdx.y, gridDim.y, ts, R,
                                   Gg + k * D * D, roff, ids, B, HSRC == PERT_H_NONE ? hterm : hterm + k * hstride, entries,
                                   obs, pattern, v != nullptr ? v + k * R * D : nullptr, nrhs, groups, seed,
                                   (uint32_t)stream_ids[k], out + k * R * D * nrhs, info, k * R);
}

}  // namespace cgps
