// Replicated observations: data sets drawn from the observation model given latent paths,
//     x[k][row][c][s] = sum_j Bm[k][c][j] z[k][row][j][s] + sum_c' T[c][c'] eps''[c'][s],
//     T T^T = LLT[k] + diag(s_row)   (T lower),
// for every row of B concatenated series under M models and every column, in one launch.  s_row[c] is the row's extra
// noise variance where the entry is observed and 0 elsewhere (never read where nothing is observed): the replicate is
// the distribution of the data at EVERY row, observed or not, so the mask only says which variances exist.
// eps''[c'], column s, is element (id 2^40 + r obs + c', s) of the generator of cgps_rng.h under stream word
// stream_ids[k] + 2 -- the two words below it are the ones a posterior draw of the series uses (cgps_leg_perturb.h) --
// with r the row's index INSIDE its series and id the series' caller-visible number: a series' replicate does not
// depend on its place in the batch.
//
// One lane per (row, model): grid (ceil(R / LEG_THREADS), column chunks, M).  The lane finds its series by binary
// search in row_offsets (leg_perturbation_row's search), factors its own T in registers and loops over its chunk's
// generator groups: the chunk width is fixed and a column's arithmetic is the same in every chunk, so neither the grid
// nor nrhs changes a value.  The noise lives in registers only.  The channel axis is a compile-time O as in
// leg_loo_rows_kernel (1..4: obs = O; 8: 1 <= obs <= 8 at run time, the channels from obs up are identity rows of T
// that nothing reads); the rank d is a run-time bound: z is consumed one latent coordinate at a time, straight into
// the O accumulators of a column, so no register array is indexed by it.
#pragma once
#include "cgps_leg.h"
#include "cgps_rng.h"

namespace cgps {

constexpr int REPL_CHUNK_GROUPS = 16;

template <typename T, int O>
__global__ __launch_bounds__(LEG_THREADS) void leg_observations_kernel(
    const T* __restrict__ z, int64_t R, int d, const T* __restrict__ Bg, const T* __restrict__ LLTg, int obs_rt,
    const unsigned char* __restrict__ pattern, const T* __restrict__ noise, const int64_t* __restrict__ roff,
    const int64_t* __restrict__ ids, int64_t B, int64_t nrhs, int64_t groups, uint64_t seed,
    const int64_t* __restrict__ stream_ids, T* __restrict__ x, int* __restrict__ info) {
  constexpr int GC = RngGroup<T>::COLS;
  const int obs = O <= 4 ? O : obs_rt;
  const int64_t i = (int64_t)blockIdx.x * LEG_THREADS + threadIdx.x;
  if (i >= R) return;
  int64_t lo = 0, hi = B;                          // first b with roff[b + 1] > i
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (roff[mid + 1] <= i) lo = mid + 1; else hi = mid;
  }
  if (lo >= B) return;                             // (offsets that do not cover R rows: nothing is written)
  const int64_t k = blockIdx.z, row = k * R + i, r = i - roff[lo];
  const uint64_t base = ((uint64_t)ids[lo] << 40) + (uint64_t)(r * obs);
  const uint32_t stream = (uint32_t)stream_ids[k] + 2u;
  const T* __restrict__ Bk = Bg + (size_t)k * obs * d;
  const T* __restrict__ Ck = LLTg + (size_t)k * obs * obs;
  const unsigned full = (1u << obs) - 1u;
  const unsigned p = pattern != nullptr ? ((unsigned)pattern[i] & full) : full;

  Chol<T, O> Tw;                                   // LLT + diag(s) = T T^T
  {
    T W[O][O];
#pragma unroll
    for (int c = 0; c < O; ++c)
#pragma unroll
      for (int q = 0; q <= c; ++q) {
        T w = c == q ? T(1) : T(0);
        if (c < obs) {                             // (q <= c < obs)
          w = Ck[c * obs + q];
          if (c == q && noise != nullptr && ((p >> c) & 1u)) w += noise[i * obs + c];
        }
        W[c][q] = W[q][c] = w;
      }
    bool fail = false;
    chol_lower<T, O>(W, Tw, fail);
    if (fail && blockIdx.y == 0) report_fail(info, row);
  }

  const T* __restrict__ zrow = z + row * d * nrhs;
  T* __restrict__ xrow = x + row * obs * nrhs;
  for (int64_t c0 = (int64_t)blockIdx.y * REPL_CHUNK_GROUPS; c0 < groups; c0 += (int64_t)gridDim.y * REPL_CHUNK_GROUPS) {
    const int64_t c1 = c0 + REPL_CHUNK_GROUPS < groups ? c0 + REPL_CHUNK_GROUPS : groups;
#pragma unroll 1
    for (int64_t g = c0; g < c1; ++g) {
      T acc[O][GC];                                // acc[c][u]: channel c, column g GC + u
#pragma unroll
      for (int c = 0; c < O; ++c)
#pragma unroll
        for (int u = 0; u < GC; ++u) acc[c][u] = T(0);
#pragma unroll 1
      for (int j = 0; j < d; ++j) {                // Bm z
        T zj[GC];
#pragma unroll
        for (int u = 0; u < GC; ++u) zj[u] = g * GC + u < nrhs ? zrow[j * nrhs + g * GC + u] : T(0);
#pragma unroll
        for (int c = 0; c < O; ++c) {
          const T b = c < obs ? Bk[c * d + j] : T(0);
#pragma unroll
          for (int u = 0; u < GC; ++u) acc[c][u] = fmaT(b, zj[u], acc[c][u]);
        }
      }
#pragma unroll
      for (int q = 0; q < O; ++q) {                // + T eps'', one column of T at a time
        if (q < obs) {
          T e[GC];
          normal_group(seed, stream, base + (uint64_t)q, (uint32_t)g, e);
#pragma unroll
          for (int c = q; c < O; ++c)
#pragma unroll
            for (int u = 0; u < GC; ++u) acc[c][u] = fmaT(Tw.l[c][q], e[u], acc[c][u]);
        }
      }
#pragma unroll
      for (int c = 0; c < O; ++c)
#pragma unroll
        for (int u = 0; u < GC; ++u)
          if (c < obs && g * GC + u < nrhs) xrow[c * nrhs + g * GC + u] = acc[c][u];
    }
  }
}

}  // namespace cgps
