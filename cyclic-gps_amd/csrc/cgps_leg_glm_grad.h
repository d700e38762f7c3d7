// Gradient of the Laplace evidence at the mode (cgps_leg_glm_evidence_rhs, cgps_leg_glm_evidence_adjoint:
// include/cgps_glm_grad.h).
//
// Per series, at the mode z, with S = J^-1, P = K^-1, v_ic = B_c S_ii B_c^T and w' = dw / d eta:
//     E = sum l(y, eta) - 1/2 z^T K z + 1/2 log|K| - 1/2 log|J|
//   rhs      s_i = -1/2 sum_c w'_ic v_ic B_c^T              (dE / dz at the mode: only -1/2 log|J| depends on z there)
//   (solve)  u = J^-1 s, by the caller
//   adjoint  G_K = 1/2 (P - S) - 1/2 z z^T - 1/2 (u z^T + z u^T) on the block-tridiagonal pattern:
//              gRs[i] = gE G_K[i][i],  gOs[i] = 2 gE G_K[i+1][i]  (K holds Os[i] and its transpose)
//            e_ic = g_ic - 1/2 w'_ic v_ic - w_ic (B_c u_i):   dE / d log_exposure_ic = e_ic,  dE / d offset_c = sum_i e_ic,
//              dE / d B_c = sum_i [e_ic z_i + g_ic u_i - w_ic S_ii B_c^T]^T
//            Gaussian: dE / d s_ic = 1/2 res^2 / s^2 - 1/2 / s + 1/2 v_ic / s^2  (w' = 0, so s = u = 0)
//
// leg_glm_evidence_rhs_kernel, leg_glm_evidence_rows_kernel: grid ceil(R / GLM_GRAD_THREADS), one lane per row,
// everything in registers, nothing shared between lanes (the row kernel of cgps_leg_loo.h).  The rows kernel finds its
// series by bisection in offsets (for gE and for whether row i + 1 belongs to the same series).
// leg_glm_evidence_series_kernel: one workgroup of ONE wave per series, as cgps_leg_glm.h: lanes stride the series' rows
// and every sum is glm_wave_all, a fixed order, so a series' partials depend on nothing else in the batch.  No
// workspace: the wave forms each row's terms again from z, u and Sd rather than read them from a staging array.
#pragma once
#include "cgps_leg_glm.h"

namespace cgps {

constexpr int GLM_GRAD_THREADS = 256;

// w' = d w / d eta from the point at eta.  Poisson: e^eta = w.  Bernoulli: w (1 - 2 sigma), with 1 - 2 sigma =
// -+(1 - e) / (1 + e), e = exp(-|eta|): nothing cancels at either tail.  Gaussian: 0.
template <typename T>
__device__ __forceinline__ T glm_wprime(int family, T eta, const GlmPoint<T>& p) {
  if (family == GLM_POISSON) return p.w;
  if (family == GLM_BERNOULLI) {
    const T e = glm_exp(-glm_abs(eta));
    const T t = (T(1) - e) / (T(1) + e);                   // |1 - 2 sigma| = tanh(|eta| / 2)
    return eta >= T(0) ? -p.w * t : p.w * t;
  }
  return T(0);
}

// What a row's observed entry (i, c) needs: the point, w', v = B_c S B_c^T and S B_c^T
template <typename T, int D>
__device__ __forceinline__ T glm_quad_form(const T* __restrict__ Bc, const T (&S)[D][D], T (&sb)[D]) {
  T v = T(0);
#pragma unroll
  for (int a = 0; a < D; ++a) {
    T t = T(0);
#pragma unroll
    for (int k = 0; k < D; ++k) t = fmaT(S[a][k], Bc[k], t);
    sb[a] = t;
    v = fmaT(Bc[a], t, v);
  }
  return v;
}

template <typename T, int D>
__device__ __forceinline__ T glm_eta(const T* __restrict__ Bc, const T (&zi)[D], const T* __restrict__ offset,
                                     const T* __restrict__ extra, int family, int64_t at, int c) {
  T eta = offset != nullptr ? offset[c] : T(0);
#pragma unroll
  for (int a = 0; a < D; ++a) eta = fmaT(Bc[a], zi[a], eta);
  if (family != GLM_GAUSSIAN && extra != nullptr) eta += extra[at];
  return eta;
}

template <typename T, int D, int O>
__global__ __launch_bounds__(GLM_GRAD_THREADS) void leg_glm_evidence_rhs_kernel(
    const T* __restrict__ z, const T* __restrict__ Sd, const T* __restrict__ ys, const unsigned char* __restrict__ pattern,
    const T* __restrict__ offset, const T* __restrict__ extra, const T* __restrict__ Bg, int64_t R, int obs_rt, int family,
    T* __restrict__ s_out) {
  const int obs = O <= 4 ? O : obs_rt;
  const int64_t i = (int64_t)blockIdx.x * GLM_GRAD_THREADS + threadIdx.x;
  if (i >= R) return;
  const unsigned full = (1u << obs) - 1u;
  const unsigned p = pattern != nullptr ? ((unsigned)pattern[i] & full) : full;
  T s[D];
#pragma unroll
  for (int a = 0; a < D; ++a) s[a] = T(0);
  if (family != GLM_GAUSSIAN && p != 0u) {
    T zi[D], S[D][D];
    load_vec<T, D>(z + i * D, zi);
#pragma unroll
    for (int a = 0; a < D; ++a) load_vec<T, D>(Sd + (i * D + a) * D, S[a]);
#pragma unroll
    for (int c = 0; c < O; ++c) {
      if (c < obs && ((p >> c) & 1u)) {
        const T* __restrict__ Bc = Bg + c * D;
        const T eta = glm_eta<T, D>(Bc, zi, offset, extra, family, i * obs + c, c);
        const GlmPoint<T> pt = glm_point<T>(family, ys[i * obs + c], eta, T(1));
        T sb[D];
        const T v = glm_quad_form<T, D>(Bc, S, sb);
        const T f = T(-0.5) * glm_wprime<T>(family, eta, pt) * v;
#pragma unroll
        for (int a = 0; a < D; ++a) s[a] = fmaT(f, Bc[a], s[a]);
      }
    }
  }
  store_vec<T, D>(s_out + i * D, s);
}

// the series of row i: the last b with offsets[b] <= i (series of length 0 are passed over); B >= 1
__device__ __forceinline__ int64_t glm_series_of(const int64_t* __restrict__ offsets, int64_t B, int64_t i) {
  int64_t lo = 0, hi = B;                                  // offsets[lo] <= i < offsets[hi] where i lies inside the batch
  while (hi - lo > 1) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (offsets[mid] <= i) lo = mid;
    else hi = mid;
  }
  return lo;
}

template <typename T, int D, int O>
__global__ __launch_bounds__(GLM_GRAD_THREADS) void leg_glm_evidence_rows_kernel(
    const T* __restrict__ z, const T* __restrict__ u, const T* __restrict__ Sd, const T* __restrict__ So,
    const T* __restrict__ Pd, const T* __restrict__ Po, const T* __restrict__ ys, const unsigned char* __restrict__ pattern,
    const T* __restrict__ offset, const T* __restrict__ extra, const T* __restrict__ Bg, const int64_t* __restrict__ offsets,
    const double* __restrict__ gE, int64_t B, int64_t R, int obs_rt, int family, T* __restrict__ gRs, T* __restrict__ gOs,
    T* __restrict__ g_extra) {
  const int obs = O <= 4 ? O : obs_rt;
  const int64_t i = (int64_t)blockIdx.x * GLM_GRAD_THREADS + threadIdx.x;
  if (i >= R) return;
  const int64_t b = glm_series_of(offsets, B, i);
  const bool mine = offsets[b] <= i && i < offsets[b + 1];  // (false only for offsets that do not cover 0 .. R)
  const T ge = mine ? (T)gE[b] : T(0);
  const bool dropped = ge == T(0);                         // selected, not multiplied: a dropped series writes exact zeros
                                                           // whatever its operands hold, NaN and infinities included
  const bool next = mine && i + 1 < R && i + 1 < offsets[b + 1];
  const unsigned full = (1u << obs) - 1u;
  const unsigned p = pattern != nullptr ? ((unsigned)pattern[i] & full) : full;

  T zi[D], ui[D];
  load_vec<T, D>(z + i * D, zi);
  load_vec<T, D>(u + i * D, ui);

  // ---- the cotangent of every observed linear predictor (or variance) of the row --------------------------------------
  {
    T S[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a) load_vec<T, D>(Sd + (i * D + a) * D, S[a]);
#pragma unroll
    for (int c = 0; c < O; ++c) {
      if (c < obs) {
        T out = T(0);
        if ((p >> c) & 1u) {
          const T* __restrict__ Bc = Bg + c * D;
          const T eta = glm_eta<T, D>(Bc, zi, offset, extra, family, i * obs + c, c);
          const T sv = family == GLM_GAUSSIAN ? extra[i * obs + c] : T(1);
          const GlmPoint<T> pt = glm_point<T>(family, ys[i * obs + c], eta, sv);
          T sb[D];
          const T v = glm_quad_form<T, D>(Bc, S, sb);
          if (family == GLM_GAUSSIAN) {
            out = T(0.5) * (pt.g * pt.g - pt.w + v * pt.w * pt.w);   // g = res / s, w = 1 / s
          } else {
            T bu = T(0);
#pragma unroll
            for (int a = 0; a < D; ++a) bu = fmaT(Bc[a], ui[a], bu);
            out = pt.g - T(0.5) * glm_wprime<T>(family, eta, pt) * v - pt.w * bu;
          }
          out = dropped ? T(0) : ge * out;
        }
        g_extra[i * obs + c] = out;
      }
    }
    // ---- gRs[i] = gE (1/2 (P - S) - 1/2 z z^T - 1/2 (u z^T + z u^T)) ---------------------------------------------------
#pragma unroll
    for (int a = 0; a < D; ++a) {
      T row[D];
      load_vec<T, D>(Pd + (i * D + a) * D, row);
#pragma unroll
      for (int k = 0; k < D; ++k) {
        T t = row[k] - S[a][k];
        t = fmaT(-zi[a], zi[k], t);
        t = fmaT(-ui[a], zi[k], t);
        t = fmaT(-zi[a], ui[k], t);
        row[k] = dropped ? T(0) : T(0.5) * ge * t;
      }
      store_vec<T, D>(gRs + (i * D + a) * D, row);
    }
  }
  // ---- gOs[i] = gE ((P - S)[i+1][i] - z_{i+1} z_i^T - u_{i+1} z_i^T - z_{i+1} u_i^T); zero between two series -------------
  if (i + 1 < R) {
    T zn[D], un[D];
#pragma unroll
    for (int a = 0; a < D; ++a) {
      zn[a] = next ? z[(i + 1) * D + a] : T(0);
      un[a] = next ? u[(i + 1) * D + a] : T(0);
    }
#pragma unroll
    for (int a = 0; a < D; ++a) {
      T row[D];
#pragma unroll
      for (int k = 0; k < D; ++k) row[k] = T(0);
      if (next) {
        T so[D];
        load_vec<T, D>(Po + (i * D + a) * D, row);
        load_vec<T, D>(So + (i * D + a) * D, so);
#pragma unroll
        for (int k = 0; k < D; ++k) {
          T t = row[k] - so[k];
          t = fmaT(-zn[a], zi[k], t);
          t = fmaT(-un[a], zi[k], t);
          t = fmaT(-zn[a], ui[k], t);
          row[k] = dropped ? T(0) : ge * t;
        }
      }
      store_vec<T, D>(gOs + (i * D + a) * D, row);
    }
  }
}

template <typename T, int D, int O>
__global__ __launch_bounds__(GLM_THREADS) void leg_glm_evidence_series_kernel(
    const T* __restrict__ z, const T* __restrict__ u, const T* __restrict__ Sd, const T* __restrict__ ys,
    const unsigned char* __restrict__ pattern, const T* __restrict__ offset, const T* __restrict__ extra,
    const T* __restrict__ Bg, const int64_t* __restrict__ offsets, const double* __restrict__ gE, int64_t R, int obs_rt,
    int family, double* __restrict__ gB_part, double* __restrict__ goffset_part) {
  const int obs = O <= 4 ? O : obs_rt;
  const int64_t b = blockIdx.x;
  int64_t r0 = offsets[b], r1 = offsets[b + 1];
  r0 = r0 < 0 ? 0 : r0;
  r1 = r1 > R ? R : r1;
  const int lane = threadIdx.x;
  const unsigned full = (1u << obs) - 1u;
  double accB[O][D], accO[O];
#pragma unroll
  for (int c = 0; c < O; ++c) {
    accO[c] = 0.0;
#pragma unroll
    for (int a = 0; a < D; ++a) accB[c][a] = 0.0;
  }
  for (int64_t i = r0 + lane; i < r1; i += GLM_THREADS) {
    const unsigned p = pattern != nullptr ? ((unsigned)pattern[i] & full) : full;
    if (p == 0u) continue;
    T zi[D], ui[D], S[D][D];
    load_vec<T, D>(z + i * D, zi);
    load_vec<T, D>(u + i * D, ui);
#pragma unroll
    for (int a = 0; a < D; ++a) load_vec<T, D>(Sd + (i * D + a) * D, S[a]);
#pragma unroll
    for (int c = 0; c < O; ++c) {
      if (c < obs && ((p >> c) & 1u)) {
        const T* __restrict__ Bc = Bg + c * D;
        const T eta = glm_eta<T, D>(Bc, zi, offset, extra, family, i * obs + c, c);
        const T sv = family == GLM_GAUSSIAN ? extra[i * obs + c] : T(1);
        const GlmPoint<T> pt = glm_point<T>(family, ys[i * obs + c], eta, sv);
        T sb[D];
        const T v = glm_quad_form<T, D>(Bc, S, sb);
        T bu = T(0);
#pragma unroll
        for (int a = 0; a < D; ++a) bu = fmaT(Bc[a], ui[a], bu);
        const T e = pt.g - T(0.5) * glm_wprime<T>(family, eta, pt) * v - pt.w * bu;
        accO[c] += (double)e;
#pragma unroll
        for (int a = 0; a < D; ++a) accB[c][a] += (double)fmaT(e, zi[a], fmaT(pt.g, ui[a], -pt.w * sb[a]));
      }
    }
  }
  const double ge = gE[b];
#pragma unroll
  for (int c = 0; c < O; ++c) {
    if (c < obs) {
      const double so = glm_wave_all(accO[c]);
      if (lane == 0) goffset_part[b * obs + c] = ge == 0.0 ? 0.0 : ge * so;
#pragma unroll
      for (int a = 0; a < D; ++a) {
        const double sB = glm_wave_all(accB[c][a]);
        if (lane == 0) gB_part[(b * obs + c) * D + a] = ge == 0.0 ? 0.0 : ge * sB;
      }
    }
  }
}

template <typename T, int D>
void launch_glm_evidence_rhs(const T* z, const T* Sd, const T* ys, const unsigned char* pattern, const T* offset,
                             const T* extra, const T* Bm, int64_t R, int obs, int family, T* s, hipStream_t st) {
  const dim3 grid((unsigned)((R + GLM_GRAD_THREADS - 1) / GLM_GRAD_THREADS)), block(GLM_GRAD_THREADS);
  cgps_host::dispatch_obs(obs, [&](auto oc) {
    hipLaunchKernelGGL((leg_glm_evidence_rhs_kernel<T, D, decltype(oc)::value>), grid, block, 0, st, z, Sd, ys, pattern, offset,
                       extra, Bm, R, obs, family, s);
  });
}

template <typename T, int D>
void launch_glm_evidence_adjoint(const T* z, const T* u, const T* Sd, const T* So, const T* Pd, const T* Po, const T* ys,
                                 const unsigned char* pattern, const T* offset, const T* extra, const T* Bm,
                                 const int64_t* offsets, const double* gE, int64_t B, int64_t R, int obs, int family, T* gRs,
                                 T* gOs, T* g_extra, double* gB_part, double* goffset_part, hipStream_t st) {
  const dim3 grid((unsigned)((R + GLM_GRAD_THREADS - 1) / GLM_GRAD_THREADS)), block(GLM_GRAD_THREADS);
  cgps_host::dispatch_obs(obs, [&](auto oc) {
    constexpr int O = decltype(oc)::value;
    hipLaunchKernelGGL((leg_glm_evidence_rows_kernel<T, D, O>), grid, block, 0, st, z, u, Sd, So, Pd, Po, ys, pattern, offset,
                       extra, Bm, offsets, gE, B, R, obs, family, gRs, gOs, g_extra);
    hipLaunchKernelGGL((leg_glm_evidence_series_kernel<T, D, O>), dim3((unsigned)B), dim3(GLM_THREADS), 0, st, z, u, Sd, ys,
                       pattern, offset, extra, Bm, offsets, gE, R, obs, family, gB_part, goffset_part);
  });
}

}  // namespace cgps
