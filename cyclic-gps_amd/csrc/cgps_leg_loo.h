// Leave-one-out predictives of LEG series from the posterior the library already computes: the
// distribution of every observed entry given all other observed entries (LOO_ENTRY), or of every row's observed entries
// given all other rows (LOO_ROW), for every row of B concatenated series under M models, and the LOO-CV score
// sum log p(x_i | x_-i) of every (model, series).
//
// Row i observes the channels of its pattern byte p (mask m = diag of p's bits) with noise Cn = LLT + diag(s_i)
// (LLT = Lambda Lambda^T + 1e-9 I as the caller passes it; s is 0 where nothing is given and never read where nothing
// is observed).  With W = m Cn m + (I - m) = T T^T (T lower; an unobserved channel is an identity row and column of W
// and of T, so it drops out of every product below), Li = m W^-1 m, the posterior N(mu_i, S_ii) of the row's latent
// and Bm its observation matrix:
//     e = m (x~ - Bm mu_i),   g = Li e = T^-T T^-1 e,
//     P = Li - Li (Bm S_ii Bm^T) Li = T^-T (m - T^-1 (m Bm S_ii Bm^T m) T^-1^T) T^-1.
// P is the row's diagonal block, g the row's block of  P_all x,  of the precision P_all of the marginal Gaussian of all
// observed entries (Woodbury), so
//     LOO_ENTRY:  var = 1 / P[c][c],  mean = x_c - g_c / P[c][c],  logpdf = -1/2 g_c^2 / P[c][c] + 1/2 log P[c][c] - 1/2 log 2 pi
//     LOO_ROW:    cov = (P[o][o])^-1,  mean = x_o - cov g_o,  logpdf = -1/2 g_o^T cov g_o + 1/2 log|P[o][o]| - k/2 log 2 pi.
// The one cancellation of the evaluation is  m - T^-1 (..) T^-T  (two matrices of size 1 in the whitened basis); it
// costs the factor kappa = Li[c][c] var_loo of DESIGN 4.20 and nothing else does.
//
// leg_loo_rows_kernel: grid (ceil(R / LOO_THREADS), M), one lane per (row, model), everything in registers: the
// channel axis is a compile-time O (1..4: obs = O; 8: 1 <= obs <= 8 at run time, the channels from obs up behave as
// unobserved ones), all loops are unrolled over it.  Model k (blockIdx.y) reads Bm[k], LLT[k] and rows k R .. of the
// posterior; xs, pattern and noise_var belong to the data and are shared.  A pivot of W or of P[o][o], or a P[c][c],
// that is not positive, or a result that is not finite, fails the row: all its outputs become NaN and info gets
// 1 + (k R + i) (report_fail).  Unobserved entries: mean = var = NaN, logpdf = 0.
// leg_loo_score_kernel: grid (B, M), one workgroup per (model, series): the series' logpdf values are added in a
// fixed order that depends on the series' own rows only (lane t takes local rows t, t + LOO_THREADS, ...; then
// block_sum2), in double, no atomics: a series' score does not depend on its place in the batch.
#pragma once
#include "cgps_host.h"
#include "cgps_math.h"

namespace cgps {

constexpr int LOO_THREADS = 256;
constexpr int LOO_ENTRY = 0, LOO_ROW = 1;

__device__ __forceinline__ float logT(float a) { return logf(a); }
__device__ __forceinline__ double logT(double a) { return log(a); }
__device__ __forceinline__ bool finiteT(float a) { return __builtin_isfinite(a); }
__device__ __forceinline__ bool finiteT(double a) { return __builtin_isfinite(a); }

// X <- L^-1 X, column by column (forward substitution down the rows)
template <typename T, int O>
__device__ __forceinline__ void lsolve_cols(const Chol<T, O>& c, T (&X)[O][O]) {
#pragma unroll
  for (int j = 0; j < O; ++j)
#pragma unroll
    for (int q = 0; q < O; ++q) {
      T s = X[j][q];
#pragma unroll
      for (int m = 0; m < j; ++m) s = fmaT(-c.l[j][m], X[m][q], s);
      X[j][q] = s * c.inv[j];
    }
}

// X <- L^-T X, column by column (backward substitution up the rows)
template <typename T, int O>
__device__ __forceinline__ void ltsolve_cols(const Chol<T, O>& c, T (&X)[O][O]) {
#pragma unroll
  for (int j = O - 1; j >= 0; --j)
#pragma unroll
    for (int q = 0; q < O; ++q) {
      T s = X[j][q];
#pragma unroll
      for (int m = j + 1; m < O; ++m) s = fmaT(-c.l[m][j], X[m][q], s);
      X[j][q] = s * c.inv[j];
    }
}

template <typename T, int D, int O>
__global__ __launch_bounds__(LOO_THREADS) void leg_loo_rows_kernel(
    const T* __restrict__ xs, const unsigned char* __restrict__ pattern, const T* __restrict__ noise, int64_t R,
    const T* __restrict__ Bg, const T* __restrict__ LLTg, int obs_rt, const T* __restrict__ mean_g,
    const T* __restrict__ Sd_g, int leave, T* __restrict__ out_mean, T* __restrict__ out_var,
    T* __restrict__ out_logpdf, int* __restrict__ info) {
  const int obs = O <= 4 ? O : obs_rt;
  const int64_t i = (int64_t)blockIdx.x * LOO_THREADS + threadIdx.x;
  if (i >= R) return;
  const int64_t k = blockIdx.y, row = k * R + i;
  const unsigned full = (1u << obs) - 1u;
  const unsigned p = pattern != nullptr ? ((unsigned)pattern[i] & full) : full;
  const T* __restrict__ Bk = Bg + (size_t)k * obs * D;
  const T* __restrict__ Ck = LLTg + (size_t)k * obs * obs;
  const T nan = (T)__builtin_nan("");

  bool on[O];
  T x[O], s[O];
#pragma unroll
  for (int c = 0; c < O; ++c) {
    on[c] = (p >> c) & 1u;                         // (false for every c >= obs)
    x[c] = on[c] ? xs[i * obs + c] : T(0);
    s[c] = (on[c] && noise != nullptr) ? noise[i * obs + c] : T(0);
  }

  // e = m (x~ - Bm mu),  Y = m Bm S Bm^T m
  T e[O], Y[O][O];
  {
    T mu[D], S[D][D], Bm[O][D];
    load_vec<T, D>(mean_g + row * D, mu);
#pragma unroll
    for (int a = 0; a < D; ++a) load_vec<T, D>(Sd_g + (row * D + a) * D, S[a]);
#pragma unroll
    for (int c = 0; c < O; ++c)
#pragma unroll
      for (int a = 0; a < D; ++a) Bm[c][a] = c < obs ? Bk[c * D + a] : T(0);
#pragma unroll
    for (int c = 0; c < O; ++c) {
      T r = x[c];
#pragma unroll
      for (int a = 0; a < D; ++a) r = fmaT(-Bm[c][a], mu[a], r);
      e[c] = on[c] ? r : T(0);
      T bs[D];                                     // row c of Bm S
#pragma unroll
      for (int b = 0; b < D; ++b) {
        T t = T(0);
#pragma unroll
        for (int a = 0; a < D; ++a) t = fmaT(Bm[c][a], S[a][b], t);
        bs[b] = t;
      }
#pragma unroll
      for (int q = 0; q <= c; ++q) {
        T t = T(0);
#pragma unroll
        for (int b = 0; b < D; ++b) t = fmaT(bs[b], Bm[q][b], t);
        Y[c][q] = Y[q][c] = (on[c] && on[q]) ? t : T(0);
      }
    }
  }

  // W = m Cn m + (I - m) = T T^T
  Chol<T, O> Tw;
  bool fail = false;
  {
    T W[O][O];
#pragma unroll
    for (int c = 0; c < O; ++c)
#pragma unroll
      for (int q = 0; q <= c; ++q) {
        T w = c == q ? T(1) : T(0);
        if (on[c] && on[q]) w = Ck[c * obs + q] + (c == q ? s[c] : T(0));
        W[c][q] = W[q][c] = w;
      }
    chol_lower<T, O>(W, Tw, fail);
  }

  // P = T^-T (m - T^-1 Y T^-T) T^-1,  g = T^-T T^-1 e
  rsolve_lt<T, O>(Tw, Y);                          // Y T^-T
  lsolve_cols<T, O>(Tw, Y);                        // T^-1 Y T^-T
#pragma unroll
  for (int c = 0; c < O; ++c)
#pragma unroll
    for (int q = 0; q < O; ++q) Y[c][q] = ((c == q && on[c]) ? T(1) : T(0)) - Y[c][q];
#pragma unroll
  for (int c = 0; c < O; ++c) bwd_subst<T, O>(Tw, Y[c]);   // (..) T^-1, row by row
  ltsolve_cols<T, O>(Tw, Y);                       // P
  fwd_subst<T, O>(Tw, e);
  bwd_subst<T, O>(Tw, e);                          // g

  const T half_log_2pi = T(0.91893853320467274178);
  if (leave == LOO_ENTRY) {
    T mean[O], var[O], lp[O];
#pragma unroll
    for (int c = 0; c < O; ++c) {
      const T pcc = Y[c][c];
      const T v = T(1) / pcc;
      fail = fail || (on[c] && !(pcc > T(0)));
      mean[c] = x[c] - e[c] * v;
      var[c] = v;
      lp[c] = T(-0.5) * e[c] * e[c] * v + T(0.5) * logT(pcc) - half_log_2pi;
      fail = fail || (on[c] && !(finiteT(mean[c]) && finiteT(v) && finiteT(lp[c])));
    }
    if (fail) report_fail(info, row);
#pragma unroll
    for (int c = 0; c < O; ++c)
      if (c < obs) {
        out_mean[row * obs + c] = (on[c] && !fail) ? mean[c] : nan;
        out_var[row * obs + c] = (on[c] && !fail) ? var[c] : nan;
        out_logpdf[row * obs + c] = fail ? nan : (on[c] ? lp[c] : T(0));
      }
  } else {
    // P[o][o] embedded in the identity = Tp Tp^T;  cov = Tp^-T Tp^-1
    Chol<T, O> Tp;
#pragma unroll
    for (int c = 0; c < O; ++c)
#pragma unroll
      for (int q = 0; q < O; ++q)
        if (!(on[c] && on[q])) Y[c][q] = c == q ? T(1) : T(0);
    const double det = chol_lower<T, O>(Y, Tp, fail);
    T X[O][O];                                     // X[r] = Tp^-1 e_r: X = Tp^-T
#pragma unroll
    for (int r = 0; r < O; ++r) {
#pragma unroll
      for (int q = 0; q < O; ++q) X[r][q] = r == q ? T(1) : T(0);
      fwd_subst<T, O>(Tp, X[r]);
    }
    fwd_subst<T, O>(Tp, e);                        // h = Tp^-1 g
    T quad = T(0);
    int cnt = 0;
#pragma unroll
    for (int c = 0; c < O; ++c) {
      quad = fmaT(e[c], e[c], quad);
      cnt += on[c] ? 1 : 0;
    }
    bwd_subst<T, O>(Tp, e);                        // cov g
    const T lp = cnt == 0 ? T(0) : T(-0.5) * quad + T(0.5) * (T)log(det) - T(cnt) * half_log_2pi;
    fail = fail || !finiteT(lp);
    T cov[O][O];
#pragma unroll
    for (int c = 0; c < O; ++c)
#pragma unroll
      for (int q = 0; q <= c; ++q) {
        T t = T(0);
#pragma unroll
        for (int m = c; m < O; ++m) t = fmaT(X[c][m], X[q][m], t);   // X[c][m] = 0 for m < c
        cov[c][q] = cov[q][c] = t;
        fail = fail || (on[c] && on[q] && !finiteT(t));
      }
#pragma unroll
    for (int c = 0; c < O; ++c) fail = fail || (on[c] && !finiteT(e[c]));
    if (fail) report_fail(info, row);
    out_logpdf[row] = fail ? nan : lp;
#pragma unroll
    for (int c = 0; c < O; ++c)
      if (c < obs) {
        out_mean[row * obs + c] = (on[c] && !fail) ? x[c] - e[c] : nan;
#pragma unroll
        for (int q = 0; q < O; ++q)
          if (q < obs) out_var[(row * obs + c) * obs + q] = (on[c] && on[q] && !fail) ? cov[c][q] : nan;
      }
  }
}

// out_score[k][b] = the sum of series b's log densities under model k; per = values per row (obs or 1)
template <typename T>
__global__ __launch_bounds__(LOO_THREADS) void leg_loo_score_kernel(const T* __restrict__ logpdf,
                                                                      const int64_t* __restrict__ roff, int64_t R, int per,
                                                                      double* __restrict__ out_score) {
  __shared__ double red[2 * (LOO_THREADS / 64)];
  const int64_t b = blockIdx.x, k = blockIdx.y;
  int64_t r0 = roff[b], r1 = roff[b + 1];
  r0 = r0 < 0 ? 0 : r0;
  r1 = r1 > R ? R : r1;                            // (offsets that do not fit R rows: nothing outside is read)
  double a = 0.0, unused = 0.0;
  for (int64_t r = r0 + threadIdx.x; r < r1; r += LOO_THREADS) {
    const T* __restrict__ lp = logpdf + (k * R + r) * per;
    for (int c = 0; c < per; ++c) a += (double)lp[c];
  }
  block_sum2<LOO_THREADS>(a, unused, red);
  if (threadIdx.x == 0) out_score[k * gridDim.x + b] = a;
}

template <typename T, int D>
void launch_loo(const T* xs, const unsigned char* pattern, const T* noise, const int64_t* roff, int64_t B, int64_t R,
                int64_t M, const T* Bm, const T* LLT, int obs, const T* mean, const T* Sd, int leave, T* out_mean,
                T* out_var, T* out_logpdf, double* out_score, int* info, hipStream_t st) {
  const dim3 grid((unsigned)((R + LOO_THREADS - 1) / LOO_THREADS), (unsigned)M), block(LOO_THREADS);
  cgps_host::dispatch_obs(obs, [&](auto oc) {
    hipLaunchKernelGGL((leg_loo_rows_kernel<T, D, decltype(oc)::value>), grid, block, 0, st, xs, pattern, noise, R, Bm, LLT,
                       obs, mean, Sd, leave, out_mean, out_var, out_logpdf, info);
  });
  hipLaunchKernelGGL((leg_loo_score_kernel<T>), dim3((unsigned)B, (unsigned)M), block, 0, st, out_logpdf, roff, R,
                     leave == LOO_ENTRY ? obs : 1, out_score);
}

}  // namespace cgps
