// The causal quantities of LEG series: for every row i of B concatenated series under M models, the
// one-step-ahead predictive p(x_i | x_<i) of the row's observation, its log density at the value that was seen, and the
// filtered state z_i | x_<=i; per (model, series) the log-likelihood sum_i log p(x_i | x_<i) and the state after the
// last row, from which a later call continues.
//
// The recursion, in the conventions of cgps_leg.h.  The prior of a series' first row is N(0, I).  Across a gap dt,
// E = exp(-1/2 dt G) = I + gap_expm1, and the state N(m, P) becomes  m^- = E m,  P^- = I + E (P - I) E^T.  The kernel
// carries Dm = P - I, Dm^- = E Dm E^T: no I - E E^T is formed, so a short gap costs nothing and a gap of zero length is
// legal (E = I).  Row i observes the channels o of its pattern byte with noise Cn = LLT + diag(s_i) (LLT = Lambda
// Lambda^T + 1e-9 I as the caller passes it; s is 0 where nothing is given and never read where nothing is observed):
//     predictive of ALL channels:  N(Bm m^-,  Bm P^- Bm^T + LLT + diag(s_i on o))
//     e = x_o - Bm_o m^-,   S = (Bm P^- Bm^T + Cn)[o, o] = T T^T   (an unobserved channel is an identity row and column)
//     logpdf = -1/2 |T^-1 e|^2 - sum log T_cc - k/2 log 2 pi        (0 for a row that observes nothing)
//     V = T^-1 Bm_o P^-,   m = m^- + V^T (T^-1 e),   Dm = Dm^- - V^T V
// A row that observes nothing has V = 0 and e = 0: m = m^- and P = P^- to the bit.
//
// leg_filter_kernel: grid (ceil(B / FILTER_THREADS), M), one lane per (series, model) walks the series' rows with
// m, Dm, E and the obs x obs factor in registers; no atomics but report_fail's, no workspace, no LDS.  The channel axis
// is a compile-time O (1..4: obs = O; 8: 1 <= obs <= 8 at run time, the channels from obs up behave as unobserved ones).
// The work is serial in a series' rows, and a row's matrix exponential (13 + squarings products of d x d blocks) is
// three quarters of it -- but E depends on the time stamps alone, so it is the one part that is parallel in time:
// leg_filter_gaps_kernel (one lane per (row, model)) evaluates E of the gap before every row first and leaves it in the
// row's slot of z_cov, where the walking lane reads it just before it stores the row's z_cov over it.  What stays in
// the chain is about four d x d products and the obs x obs factor per row.  Only the gap from a start state t0 to a
// series' first row is evaluated by the walking lane itself (gap_expm1, the same routine: the same bits).
// A gap that is negative or not finite, a pivot of S that is not positive, or a result that is not finite fails the
// row: it and every later row of that series under that model are NaN, the series' log-likelihood and end state are
// NaN, and info gets 1 + (k R + i) of the first such row (report_fail).
#pragma once
#include "cgps_host.h"
#include "cgps_leg.h"
#include "cgps_leg_loo.h"

namespace cgps {

constexpr int FILTER_THREADS = 64;

// E of the gap before every row but the first of the R, under every model, into that row's slot of z_cov: one lane per
// (row, model), grid (ceil(R / FILTER_THREADS), M).  The gap before a series' first row is the previous series' business
// or nobody's: its slot is written and never read.  A gap that is negative or not finite is evaluated as zero; the lane
// that walks the series fails the row from the time stamps themselves.
template <typename T, int D>
__global__ __launch_bounds__(FILTER_THREADS) void leg_filter_gaps_kernel(const T* __restrict__ ts, int64_t R,
                                                                         const T* __restrict__ Gg, T* __restrict__ z_cov) {
  const int64_t i = (int64_t)blockIdx.x * FILTER_THREADS + threadIdx.x;
  if (i < 1 || i >= R) return;
  const int64_t k = blockIdx.y;
  const T* __restrict__ Gk = Gg + (size_t)k * D * D;
  const T dt = ts[i] - ts[i - 1];
  T E[D][D];
  gap_expm1<T, D>((dt >= T(0) && finiteT(dt)) ? dt : T(0), [&](int a, int c) { return Gk[a * D + c]; }, E);
  add_identity<T, D>(E);
  T* __restrict__ out = z_cov + (k * R + i) * D * D;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int c = 0; c < D; ++c) out[a * D + c] = E[a][c];
}

template <typename T, int D, int O>
__global__ __launch_bounds__(FILTER_THREADS) void leg_filter_kernel(
    const T* __restrict__ ts, const T* __restrict__ xs, const unsigned char* __restrict__ pattern,
    const T* __restrict__ noise, const int64_t* __restrict__ roff, int64_t B, int64_t R, const T* __restrict__ Gg,
    const T* __restrict__ Bg, const T* __restrict__ LLTg, int obs_rt, const T* __restrict__ t0, const T* __restrict__ m0,
    const T* __restrict__ P0, T* __restrict__ pred_mean, T* __restrict__ pred_cov, T* __restrict__ logpdf,
    T* __restrict__ z_mean, T* z_cov, double* __restrict__ loglik, T* __restrict__ m_end,
    T* __restrict__ P_end, int* __restrict__ info) {
  const int obs = O <= 4 ? O : obs_rt;
  const int64_t b = (int64_t)blockIdx.x * FILTER_THREADS + threadIdx.x;
  if (b >= B) return;
  const int64_t k = blockIdx.y;
  int64_t r0 = roff[b], r1 = roff[b + 1];
  r0 = r0 < 0 ? 0 : r0;
  r1 = r1 > R ? R : r1;                            // (offsets that do not fit R rows: nothing outside is touched)
  const T* __restrict__ Gk = Gg + (size_t)k * D * D;
  const T* __restrict__ Bk = Bg + (size_t)k * obs * D;
  const T* __restrict__ Ck = LLTg + (size_t)k * obs * obs;
  const unsigned full = (1u << obs) - 1u;
  const T nan = (T)__builtin_nan("");
  const T half_log_2pi = T(0.91893853320467274178);
  auto Bm = [&](int c, int a) -> T { return c < obs ? Bk[c * D + a] : T(0); };

  T m[D], Dm[D][D], tprev = T(0);
  bool have = t0 != nullptr;                       // a state to predict from (false: the prior, at the first row)
  if (have) {
    const int64_t s = k * B + b;
    tprev = t0[b];
    load_vec<T, D>(m0 + s * D, m);
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int c = 0; c <= a; ++c) Dm[a][c] = Dm[c][a] = P0[(s * D + a) * D + c] - (a == c ? T(1) : T(0));
  } else {
#pragma unroll
    for (int a = 0; a < D; ++a) {
      m[a] = T(0);
#pragma unroll
      for (int c = 0; c < D; ++c) Dm[a][c] = T(0);
    }
  }

  bool fail = false;
  double ll = 0.0;
  // what a (model, series) leaves behind.  Stored from INSIDE the walk, by the iteration of the series' last row: the
  // lanes of a wave leave the loop at different rows, and nothing a lane carries is read after it has left
  const int64_t slot = k * B + b;
  auto store_end = [&]() {
    loglik[slot] = fail ? __builtin_nan("") : ll;
#pragma unroll
    for (int a = 0; a < D; ++a) {
      m_end[slot * D + a] = fail ? nan : m[a];
#pragma unroll
      for (int c = 0; c < D; ++c) P_end[(slot * D + a) * D + c] = fail ? nan : Dm[a][c] + (a == c ? T(1) : T(0));
    }
  };
  if (r1 <= r0) store_end();                       // (a series without rows: the state it started from)
  for (int64_t i = r0; i < r1; ++i) {
    const int64_t row = k * R + i;
    if (!fail) {
      // ---- predict across the gap
      const T t = ts[i];
      if (have) {
        const T dt = t - tprev;
        fail = !(dt >= T(0)) || !finiteT(dt);
        T E[D][D];
        if (i > r0) {                              // (leg_filter_gaps_kernel left it in the slot this row's z_cov goes to)
#pragma unroll
          for (int a = 0; a < D; ++a) load_vec<T, D>(z_cov + (row * D + a) * D, E[a]);
        } else {                                   // the gap from t0 to the first row
          gap_expm1<T, D>(fail ? T(0) : dt, [&](int a, int c) { return Gk[a * D + c]; }, E);
          add_identity<T, D>(E);
        }
        {
          T ED[D][D];
          mat_mul<T, D>(ED, E, Dm);
#pragma unroll
          for (int a = 0; a < D; ++a)
#pragma unroll
            for (int c = 0; c <= a; ++c) {
              T s = T(0);
#pragma unroll
              for (int q = 0; q < D; ++q) s = fmaT(ED[a][q], E[c][q], s);
              Dm[a][c] = Dm[c][a] = s;
            }
        }
        T mp[D];
#pragma unroll
        for (int a = 0; a < D; ++a) {
          T s = T(0);
#pragma unroll
          for (int q = 0; q < D; ++q) s = fmaT(E[a][q], m[q], s);
          mp[a] = s;
        }
#pragma unroll
        for (int a = 0; a < D; ++a) m[a] = mp[a];
      }
      have = true;
      tprev = t;

      // ---- the row's observation
      const unsigned p = pattern != nullptr ? ((unsigned)pattern[i] & full) : full;
      bool on[O];
      T x[O], s[O];
#pragma unroll
      for (int c = 0; c < O; ++c) {
        on[c] = (p >> c) & 1u;                     // (false for every c >= obs)
        x[c] = on[c] ? xs[i * obs + c] : T(0);
        s[c] = (on[c] && noise != nullptr) ? noise[i * obs + c] : T(0);
      }
      T bp[O][D], pm[O], pc[O][O];                 // Bm P^-, Bm m^-, the predictive covariance of all channels
#pragma unroll
      for (int c = 0; c < O; ++c) {
        T r = T(0);
#pragma unroll
        for (int a = 0; a < D; ++a) {
          T u = Bm(c, a);
#pragma unroll
          for (int q = 0; q < D; ++q) u = fmaT(Bm(c, q), Dm[q][a], u);
          bp[c][a] = u;
          r = fmaT(Bm(c, a), m[a], r);
        }
        pm[c] = r;
      }
      Chol<T, O> Tw;
      {
        T W[O][O];
#pragma unroll
        for (int c = 0; c < O; ++c)
#pragma unroll
          for (int q = 0; q <= c; ++q) {
            T u = (c < obs && q < obs) ? Ck[c * obs + q] : T(0);
#pragma unroll
            for (int a = 0; a < D; ++a) u = fmaT(bp[c][a], Bm(q, a), u);
            if (c == q) u += s[c];
            pc[c][q] = pc[q][c] = u;
            W[c][q] = W[q][c] = (on[c] && on[q]) ? u : (c == q ? T(1) : T(0));
          }
        chol_lower<T, O>(W, Tw, fail);
      }
      T e[O];
#pragma unroll
      for (int c = 0; c < O; ++c) e[c] = on[c] ? x[c] - pm[c] : T(0);
      fwd_subst<T, O>(Tw, e);                      // T^-1 e
      T quad = T(0), slog = T(0);
      int cnt = 0;
#pragma unroll
      for (int c = 0; c < O; ++c) {
        quad = fmaT(e[c], e[c], quad);
        slog += on[c] ? logT(Tw.l[c][c]) : T(0);
        cnt += on[c] ? 1 : 0;
      }
      const T lp = cnt == 0 ? T(0) : T(-0.5) * quad - slog - T(cnt) * half_log_2pi;

      // ---- update:  V = T^-1 Bm_o P^-  (column a of V is Vt[a])
      T chk = lp;
      {
        T Vt[D][O];
#pragma unroll
        for (int a = 0; a < D; ++a) {
#pragma unroll
          for (int c = 0; c < O; ++c) Vt[a][c] = on[c] ? bp[c][a] : T(0);
          fwd_subst<T, O>(Tw, Vt[a]);
        }
#pragma unroll
        for (int a = 0; a < D; ++a) {
          T u = m[a];
#pragma unroll
          for (int c = 0; c < O; ++c) u = fmaT(Vt[a][c], e[c], u);
          m[a] = u;
          chk += u;
#pragma unroll
          for (int q = 0; q <= a; ++q) {
            T w = Dm[a][q];
#pragma unroll
            for (int c = 0; c < O; ++c) w = fmaT(-Vt[a][c], Vt[q][c], w);
            Dm[a][q] = Dm[q][a] = w;
            chk += w;
          }
        }
      }
#pragma unroll
      for (int c = 0; c < O; ++c) {
        chk += pm[c];
#pragma unroll
        for (int q = 0; q <= c; ++q) chk += pc[c][q];
      }
      fail = fail || !finiteT(chk);
      if (fail) report_fail(info, row);

      if (!fail) {
        ll += (double)lp;
        logpdf[row] = lp;
#pragma unroll
        for (int c = 0; c < O; ++c)
          if (c < obs) {
            pred_mean[row * obs + c] = pm[c];
#pragma unroll
            for (int q = 0; q < O; ++q)
              if (q < obs) pred_cov[(row * obs + c) * obs + q] = pc[c][q];
          }
        store_vec<T, D>(z_mean + row * D, m);
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
          for (int c = 0; c < D; ++c) z_cov[(row * D + a) * D + c] = Dm[a][c] + (a == c ? T(1) : T(0));
        if (i + 1 == r1) store_end();
        continue;
      }
    }
    // a failed row, or a row after one
    logpdf[row] = nan;
    for (int c = 0; c < obs; ++c) {
      pred_mean[row * obs + c] = nan;
      for (int q = 0; q < obs; ++q) pred_cov[(row * obs + c) * obs + q] = nan;
    }
#pragma unroll
    for (int a = 0; a < D; ++a) {
      z_mean[row * D + a] = nan;
#pragma unroll
      for (int c = 0; c < D; ++c) z_cov[(row * D + a) * D + c] = nan;
    }
    if (i + 1 == r1) store_end();
  }
}

template <typename T, int D>
void launch_filter(const T* ts, const T* xs, const unsigned char* pattern, const T* noise, const int64_t* roff, int64_t B,
                   int64_t R, int64_t M, const T* G, const T* Bm, const T* LLT, int obs, const T* t0, const T* m0,
                   const T* P0, T* pred_mean, T* pred_cov, T* logpdf, T* z_mean, T* z_cov, double* loglik, T* m_end,
                   T* P_end, int* info, hipStream_t st) {
  const dim3 grid((unsigned)((B + FILTER_THREADS - 1) / FILTER_THREADS), (unsigned)M), block(FILTER_THREADS);
  if (R > 1)
    hipLaunchKernelGGL((leg_filter_gaps_kernel<T, D>), dim3((unsigned)((R + FILTER_THREADS - 1) / FILTER_THREADS), (unsigned)M),
                       block, 0, st, ts, R, G, z_cov);
  cgps_host::dispatch_obs(obs, [&](auto oc) {
    hipLaunchKernelGGL((leg_filter_kernel<T, D, decltype(oc)::value>), grid, block, 0, st, ts, xs, pattern, noise, roff, B, R,
                       G, Bm, LLT, obs, t0, m0, P0, pred_mean, pred_cov, logpdf, z_mean, z_cov, loglik, m_end, P_end, info);
  });
}

}  // namespace cgps
