// Gradients through the LEG filter: the reverse walk of cgps_leg_filter's recursion.
//
// Conventions are those of cgps_leg_filter.h.  Row i carries the state (m, Dm) of the row before it across the gap,
// m^- = E m, Dm^- = E Dm E^T, P = I + Dm^-, and observes the channels o:  A = Bm_o,  S = A P A^T + Cn[o, o],  W = S^-1,
// e = x_o - A m^-,  alpha = W e,  K = P A^T W,  m' = m^- + K e,  Dm' = Dm^- - K S K^T.  With (mb, Db) the adjoint of
// (m', Dm') -- what row i + 1 hands back plus the row's own cotangents of z_mean and z_cov, Db symmetric --, lb the
// cotangent of logpdf, gm and Cs = sym(cotangent of cov) those of the predictive of ALL channels, sym(X) = (X + X^T) / 2:
//     h = K^T mb,   Y = K^T Db K,   eb = h - lb alpha                                          -> x_bar_o = eb
//     Sb = Y - sym(h alpha^T) + lb / 2 (alpha alpha^T - W)   on o x o, 0 elsewhere;   Sf = Sb + Cs,   ef = eb - gm
//     s_bar_c = Sf_cc on observed c,   LLT_bar += Sf
//     Db^- = Db + sym(mb (A^T alpha)^T) - 2 sym(Db K A) + Bm^T Sf Bm,    mb^- = mb - Bm^T ef
//     Bm_bar += -ef m^-^T + alpha (P mb)^T + 2 Sf Bm P - 2 K^T Db P
// (alpha, K^T and h are zero at unobserved channels, so every product above runs over all channels), and across the gap
//     mb_prev = E^T mb^-,   Db_prev = E^T Db^- E,   E_bar = mb^- m^T + 2 Db^- E Dm.
// A row that observes nothing has K = 0, alpha = 0: it passes (mb, Db) through the gap, its x_bar and s_bar are 0.
//
// Three kernels, one launch each:
//   leg_filter_adjoint_gaps_kernel     one lane per (row, model): E = I + gap_expm1(gap[i]) into slot (k, i) of the
//                                      workspace [M][R][d][d]; gap[R] is the caller's (0 at a first row without a start
//                                      state: E = I exactly), so the walking lane evaluates no exponential.
//   leg_filter_adjoint_kernel          grid, lane mapping and channel forms of leg_filter_kernel; the lane walks its rows
//                                      from last to first.  Per row it reads the previous row's saved z_mean, z_cov (the
//                                      start state at the first row), E and the row's data and cotangents, recomputes
//                                      m^-, P, the factor and K^T, applies the formulas, stores x_bar, s_bar and E_bar
//                                      OVER the E it has just read.  Bm_bar and LLT_bar of the (model, series) add up in
//                                      registers for O <= 4 and in the lane's own output slot for O = 8.  What a series
//                                      leaves behind is stored from inside the walk, by the iteration of its first row.
//   leg_filter_adjoint_frechet_kernel  one lane per (row, model): A = -1/2 gap G, A_bar = L_exp(A^T, E_bar),
//                                      G_bar += -1/2 gap A_bar summed per workgroup in a fixed order (as
//                                      peg_precision_adjoint_kernel), gap_bar = -1/2 <G, A_bar>.
// A (model, series) whose forward failed (its last row's state is not finite) gets NaN in x_bar, s_bar, E_bar of its
// rows and in its Bm_bar, LLT_bar and start-state adjoints; no other lane is touched.
#pragma once
#include "cgps_host.h"
#include "cgps_leg.h"
#include "cgps_leg_filter.h"

namespace cgps {

template <typename T, int D>
__global__ __launch_bounds__(FILTER_THREADS) void leg_filter_adjoint_gaps_kernel(const T* __restrict__ gap, int64_t R,
                                                                                 const T* __restrict__ Gg,
                                                                                 T* __restrict__ Ews) {
  const int64_t i = (int64_t)blockIdx.x * FILTER_THREADS + threadIdx.x;
  if (i >= R) return;
  const int64_t k = blockIdx.y;
  const T* __restrict__ Gk = Gg + (size_t)k * D * D;
  const T dt = gap[i];
  T E[D][D];
  gap_expm1<T, D>((dt >= T(0) && finiteT(dt)) ? dt : T(0), [&](int a, int c) { return Gk[a * D + c]; }, E);
  add_identity<T, D>(E);
  T* __restrict__ out = Ews + (k * R + i) * D * D;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int c = 0; c < D; ++c) out[a * D + c] = E[a][c];
}

template <typename T, int D, int O>
__global__ __launch_bounds__(FILTER_THREADS) void leg_filter_adjoint_kernel(
    const T* __restrict__ xs, const unsigned char* __restrict__ pattern, const T* __restrict__ noise,
    const int64_t* __restrict__ roff, int64_t B, int64_t R, const T* __restrict__ Bg, const T* __restrict__ LLTg,
    int obs_rt, const T* __restrict__ z_mean, const T* __restrict__ z_cov, const T* __restrict__ m0,
    const T* __restrict__ P0, const T* __restrict__ g_mean, const T* __restrict__ g_cov, const T* __restrict__ g_lp,
    const T* __restrict__ g_zm, const T* __restrict__ g_zc, T* Ews, T* __restrict__ x_bar, T* __restrict__ s_bar,
    T* B_bar, T* LLT_bar, T* __restrict__ m0_bar, T* __restrict__ P0_bar) {
  constexpr bool REG = O <= 4;                     // Bm_bar and LLT_bar add up in registers (else: in the output slot)
  const int obs = O <= 4 ? O : obs_rt;
  const int64_t b = (int64_t)blockIdx.x * FILTER_THREADS + threadIdx.x;
  if (b >= B) return;
  const int64_t k = blockIdx.y;
  int64_t r0 = roff[b], r1 = roff[b + 1];
  r0 = r0 < 0 ? 0 : r0;
  r1 = r1 > R ? R : r1;
  const T* __restrict__ Bk = Bg + (size_t)k * obs * D;
  const T* __restrict__ Ck = LLTg + (size_t)k * obs * obs;
  const unsigned full = (1u << obs) - 1u;
  const T nan = (T)__builtin_nan("");
  const int64_t slot = k * B + b;
  T* Bb = B_bar + slot * obs * D;
  T* Lb = LLT_bar + slot * obs * obs;
  auto Bm = [&](int c, int a) -> T { return c < obs ? Bk[c * D + a] : T(0); };

  // did the forward fail this (model, series)?  Then its last row's state is NaN
  bool bad = false;
  if (r1 > r0) {
    const int64_t last = k * R + r1 - 1;
    T chk = T(0);
#pragma unroll
    for (int a = 0; a < D; ++a) {
      chk += z_mean[last * D + a];
#pragma unroll
      for (int c = 0; c < D; ++c) chk += z_cov[(last * D + a) * D + c];
    }
    bad = !finiteT(chk);
  }
  if (bad || r1 <= r0) {                           // NaN everywhere, or (no rows) nothing to hand back
    const T v = bad ? nan : T(0);
    for (int64_t i = r0; i < r1; ++i) {
      const int64_t row = k * R + i;
      for (int c = 0; c < obs; ++c) x_bar[row * obs + c] = s_bar[row * obs + c] = v;
      for (int q = 0; q < D * D; ++q) Ews[row * D * D + q] = v;
    }
    for (int q = 0; q < obs * D; ++q) Bb[q] = v;
    for (int q = 0; q < obs * obs; ++q) Lb[q] = v;
    for (int q = 0; q < D; ++q) m0_bar[slot * D + q] = v;
    for (int q = 0; q < D * D; ++q) P0_bar[slot * D * D + q] = v;
    return;
  }

  T Bacc[REG ? O : 1][REG ? D : 1], Lacc[REG ? O : 1][REG ? O : 1];
  if constexpr (REG) {
#pragma unroll
    for (int c = 0; c < O; ++c) {
#pragma unroll
      for (int a = 0; a < D; ++a) Bacc[c][a] = T(0);
#pragma unroll
      for (int q = 0; q < O; ++q) Lacc[c][q] = T(0);
    }
  } else {
    for (int q = 0; q < obs * D; ++q) Bb[q] = T(0);
    for (int q = 0; q < obs * obs; ++q) Lb[q] = T(0);
  }

  T mb[D], Db[D][D];                               // the adjoint of the state after row i
#pragma unroll
  for (int a = 0; a < D; ++a) {
    mb[a] = T(0);
#pragma unroll
    for (int c = 0; c < D; ++c) Db[a][c] = T(0);
  }

  for (int64_t i = r1 - 1; i >= r0; --i) {
    const int64_t row = k * R + i;
    // ---- the row's own cotangents of the filtered state
    if (g_zm != nullptr) {
#pragma unroll
      for (int a = 0; a < D; ++a) mb[a] += g_zm[row * D + a];
    }
    if (g_zc != nullptr) {
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int c = 0; c <= a; ++c) {
          const T u = T(0.5) * (g_zc[(row * D + a) * D + c] + g_zc[(row * D + c) * D + a]);
          Db[a][c] += u;
          if (c != a) Db[c][a] += u;
        }
    }
    const T lb = g_lp != nullptr ? g_lp[row] : T(0);

    // ---- recompute the prediction: the state before the row, across the gap
    T E[D][D], mp[D], ED[D][D], m[D], P[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a) load_vec<T, D>(Ews + (row * D + a) * D, E[a]);
    {
      T Dp[D][D];
      if (i > r0) {
        load_vec<T, D>(z_mean + (row - 1) * D, mp);
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
          for (int c = 0; c <= a; ++c) Dp[a][c] = Dp[c][a] = z_cov[((row - 1) * D + a) * D + c] - (a == c ? T(1) : T(0));
      } else if (m0 != nullptr) {
        load_vec<T, D>(m0 + slot * D, mp);
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
          for (int c = 0; c <= a; ++c) Dp[a][c] = Dp[c][a] = P0[(slot * D + a) * D + c] - (a == c ? T(1) : T(0));
      } else {
#pragma unroll
        for (int a = 0; a < D; ++a) {
          mp[a] = T(0);
#pragma unroll
          for (int c = 0; c < D; ++c) Dp[a][c] = T(0);
        }
      }
      mat_mul<T, D>(ED, E, Dp);
    }
#pragma unroll
    for (int a = 0; a < D; ++a) {
      T s = T(0);
#pragma unroll
      for (int q = 0; q < D; ++q) s = fmaT(E[a][q], mp[q], s);
      m[a] = s;
#pragma unroll
      for (int c = 0; c <= a; ++c) {
        T u = a == c ? T(1) : T(0);
#pragma unroll
        for (int q = 0; q < D; ++q) u = fmaT(ED[a][q], E[c][q], u);
        P[a][c] = P[c][a] = u;
      }
    }

    // ---- the row's observation, its factor, alpha and K^T
    const unsigned p = pattern != nullptr ? ((unsigned)pattern[i] & full) : full;
    bool on[O];
    T al[O], bp[O][D], ef[O], Sf[O][O], DK[D][O];
#pragma unroll
    for (int c = 0; c < O; ++c) {
      on[c] = (p >> c) & 1u;
#pragma unroll
      for (int a = 0; a < D; ++a) {
        T u = T(0);
#pragma unroll
        for (int q = 0; q < D; ++q) u = fmaT(Bm(c, q), P[q][a], u);
        bp[c][a] = u;
      }
    }
    {
      // S, its factor, alpha, K^T and Sf in fp64 in BOTH precisions: lb / 2 (alpha alpha^T - W) cancels (it vanishes in
      // the mean at the maximum of the likelihood), and what it cancels against is a few obs x obs solves
      using A = double;
      A alA[O], KtA[O][D];
      Chol<A, O> Tw;
      {
        A W[O][O];
        bool f = false;
#pragma unroll
        for (int c = 0; c < O; ++c) {
          A pmc = A(0);
#pragma unroll
          for (int a = 0; a < D; ++a) pmc = fmaT((A)Bm(c, a), (A)m[a], pmc);
          alA[c] = on[c] ? (A)xs[i * obs + c] - pmc : A(0);
#pragma unroll
          for (int q = 0; q <= c; ++q) {
            A u = (c < obs && q < obs) ? (A)Ck[c * obs + q] : A(0);
#pragma unroll
            for (int a = 0; a < D; ++a) u = fmaT((A)bp[c][a], (A)Bm(q, a), u);
            if (c == q && on[c] && noise != nullptr) u += (A)noise[i * obs + c];
            W[c][q] = W[q][c] = (on[c] && on[q]) ? u : (c == q ? A(1) : A(0));
          }
        }
        chol_lower<A, O>(W, Tw, f);
      }
      fwd_subst<A, O>(Tw, alA);
      bwd_subst<A, O>(Tw, alA);
#pragma unroll
      for (int a = 0; a < D; ++a) {
        A v[O];
#pragma unroll
        for (int c = 0; c < O; ++c) v[c] = on[c] ? (A)bp[c][a] : A(0);
        fwd_subst<A, O>(Tw, v);
        bwd_subst<A, O>(Tw, v);
#pragma unroll
        for (int c = 0; c < O; ++c) KtA[c][a] = v[c];
      }

      // ---- h, Db K, Sf, ef
      A h[O], DKA[D][O];
#pragma unroll
      for (int c = 0; c < O; ++c) {
        A u = A(0);
#pragma unroll
        for (int a = 0; a < D; ++a) u = fmaT(KtA[c][a], (A)mb[a], u);
        h[c] = u;
      }
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int c = 0; c < O; ++c) {
          A u = A(0);
#pragma unroll
          for (int q = 0; q < D; ++q) u = fmaT((A)Db[a][q], KtA[c][q], u);
          DKA[a][c] = u;
          DK[a][c] = (T)u;
        }
      // W = S^-1, column by column (only the cotangent of logpdf asks for it)
      A Wi[O][O];
#pragma unroll
      for (int q = 0; q < O; ++q) {
        A v[O];
#pragma unroll
        for (int c = 0; c < O; ++c) v[c] = (c == q && lb != T(0)) ? A(1) : A(0);
        if (lb != T(0)) {
          fwd_subst<A, O>(Tw, v);
          bwd_subst<A, O>(Tw, v);
        }
#pragma unroll
        for (int c = 0; c < O; ++c) Wi[c][q] = v[c];
      }
#pragma unroll
      for (int c = 0; c < O; ++c) {
        const A eb = on[c] ? h[c] - (A)lb * alA[c] : A(0);
        if (c < obs) x_bar[row * obs + c] = (T)eb;
        ef[c] = (T)(eb - ((g_mean != nullptr && c < obs) ? (A)g_mean[row * obs + c] : A(0)));
        al[c] = (T)alA[c];
#pragma unroll
        for (int q = 0; q <= c; ++q) {
          A u = A(0);
          if (on[c] && on[q]) {
#pragma unroll
            for (int a = 0; a < D; ++a) u = fmaT(KtA[c][a], DKA[a][q], u);
            u -= A(0.5) * (h[c] * alA[q] + h[q] * alA[c]);
            u += A(0.5) * (A)lb * (alA[c] * alA[q] - Wi[c][q]);
          }
          if (g_cov != nullptr && c < obs && q < obs)
            u += A(0.5) * ((A)g_cov[(row * obs + c) * obs + q] + (A)g_cov[(row * obs + q) * obs + c]);
          Sf[c][q] = Sf[q][c] = (T)u;
        }
        if (c < obs) s_bar[row * obs + c] = on[c] ? Sf[c][c] : T(0);
      }
    }

    // ---- Bm_bar, LLT_bar
    {
      T Pmb[D];
#pragma unroll
      for (int a = 0; a < D; ++a) {
        T u = T(0);
#pragma unroll
        for (int q = 0; q < D; ++q) u = fmaT(P[a][q], mb[q], u);
        Pmb[a] = u;
      }
#pragma unroll
      for (int c = 0; c < O; ++c) {
#pragma unroll
        for (int a = 0; a < D; ++a) {
          T u = fmaT(al[c], Pmb[a], -ef[c] * m[a]);
#pragma unroll
          for (int q = 0; q < O; ++q) u = fmaT(T(2) * Sf[c][q], bp[q][a], u);
#pragma unroll
          for (int q = 0; q < D; ++q) u = fmaT(T(-2) * DK[q][c], P[q][a], u);
          if constexpr (REG) Bacc[c][a] += u;
          else if (c < obs) Bb[c * D + a] += u;
        }
#pragma unroll
        for (int q = 0; q < O; ++q) {
          if constexpr (REG) Lacc[c][q] += Sf[c][q];
          else if (c < obs && q < obs) Lb[c * obs + q] += Sf[c][q];
        }
      }
    }

    // ---- the adjoint of the predicted state:  mb^- (in mb), Db^- (in Db)
    {
      T w[D], SB[O][D];
#pragma unroll
      for (int a = 0; a < D; ++a) {
        T u = T(0);
#pragma unroll
        for (int c = 0; c < O; ++c) u = fmaT(al[c], Bm(c, a), u);
        w[a] = u;
      }
#pragma unroll
      for (int c = 0; c < O; ++c)
#pragma unroll
        for (int a = 0; a < D; ++a) {
          T u = T(0);
#pragma unroll
          for (int q = 0; q < O; ++q) u = fmaT(Sf[c][q], Bm(q, a), u);
          SB[c][a] = u;
        }
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int c = 0; c <= a; ++c) {
          T u = Db[a][c] + T(0.5) * (mb[a] * w[c] + mb[c] * w[a]);
#pragma unroll
          for (int q = 0; q < O; ++q) {
            u = fmaT(-DK[a][q], Bm(q, c), u);
            u = fmaT(-DK[c][q], Bm(q, a), u);
            u = fmaT(Bm(q, a), SB[q][c], u);
          }
          Db[a][c] = Db[c][a] = u;
        }
#pragma unroll
      for (int a = 0; a < D; ++a) {
        T u = mb[a];
#pragma unroll
        for (int c = 0; c < O; ++c) u = fmaT(-Bm(c, a), ef[c], u);
        mb[a] = u;
      }
    }

    // ---- across the gap:  E_bar = mb^- m_prev^T + 2 Db^- (E Dm_prev)  over E's slot;  (mb, Db) <- (E^T mb^-, E^T Db^- E)
    {
      T* out = Ews + row * D * D;
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int c = 0; c < D; ++c) {
          T u = mb[a] * mp[c];
#pragma unroll
          for (int q = 0; q < D; ++q) u = fmaT(T(2) * Db[a][q], ED[q][c], u);
          out[a * D + c] = u;
        }
      T DE[D][D], mn[D];
      mat_mul<T, D>(DE, Db, E);
#pragma unroll
      for (int a = 0; a < D; ++a) {
        T s = T(0);
#pragma unroll
        for (int q = 0; q < D; ++q) s = fmaT(E[q][a], mb[q], s);
        mn[a] = s;
      }
#pragma unroll
      for (int a = 0; a < D; ++a) {
        mb[a] = mn[a];
#pragma unroll
        for (int c = 0; c <= a; ++c) {
          T u = T(0);
#pragma unroll
          for (int q = 0; q < D; ++q) u = fmaT(E[q][a], DE[q][c], u);
          Db[a][c] = u;
        }
      }
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int c = 0; c < a; ++c) Db[c][a] = Db[a][c];
    }

    if (i == r0) {                                 // what the (model, series) leaves behind
#pragma unroll
      for (int a = 0; a < D; ++a) {
        m0_bar[slot * D + a] = mb[a];
#pragma unroll
        for (int c = 0; c < D; ++c) P0_bar[(slot * D + a) * D + c] = Db[a][c];
      }
      if constexpr (REG) {
#pragma unroll
        for (int c = 0; c < O; ++c) {
#pragma unroll
          for (int a = 0; a < D; ++a) Bb[c * D + a] = Bacc[c][a];
#pragma unroll
          for (int q = 0; q < O; ++q) Lb[c * O + q] = Lacc[c][q];
        }
      }
    }
  }
}

// G_bar partial sums [M][gridDim.x][d][d] and gap_bar [M][R] from E_bar [M][R][d][d]
template <typename T, int D>
__global__ __launch_bounds__(FILTER_THREADS) void leg_filter_adjoint_frechet_kernel(
    const T* __restrict__ gap, int64_t R, const T* __restrict__ Gg, const T* __restrict__ Ebar_g,
    T* __restrict__ gG_partial, T* __restrict__ g_gap) {
  constexpr int DD = D * D;
  __shared__ T red[DD];
  const int64_t i = (int64_t)blockIdx.x * FILTER_THREADS + threadIdx.x;
  const int64_t k = blockIdx.y;
  const T* __restrict__ Gk = Gg + (size_t)k * DD;
  T Gbar[D][D];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int c = 0; c < D; ++c) Gbar[a][c] = T(0);
  if (i < R) {
    const T dt0 = gap[i];
    const T dt = (dt0 >= T(0) && finiteT(dt0)) ? dt0 : T(0);
    T At[D][D], Ebar[D][D], Ex[D][D], Abar[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int c = 0; c < D; ++c) {
        At[a][c] = T(-0.5) * dt * Gk[c * D + a];
        Ebar[a][c] = Ebar_g[(k * R + i) * DD + a * D + c];
      }
    mat_exp_frechet<T, D>(Ex, Abar, At, Ebar);
    T tb = T(0);
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int c = 0; c < D; ++c) {
        Gbar[a][c] = T(-0.5) * dt * Abar[a][c];
        tb = fmaT(Abar[a][c], Gk[a * D + c], tb);
      }
    g_gap[k * R + i] = T(-0.5) * tb;
  }
  // sum over the wave (FILTER_THREADS = 64: one wave per workgroup), fixed order
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int c = 0; c < D; ++c) {
      T v = Gbar[a][c];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if (threadIdx.x == 0) red[a * D + c] = v;
    }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < DD; ++q) gG_partial[((size_t)k * gridDim.x + blockIdx.x) * DD + q] = red[q];
  }
}

template <typename T, int D>
void launch_filter_adjoint(const T* xs, const unsigned char* pattern, const T* noise, const int64_t* roff, int64_t B,
                           int64_t R, int64_t M, const T* G, const T* Bm, const T* LLT, int obs, const T* gap,
                           const T* z_mean, const T* z_cov, const T* m0, const T* P0, const T* g_mean, const T* g_cov,
                           const T* g_lp, const T* g_zm, const T* g_zc, T* Ews, T* x_bar, T* s_bar, T* B_bar, T* LLT_bar,
                           T* m0_bar, T* P0_bar, T* gG_partial, T* g_gap, hipStream_t st) {
  const dim3 rows((unsigned)((R + FILTER_THREADS - 1) / FILTER_THREADS), (unsigned)M), block(FILTER_THREADS);
  const dim3 grid((unsigned)((B + FILTER_THREADS - 1) / FILTER_THREADS), (unsigned)M);
  hipLaunchKernelGGL((leg_filter_adjoint_gaps_kernel<T, D>), rows, block, 0, st, gap, R, G, Ews);
  cgps_host::dispatch_obs(obs, [&](auto oc) {
    hipLaunchKernelGGL((leg_filter_adjoint_kernel<T, D, decltype(oc)::value>), grid, block, 0, st, xs, pattern, noise, roff,
                       B, R, Bm, LLT, obs, z_mean, z_cov, m0, P0, g_mean, g_cov, g_lp, g_zm, g_zc, Ews, x_bar, s_bar, B_bar,
                       LLT_bar, m0_bar, P0_bar);
  });
  hipLaunchKernelGGL((leg_filter_adjoint_frechet_kernel<T, D>), rows, block, 0, st, gap, R, G, (const T*)Ews, gG_partial,
                     g_gap);
}

}  // namespace cgps
