// One damped Newton step of the Laplace approximation for count, binary and Gaussian observations under a LEG prior
// (cgps_leg_glm_step, include/cgps_glm.h).
//
// One workgroup of ONE wave per series: its 64 lanes stride the series' rows and every sum is a shuffle tree over the
// wave, a fixed order, so a series' step depends on nothing else in the batch (the contract of cgps_leg_loglik_batch).
//
//   pass 1  delta = prop - z.  The prior quadratic form along the line needs three sums,
//             a = z^T K z,  b = z^T K delta,  c = delta^T K delta,
//           and the likelihood one sum per candidate: sum_ic [l(eta + alpha dEta) - l(eta)] for alpha = 1, 1/2, ..,
//           2^-(GLM_CANDIDATES - 1), each difference written so that nothing of the size of l itself cancels
//           (Poisson: y t - e^eta expm1(t); Bernoulli: y' t' - log1p(m expm1(t')) with m = sigma(-|eta|) <= 1/2 and
//           (y', t') = (y, t) at eta <= 0, (1 - y, -t) at eta > 0; Gaussian: a polynomial in t).
//           gain(alpha) = that sum - alpha b - alpha^2 c / 2 is the objective's change, in fp64 in both precisions.
//           A candidate whose gain is NaN or infinite (e^eta overflowed) fails `gain >= 0` and is rejected.
//   choose  the largest alpha with a finite gain >= 0.  None: the series keeps z; by concavity no step along delta gains
//           more than |grad psi . delta|, so below the tolerance that is convergence, above it the series has stalled.
//   pass 2  z_out = z + alpha delta (prop itself at alpha = 1), and at z_out: J_Rs = Rs + B^T W B, rhs = B^T (W B z + g),
//           the log-likelihood sum, hence psi = sum - (a + 2 alpha b + alpha^2 c) / 2.
// A series that has converged or stalled is frozen: prop is not read for it, z_out = z, its state is copied, and J_Rs
// and rhs are written again at the same z (every output element is written by every call).
#pragma once
#include "cgps_math.h"

namespace cgps {

constexpr int GLM_THREADS = 64;
constexpr int GLM_CANDIDATES = 12;       // alpha = 1 .. 2^-11 (what Poisson counts of 1000 from z = 0 need)
constexpr int GLM_STATE = 4;             // doubles per series: psi, iterations, flags, the accepted alpha
enum { GLM_POISSON = 0, GLM_BERNOULLI = 1, GLM_GAUSSIAN = 2 };
enum { GLM_CONVERGED = 1, GLM_STALLED = 2 };

__device__ __forceinline__ float glm_exp(float x) { return expf(x); }
__device__ __forceinline__ double glm_exp(double x) { return exp(x); }
__device__ __forceinline__ float glm_expm1(float x) { return expm1f(x); }
__device__ __forceinline__ double glm_expm1(double x) { return expm1(x); }
__device__ __forceinline__ float glm_log1p(float x) { return log1pf(x); }
__device__ __forceinline__ double glm_log1p(double x) { return log1p(x); }
__device__ __forceinline__ float glm_log(float x) { return logf(x); }
__device__ __forceinline__ double glm_log(double x) { return log(x); }
__device__ __forceinline__ float glm_abs(float x) { return fabsf(x); }
__device__ __forceinline__ double glm_abs(double x) { return fabs(x); }

// the sum over the wave, in every lane (the same shuffle tree whatever the data: a fixed order)
__device__ __forceinline__ double glm_wave_all(double v) { return __shfl(wave_sum(v), 0, 64); }

// What a family needs of one entry at the linear predictor eta: the log density l (without lgamma(y + 1)), its
// derivative g, the weight w = -l'' >= 0, and `base`, the factor of the line difference (diff below); `up`: Bernoulli
// with eta > 0, where the difference is taken on the mirror image l(eta; y) = l(-eta; 1 - y).
template <typename T>
struct GlmPoint {
  T l, g, w, base;
  bool up;
};

template <typename T>
__device__ __forceinline__ GlmPoint<T> glm_point(int family, T y, T eta, T s) {
  GlmPoint<T> p;
  p.up = false;
  if (family == GLM_POISSON) {
    const T e = glm_exp(eta);
    p.l = y * eta - e;
    p.g = y - e;
    p.w = e;
    p.base = e;
  } else if (family == GLM_BERNOULLI) {
    const T e = glm_exp(-glm_abs(eta));                     // in (0, 1]: nothing overflows
    const T r = T(1) / (T(1) + e);
    const T sig = eta >= T(0) ? r : e * r;                  // sigma(eta)
    p.l = y * eta - ((eta > T(0) ? eta : T(0)) + glm_log1p(e));
    p.g = y - sig;
    p.w = e * r * r;                                        // sigma (1 - sigma)
    p.base = e * r;                                         // sigma(-|eta|): sigma at eta <= 0, 1 - sigma at eta > 0
    p.up = eta > T(0);
  } else {
    const T is = T(1) / s, res = y - eta;
    p.l = T(-0.5) * res * res * is - T(0.5) * glm_log(T(6.283185307179586476925) * s);
    p.g = res * is;
    p.w = is;
    p.base = is;
  }
  return p;
}

// l(eta + t) - l(eta) from the point at eta; +-inf or NaN where e^t overflows.
// Bernoulli: softplus(eta + t) - softplus(eta) = log1p(sigma(eta) expm1(t)), but 1 + sigma expm1(t) = (1 - sigma) + sigma e^t
// is then formed from two numbers that have each been rounded to about 1 when eta >> 0 and t << 0 (at eta = 18, t = -20
// in fp32 it rounds to 0 and the difference to +inf).  So the line is always walked from the side on which sigma <= 1/2:
// at eta > 0 on the mirror image (-eta, -t, 1 - y), which is the same function.  Then m <= 1/2 and expm1 >= -1 put the
// argument of log1p at or above -1/2, nothing cancels, and a data set and its mirror image take bit-equal differences.
template <typename T>
__device__ __forceinline__ T glm_diff(int family, T y, const GlmPoint<T>& p, T t) {
  if (family == GLM_POISSON) return y * t - p.base * glm_expm1(t);
  if (family == GLM_BERNOULLI) {
    const T ym = p.up ? T(1) - y : y, tm = p.up ? -t : t;
    return ym * tm - glm_log1p(p.base * glm_expm1(tm));
  }
  return t * (p.g - T(0.5) * t * p.base);
}

template <typename T, int D, int O>
__global__ __launch_bounds__(GLM_THREADS) void leg_glm_step_kernel(
    const T* __restrict__ z, const T* __restrict__ prop, const T* __restrict__ Rs, const T* __restrict__ Os,
    const T* __restrict__ ys, const unsigned char* __restrict__ pattern, const T* __restrict__ offset,
    const T* __restrict__ extra, const T* __restrict__ Bg, const int64_t* __restrict__ offsets, int64_t R, int obs_rt,
    int family, double tol, const double* __restrict__ state_in, T* __restrict__ z_out, T* __restrict__ J_Rs,
    T* __restrict__ rhs, double* __restrict__ state_out) {
  const int obs = O <= 4 ? O : obs_rt;
  const int64_t b = blockIdx.x;
  int64_t r0 = offsets[b], r1 = offsets[b + 1];
  r0 = r0 < 0 ? 0 : r0;
  r1 = r1 > R ? R : r1;                              // (offsets that do not fit R rows: nothing outside is touched)
  const int lane = threadIdx.x;
  const unsigned full = (1u << obs) - 1u;

  double psi = 0.0, iters = 0.0;
  int flags = 0;
  if (prop != nullptr) {
    psi = state_in[b * GLM_STATE + 0];
    iters = state_in[b * GLM_STATE + 1];
    flags = (int)state_in[b * GLM_STATE + 2];
  }
  const bool active = prop != nullptr && (flags & (GLM_CONVERGED | GLM_STALLED)) == 0;

  // ---- pass 1: the three sums of the prior, the candidates' likelihood differences --------------------------------
  double qa = 0.0, qb = 0.0, qc = 0.0, gd = 0.0, dL[GLM_CANDIDATES];
#pragma unroll
  for (int k = 0; k < GLM_CANDIDATES; ++k) dL[k] = 0.0;
  for (int64_t i = r0 + lane; i < r1; i += GLM_THREADS) {
    const bool next = i + 1 < r1;
    T zi[D], di[D], zn[D], dn[D];
    load_vec<T, D>(z + i * D, zi);
#pragma unroll
    for (int a = 0; a < D; ++a) di[a] = active ? prop[i * D + a] - zi[a] : T(0);
#pragma unroll
    for (int a = 0; a < D; ++a) {
      zn[a] = next ? z[(i + 1) * D + a] : T(0);
      dn[a] = (next && active) ? prop[(i + 1) * D + a] - zn[a] : T(0);
    }
    T zRz = T(0), zRd = T(0), dRd = T(0), nOz = T(0), nOd = T(0), mOz = T(0), mOd = T(0);
#pragma unroll
    for (int a = 0; a < D; ++a) {
      T row[D], rz = T(0), rd = T(0);
      load_vec<T, D>(Rs + (i * D + a) * D, row);
#pragma unroll
      for (int k = 0; k < D; ++k) {
        rz = fmaT(row[k], zi[k], rz);
        rd = fmaT(row[k], di[k], rd);
      }
      zRz = fmaT(zi[a], rz, zRz);
      zRd = fmaT(zi[a], rd, zRd);
      dRd = fmaT(di[a], rd, dRd);
    }
    if (next) {                                      // O_i = K[i + 1][i]
#pragma unroll
      for (int a = 0; a < D; ++a) {
        T row[D], oz = T(0), od = T(0);
        load_vec<T, D>(Os + (i * D + a) * D, row);
#pragma unroll
        for (int k = 0; k < D; ++k) {
          oz = fmaT(row[k], zi[k], oz);
          od = fmaT(row[k], di[k], od);
        }
        nOz = fmaT(zn[a], oz, nOz);
        nOd = fmaT(zn[a], od, nOd);
        mOz = fmaT(dn[a], oz, mOz);
        mOd = fmaT(dn[a], od, mOd);
      }
    }
    qa += (double)zRz + 2.0 * (double)nOz;
    qb += (double)zRd + (double)nOd + (double)mOz;
    qc += (double)dRd + 2.0 * (double)mOd;
    if (active) {
      const unsigned p = pattern != nullptr ? ((unsigned)pattern[i] & full) : full;
#pragma unroll
      for (int c = 0; c < O; ++c) {
        if (c < obs && ((p >> c) & 1u)) {
          T eta = offset != nullptr ? offset[c] : T(0), de = T(0);
#pragma unroll
          for (int a = 0; a < D; ++a) {
            eta = fmaT(Bg[c * D + a], zi[a], eta);
            de = fmaT(Bg[c * D + a], di[a], de);
          }
          T s = T(1);
          if (family == GLM_GAUSSIAN) s = extra[i * obs + c];
          else if (extra != nullptr) eta += extra[i * obs + c];
          const T y = ys[i * obs + c];
          const GlmPoint<T> pt = glm_point<T>(family, y, eta, s);
          gd += (double)(pt.g * de);
          T t = de;
#pragma unroll
          for (int k = 0; k < GLM_CANDIDATES; ++k) {
            dL[k] += (double)glm_diff<T>(family, y, pt, t);
            t *= T(0.5);
          }
        }
      }
    }
  }
  qa = glm_wave_all(qa);
  double alpha = 0.0, gain = 0.0;
  bool found = false;
  if (active) {                                      // (uniform over the wave)
    qb = glm_wave_all(qb);
    qc = glm_wave_all(qc);
    gd = glm_wave_all(gd);
    double ak = 1.0;
#pragma unroll
    for (int k = 0; k < GLM_CANDIDATES; ++k) {
      const double gk = glm_wave_all(dL[k]) - ak * qb - 0.5 * ak * ak * qc;
      if (!found && gk >= 0.0 && gk <= 1.79769313486231570815e308) {   // (a NaN fails both comparisons)
        found = true;
        alpha = ak;
        gain = gk;
      }
      ak *= 0.5;
    }
  }

  // ---- pass 2: the step, and the Newton system at the new point -----------------------------------------------------
  const T aT = (T)alpha;                             // (a power of two: exact in both precisions)
  double L = 0.0;
  for (int64_t i = r0 + lane; i < r1; i += GLM_THREADS) {
    T zi[D];
    load_vec<T, D>(z + i * D, zi);
    if (alpha == 1.0) {
      load_vec<T, D>(prop + i * D, zi);
    } else if (alpha != 0.0) {
#pragma unroll
      for (int a = 0; a < D; ++a) zi[a] = fmaT(aT, prop[i * D + a] - zi[a], zi[a]);
    }
    store_vec<T, D>(z_out + i * D, zi);
    const unsigned p = pattern != nullptr ? ((unsigned)pattern[i] & full) : full;
    T w[O], u[O];                                    // u = w (B z) + g
#pragma unroll
    for (int c = 0; c < O; ++c) {
      w[c] = T(0);
      u[c] = T(0);
      if (c < obs && ((p >> c) & 1u)) {
        T bz = T(0);
#pragma unroll
        for (int a = 0; a < D; ++a) bz = fmaT(Bg[c * D + a], zi[a], bz);
        T eta = bz + (offset != nullptr ? offset[c] : T(0));
        T s = T(1);
        if (family == GLM_GAUSSIAN) s = extra[i * obs + c];
        else if (extra != nullptr) eta += extra[i * obs + c];
        const GlmPoint<T> pt = glm_point<T>(family, ys[i * obs + c], eta, s);
        L += (double)pt.l;
        w[c] = pt.w;
        u[c] = fmaT(pt.w, bz, pt.g);
      }
    }
    T r[D];
#pragma unroll
    for (int a = 0; a < D; ++a) {
      T row[D], ra = T(0);
      load_vec<T, D>(Rs + (i * D + a) * D, row);
#pragma unroll
      for (int c = 0; c < O; ++c) {
        if (c < obs) {                               // (w = u = 0 at an unobserved entry: the products add nothing)
          const T wb = w[c] * Bg[c * D + a];
#pragma unroll
          for (int k = 0; k < D; ++k) row[k] = fmaT(wb, Bg[c * D + k], row[k]);
          ra = fmaT(Bg[c * D + a], u[c], ra);
        }
      }
      store_vec<T, D>(J_Rs + (i * D + a) * D, row);
      r[a] = ra;
    }
    store_vec<T, D>(rhs + i * D, r);
  }
  L = glm_wave_all(L);
  if (lane == 0) {
    double* so = state_out + b * GLM_STATE;
    if (prop != nullptr && !active) {                // frozen: as it was
      so[0] = psi;
      so[1] = iters;
      so[2] = (double)flags;
      so[3] = state_in[b * GLM_STATE + 3];
    } else {
      const double psi_new = L - 0.5 * (qa + 2.0 * alpha * qb + alpha * alpha * qc);
      int f = 0;
      if (active) {
        const double bound = tol * (1.0 + fabs(psi_new));
        if (found) f = gain <= bound ? GLM_CONVERGED : 0;
        else f = fabs(gd - qb) <= bound ? GLM_CONVERGED : GLM_STALLED;
      }
      so[0] = psi_new;
      so[1] = active ? iters + 1.0 : 0.0;
      so[2] = (double)f;
      so[3] = alpha;
    }
  }
}

template <typename T, int D>
void launch_glm_step(const T* z, const T* prop, const T* Rs, const T* Os, const T* ys, const unsigned char* pattern,
                     const T* offset, const T* extra, const T* Bm, const int64_t* offsets, int64_t B, int64_t R, int obs,
                     int family, double tol, const double* state_in, T* z_out, T* J_Rs, T* rhs, double* state_out,
                     hipStream_t st) {
  cgps_host::dispatch_obs(obs, [&](auto oc) {
    hipLaunchKernelGGL((leg_glm_step_kernel<T, D, decltype(oc)::value>), dim3((unsigned)B), dim3(GLM_THREADS), 0, st, z, prop,
                       Rs, Os, ys, pattern, offset, extra, Bm, offsets, R, obs, family, tol, state_in, z_out, J_Rs, rhs,
                       state_out);
  });
}

}  // namespace cgps
