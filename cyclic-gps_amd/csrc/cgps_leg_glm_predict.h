// Predictions on the response scale from a latent Gaussian (cgps_leg_glm_predict: include/cgps_glm_predict.h).
//
// Per entry (k, c): mu = B_c m_k + offset_c + log_exposure_kc and v = max(B_c S_k B_c^T, 0) in the arrays' precision,
// then in fp64 the moments of y and log I(y) = log of the integral of p(y | eta) N(eta; mu, v):
//   Gaussian   mean = mu, var = v + s, log I = -1/2 (y - mu)^2 / (v + s) - 1/2 log(2 pi (v + s))
//   Poisson    mean = exp(mu + v / 2), var = mean + mean^2 expm1(v), log I by the rule
//   Bernoulli  L1 = log I(1), L0 = log I(0) by the rule; mean = exp(L1), var = exp(L1 + L0) (never p (1 - p): that
//              loses every digit near certainty)
// The rule (glm_log_integral) is adaptive Gauss-Hermite in the standardised variable u, eta(u) = mu + sqrt(v) u,
// h(u) = l(y, eta(u)) - u^2 / 2: GLM_PREDICT_NEWTON clipped Newton steps from u = 0 to the centre u*, the scale
// s = (1 + v w(eta(u*)))^(-1/2), and log I = log s + logsumexp_i [log(w_i / sqrt(pi)) + x_i^2 + h(u* + sqrt(2) s x_i)]
// over the GLM_PREDICT_NODES physicists' nodes.  The sum is taken relative to h(u*): term i is
//     c_i + (l_i - l*) - delta_i (u* + delta_i / 2),   delta_i = sqrt(2) s x_i,   c_i = log(w_i / sqrt(pi)) + x_i^2,
// which is what is left of x_i^2 + h(u_i) - h(u*) once the squares are multiplied out.  h is concave, so at a converged
// centre no term exceeds c_i <= 0: one pass, nothing overflows.
//
// leg_glm_predict_kernel: grid ceil(P obs / GLM_PREDICT_THREADS), one lane per (row, channel), everything in registers,
// nothing shared between lanes.  A row of S is consumed as it is loaded, so a lane holds 2 D values of its operands
// whatever the rank.  Every loop has a compile-time trip count: NaN in gives NaN out.
#pragma once
#include "cgps_leg_glm.h"

namespace cgps {

constexpr int GLM_PREDICT_THREADS = 256;
constexpr int GLM_PREDICT_NEWTON = 12;
constexpr int GLM_PREDICT_NODES = 32;

// the positive half of the 32 physicists' Gauss-Hermite nodes x_i (the rule is symmetric), their weights w_i, and
// c_i = log(w_i / sqrt(pi)) + x_i^2 (formed at 60 digits, so that nothing cancels at run time)
__device__ const double GLM_GH_X[GLM_PREDICT_NODES / 2] = {
    0.19484074156939933, 0.58497876543593245, 0.97650046358968284, 1.3703764109528718,
    1.7676541094632016,  2.1694991836061122,  2.5772495377323175,  2.9924908250023742,
    3.4171674928185707,  3.8537554854714446,  4.3055479533511984,  4.7771645035025964,
    5.2755509865158801,  5.8122259495159138,  6.4094981492696604,  7.1258139098307276};
// w_i: 0.37523835259280239, 0.2774581423025299, 0.15126973407664248, 0.060458130955912614, 0.01755342883157343,
//      0.0036548903266544281, 0.00053626836552797205, 5.4165840618199826e-5, 3.6505851295623761e-6,
//      1.574167792545594e-7, 4.0988321647708966e-9, 5.9332914633966386e-11, 4.2150102113264476e-13,
//      1.1973440170928487e-15, 9.2317365365182922e-19, 7.3106764273841624e-23
__device__ const double GLM_GH_C[GLM_PREDICT_NODES / 2] = {
    -1.5145958763594943, -1.5122499826361202, -1.507502504881913,  -1.5002376390668201,
    -1.4902698653576023, -1.4773274278750061, -1.4610256034209449, -1.4408237003057275,
    -1.4159543626976631, -1.3853025051344199, -1.3471855059889207, -1.298921160459867,
    -1.2358809264517319, -1.1490650649154518, -1.0171680130339496, -0.76526240024416115};

// l(y, eta) without lgamma(y + 1).  Bernoulli: y eta - softplus(eta) as (y - [eta > 0]) eta - log1p(e^-|eta|): the same
// number, and exact where y eta and max(eta, 0) cancel (y = 1, eta >> 0), so an entry and its mirror image (1 - y, -eta)
// take bit-equal values.
template <int FAM>
__device__ __forceinline__ double glm_predict_l(double y, double eta) {
  if (FAM == GLM_POISSON) return y * eta - exp(eta);
  return (y - (eta > 0.0 ? 1.0 : 0.0)) * eta - log1p(exp(-fabs(eta)));
}

// l, g = dl / d eta and w = -d^2 l / d eta^2.  Bernoulli: g = y - sigma as (y - [eta > 0]) -+ sigma(-|eta|)
template <int FAM>
__device__ __forceinline__ void glm_predict_point(double y, double eta, double& l, double& g, double& w) {
  if (FAM == GLM_POISSON) {
    const double e = exp(eta);
    l = y * eta - e;
    g = y - e;
    w = e;
  } else {
    const double e = exp(-fabs(eta)), r = 1.0 / (1.0 + e), m = e * r;      // m = sigma(-|eta|) <= 1/2
    const double up = eta > 0.0 ? 1.0 : 0.0;
    l = (y - up) * eta - log1p(e);
    g = (y - up) + (eta > 0.0 ? m : -m);
    w = m * r;
  }
}

// log of the integral of exp(l(y, eta)) N(eta; mu, v) over eta, v >= 0; Poisson without its -lgamma(y + 1)
template <int FAM>
__device__ __forceinline__ double glm_log_integral(double y, double mu, double v) {
  const double sv = sqrt(v);
  const double cap = 1.0 / sv;                             // (inf at v = 0: the clip is never taken)
  double u = 0.0, l, g, w;
#pragma unroll 1
  for (int it = 0; it < GLM_PREDICT_NEWTON; ++it) {
    glm_predict_point<FAM>(y, fma(sv, u, mu), l, g, w);
    const double step = (sv * g - u) / fma(v, w, 1.0);
    u += step > cap ? cap : step;                          // (a NaN step fails the comparison and stays NaN)
  }
  glm_predict_point<FAM>(y, fma(sv, u, mu), l, g, w);
  const double s = 1.0 / sqrt(fma(v, w, 1.0));
  const double r2s = 1.41421356237309504880 * s;
  double sum = 0.0;
#pragma unroll 1
  for (int i = 0; i < GLM_PREDICT_NODES / 2; ++i) {
    const double dl = r2s * GLM_GH_X[i], c = GLM_GH_C[i];
    const double lp = glm_predict_l<FAM>(y, fma(sv, u + dl, mu)), lm = glm_predict_l<FAM>(y, fma(sv, u - dl, mu));
    sum += exp(c + (lp - l) - dl * (u + 0.5 * dl)) + exp(c + (lm - l) + dl * (u - 0.5 * dl));
  }
  return log(s) + (l - 0.5 * u * u) + log(sum);
}

template <typename T, int D, int FAM>
__global__ __launch_bounds__(GLM_PREDICT_THREADS) void leg_glm_predict_kernel(
    const T* __restrict__ zm, const T* __restrict__ zc, const T* __restrict__ ys, const unsigned char* __restrict__ pattern,
    const T* __restrict__ offset, const T* __restrict__ extra, const T* __restrict__ Bg, int64_t P, int obs,
    T* __restrict__ eta_mean, T* __restrict__ eta_var, T* __restrict__ mean, T* __restrict__ var, T* __restrict__ logpdf) {
  const int64_t at = (int64_t)blockIdx.x * GLM_PREDICT_THREADS + threadIdx.x;
  if (at >= P * obs) return;
  const int64_t k = at / obs;
  const int c = (int)(at - k * obs);
  T Bc[D], row[D];
  load_vec<T, D>(Bg + c * D, Bc);
  load_vec<T, D>(zm + k * D, row);
  T muT = offset != nullptr ? offset[c] : T(0);
#pragma unroll
  for (int a = 0; a < D; ++a) muT = fmaT(Bc[a], row[a], muT);
  if (FAM != GLM_GAUSSIAN && extra != nullptr) muT += extra[at];
  T vT = T(0);
#pragma unroll
  for (int a = 0; a < D; ++a) {
    load_vec<T, D>(zc + (k * D + a) * D, row);
    T t = T(0);
#pragma unroll
    for (int b = 0; b < D; ++b) t = fmaT(row[b], Bc[b], t);
    vT = fmaT(Bc[a], t, vT);
  }
  vT = vT < T(0) ? T(0) : vT;                              // (a NaN stays NaN; a rounding-negative form reaches no square root)
  const bool given = ys != nullptr && (pattern == nullptr || (((unsigned)pattern[k] >> c) & 1u));
  const double mu = (double)muT, v = (double)vT;
  const double y = given ? (double)ys[at] : 0.0;
  double m_out, v_out, lp = 0.0;
  if (FAM == GLM_GAUSSIAN) {
    const double tot = v + (double)extra[at], res = y - mu;
    m_out = mu;
    v_out = tot;
    lp = -0.5 * res * res / tot - 0.5 * log(6.283185307179586476925 * tot);
  } else if (FAM == GLM_POISSON) {
    m_out = exp(mu + 0.5 * v);
    v_out = fma(m_out * m_out, expm1(v), m_out);
    if (given) lp = glm_log_integral<GLM_POISSON>(y, mu, v) - lgamma(y + 1.0);
  } else {
    // L1, L0, and the rule at y itself where y is neither (values of ys are not checked): one copy of the rule's code
    const bool other = given && y != 1.0 && y != 0.0;
    double L1 = 0.0, L0 = 0.0;
#pragma unroll 1
    for (int j = 0; j < 3; ++j) {
      if (j == 2 && !other) continue;
      const double r = glm_log_integral<GLM_BERNOULLI>(j == 0 ? 1.0 : (j == 1 ? 0.0 : y), mu, v);
      if (j == 0) L1 = r;
      else if (j == 1) L0 = r;
      else lp = r;
    }
    m_out = exp(L1);
    v_out = exp(L1 + L0);
    if (given && !other) lp = y == 1.0 ? L1 : L0;
  }
  eta_mean[at] = muT;
  eta_var[at] = vT;
  mean[at] = (T)m_out;
  var[at] = (T)v_out;
  if (ys != nullptr) logpdf[at] = given ? (T)lp : T(0);
}

template <typename T, int D>
void launch_glm_predict(const T* zm, const T* zc, const T* ys, const unsigned char* pattern, const T* offset, const T* extra,
                        const T* Bm, int64_t P, int obs, int family, T* eta_mean, T* eta_var, T* mean, T* var, T* logpdf,
                        hipStream_t st) {
  const dim3 grid((unsigned)((P * obs + GLM_PREDICT_THREADS - 1) / GLM_PREDICT_THREADS)), block(GLM_PREDICT_THREADS);
  if (family == GLM_POISSON)
    hipLaunchKernelGGL((leg_glm_predict_kernel<T, D, GLM_POISSON>), grid, block, 0, st, zm, zc, ys, pattern, offset, extra, Bm,
                       P, obs, eta_mean, eta_var, mean, var, logpdf);
  else if (family == GLM_BERNOULLI)
    hipLaunchKernelGGL((leg_glm_predict_kernel<T, D, GLM_BERNOULLI>), grid, block, 0, st, zm, zc, ys, pattern, offset, extra,
                       Bm, P, obs, eta_mean, eta_var, mean, var, logpdf);
  else
    hipLaunchKernelGGL((leg_glm_predict_kernel<T, D, GLM_GAUSSIAN>), grid, block, 0, st, zm, zc, ys, pattern, offset, extra,
                       Bm, P, obs, eta_mean, eta_var, mean, var, logpdf);
}

}  // namespace cgps
