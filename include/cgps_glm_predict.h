/* libcgps -- predictions on the response scale from a latent Gaussian, for the families of cgps_glm.h.  A
 * header of its own beside cgps_glm.h and cgps_glm_grad.h: the symbol here is exported by the same libcgps.so and follows
 * the conventions of cgps.h (device pointers, C-contiguous arrays, CGPS_F32 / CGPS_F64, error codes, cgps_last_error, a
 * HIP stream as void*, nothing allocated, freed or synchronised), and is held to the same memory contract.  CGPS_VERSION
 * is that of cgps.h.
 *
 * Per entry (k, c), with the latent z_k ~ N(m_k, S_k) (cgps_leg_intercast_seg at a target time, or a row of the Laplace
 * posterior), the linear predictor eta = Bmat[c,:] z_k + offset[c] + log_exposure[k][c] is Gaussian with
 *     mu = Bmat[c,:] m_k + offset[c] + log_exposure[k][c],     v = Bmat[c,:] S_k Bmat[c,:]^T   (clamped at 0 from below)
 * and the entry's outputs are the moments of y and log I(y), I(y) = integral of p(y | eta) N(eta; mu, v) d eta:
 *   CGPS_GLM_GAUSSIAN    mean = mu, var = v + s, log I in closed form (s = extra[k][c], the observation variance)
 *   CGPS_GLM_POISSON     mean = exp(mu + v / 2), var = mean + mean^2 expm1(v), log I by the rule below
 *   CGPS_GLM_BERNOULLI   with L1 = log I(1), L0 = log I(0) by the rule: mean = exp(L1), var = exp(L1 + L0)
 * The rule is adaptive Gauss-Hermite in the standardised variable u, eta(u) = mu + sqrt(v) u, h(u) = l(y, eta(u)) - u^2/2
 * (l as in cgps_leg_glm_step, Poisson with its -lgamma(y + 1)), in fp64 in both precisions:
 *   centre   u = 0, then 12 steps u += min((sqrt(v) g - u) / (1 + v w), 1 / sqrt(v)), g = dl / d eta and w = -d^2 l / d eta^2
 *            at eta(u) (the clip, skipped at v = 0, keeps eta from rising by more than 1 per step)
 *   scale    s = (1 + v w(eta(u*)))^(-1/2)
 *   value    log I = log s + logsumexp_i [log(w_i / sqrt(pi)) + x_i^2 + h(u* + sqrt(2) s x_i)] over the 32 physicists'
 *            Gauss-Hermite nodes x_i and weights w_i
 * At v = 0 it returns l(y, mu) up to rounding.  Every loop has a fixed trip count: NaN in gives NaN out.
 */
#ifndef CGPS_GLM_PREDICT_H
#define CGPS_GLM_PREDICT_H

#include "cgps_glm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One lane per (row, channel); an entry's outputs depend on that row's operands alone: the same bits wherever the row
 * sits and whatever else is in the call.
 *
 * Read (never written):
 *   zm [P][d]          the latent means
 *   zc [P][d][d]       the latent covariances
 *   ys [P][obs] or NULL   held-out values; an entry that pattern marks as absent is never read
 *   pattern [P] or NULL   a bit per channel, as in cgps_leg_glm_step: which entries of ys exist (NULL: all of them)
 *   offset [obs] or NULL
 *   extra [P][obs]     CGPS_GLM_GAUSSIAN: the observation variances, required; other families: log_exposure or NULL.
 *                      Read at EVERY (k, c), whatever pattern says: eta_mean, mean and var depend on it
 *   Bmat [obs][d]
 * Written (every element, by every call):
 *   eta_mean [P][obs]  mu
 *   eta_var [P][obs]   v, never below 0
 *   mean [P][obs], var [P][obs]   the moments of y
 *   logpdf [P][obs]    log I(ys[k][c]); exact zero where pattern marks the entry absent.  Required when ys is given;
 *                      may be NULL only together with ys (then nothing is written for it)
 *
 * Alignment: zc on a 16-byte boundary, everything else on its element size.  A null required pointer, a
 * misaligned one (both named in cgps_last_error()), P < 0, an unknown family, CGPS_GLM_GAUSSIAN without extra, or ys
 * without logpdf (or logpdf without ys) are CGPS_ERR_ARG; obs outside 1..8, d outside 1..8 or an unknown dtype are
 * CGPS_ERR_UNSUPPORTED; all before anything is launched.  P = 0 returns CGPS_OK and touches nothing.  No workspace. */
int cgps_leg_glm_predict(const void* zm, const void* zc, const void* ys, const unsigned char* pattern, const void* offset,
                         const void* extra, const void* Bmat, int64_t P, int d, int obs, int dtype, int family,
                         void* eta_mean, void* eta_var, void* mean, void* var, void* logpdf, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CGPS_GLM_PREDICT_H */
