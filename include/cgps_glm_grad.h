/* libcgps -- the gradient of the Laplace evidence of cgps_glm.h at the mode.  A header of its own beside
 * cgps_glm.h: the symbols here are exported by the same libcgps.so and follow the conventions of cgps.h and cgps_glm.h
 * (device pointers, C-contiguous arrays, CGPS_F32 / CGPS_F64, error codes, cgps_last_error, a HIP stream as void*,
 * nothing allocated, freed or synchronised), and are held to the same memory contract.  CGPS_VERSION is that of cgps.h.
 *
 * Per series, at the mode z of psi (cgps_leg_glm_step), the approximate log evidence is
 *     E = sum over observed (i, c) of l(y_ic, eta_ic) - 1/2 z^T K z + 1/2 log|K| - 1/2 log|J|,
 *     J = K + blockdiag(Bmat^T W_i Bmat),   eta_ic = Bmat[c,:] z_i + offset[c] + log_exposure[i][c],
 * with g = dl / d eta, w = -d^2 l / d eta^2 and w' = dw / d eta (Poisson: e^eta; Bernoulli: sigma (1 - sigma)
 * (1 - 2 sigma); Gaussian: 0).  With S = J^-1, P = K^-1 and v_ic = Bmat[c,:] S_ii Bmat[c,:]^T its gradient is, by the
 * implicit function theorem,
 *     s_i = -1/2 sum_c w'_ic v_ic Bmat[c,:]^T                       (cgps_leg_glm_evidence_rhs)
 *     u = J^-1 s                                                    (the caller's solve on the factor of J)
 *     G_K = 1/2 (P - S) - 1/2 z z^T - 1/2 (u z^T + z u^T)           on the block-tridiagonal pattern
 *     e_ic = g_ic - 1/2 w'_ic v_ic - w_ic (Bmat[c,:] u_i)           (cgps_leg_glm_evidence_adjoint)
 * pattern, offset and extra mean what they mean in cgps_leg_glm_step and are optional in the same way.
 */
#ifndef CGPS_GLM_GRAD_H
#define CGPS_GLM_GRAD_H

#include "cgps_glm.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The right-hand side of the implicit term, dE / dz at the mode, for every row of the concatenated batch.  One lane per
 * row; a row's result depends on that row alone.
 *
 * Read (never written):
 *   z [R][d]           the mode
 *   Sd [R][d][d]       the diagonal blocks of J^-1 at the mode
 *   ys [R][obs], pattern [R] or NULL, offset [obs] or NULL, extra [R][obs] (CGPS_GLM_GAUSSIAN: the variances, required;
 *                      other families: log_exposure or NULL), Bmat [obs][d]: as in cgps_leg_glm_step.  An unobserved
 *                      entry of ys and extra is never read.
 * Written (every element, by every call):
 *   s [R][d]           -1/2 sum over the row's observed c of w'_ic v_ic Bmat[c,:]; zeros where a row observes nothing and
 *                      for CGPS_GLM_GAUSSIAN
 *
 * Alignment: z, Sd and s on 16-byte boundaries, everything else on its element size.  A null required pointer, a
 * misaligned one (both named in cgps_last_error()), R < 0, an unknown family, or CGPS_GLM_GAUSSIAN without extra are
 * CGPS_ERR_ARG; obs outside 1..8, d outside 1..8 or an unknown dtype are CGPS_ERR_UNSUPPORTED; all before anything is
 * launched.  R = 0 returns CGPS_OK and touches nothing.  No workspace. */
int cgps_leg_glm_evidence_rhs(const void* z, const void* Sd, const void* ys, const unsigned char* pattern,
                              const void* offset, const void* extra, const void* Bmat, int64_t R, int d, int obs, int dtype,
                              int family, void* s, void* stream);

/* The cotangents of everything the evidence of B series is made of, each series' scaled by its gE[b].  A row kernel
 * (one lane per row) writes what belongs to a row; then one workgroup per series adds the series' terms of dE / dBmat
 * and dE / doffset in a fixed order, so a series' results do not depend on the rest of the batch.  The sum of the
 * partials over the series is the caller's.
 *
 * Read (never written):
 *   z [R][d]           the mode, R = offsets[B] rows in all
 *   u [R][d]           J^-1 s, s from cgps_leg_glm_evidence_rhs
 *   Sd [R][d][d], So [R-1][d][d]   the blocks [i][i] and [i+1][i] of J^-1 (So may be NULL when R = 1; its entry between
 *                      two series is never read)
 *   Pd [R][d][d], Po [R-1][d][d]   the same blocks of K^-1, K the prior precision
 *   ys, pattern, offset, extra, Bmat   as above
 *   offsets [B+1]      int64, rows of series b are offsets[b] .. offsets[b+1] - 1; clamped to 0 .. R
 *   gE [B]             doubles, the cotangent of every series' evidence
 * Written (every element, by every call):
 *   gRs [R][d][d]      gE_b G_K[i][i]: the cotangent of the prior's diagonal blocks
 *   gOs [R-1][d][d]    2 gE_b G_K[i+1][i], in the orientation of Os (K holds Os[i] and its transpose, hence the 2); a zero
 *                      block between two series (may be NULL when R = 1)
 *   g_extra [R][obs]   gE_b e_ic, the cotangent of log_exposure; CGPS_GLM_GAUSSIAN: that of the variances,
 *                      gE_b (1/2 res^2 / s^2 - 1/2 / s + 1/2 v_ic / s^2), res = y - eta.  Zero at unobserved entries.
 *   gB_part [B][obs][d]    doubles, gE_b sum over the series' observed (i, c) of e_ic z_i + g_ic u_i - w_ic S_ii Bmat[c,:]^T
 *   goffset_part [B][obs]  doubles, gE_b sum over the series' observed i of e_ic
 * A row that offsets assigns to no series takes gE = 0.  A series with gE[b] = 0 gets exact zeros in all five outputs
 * whatever its operands hold (selected, not multiplied: NaN or infinities in z, u or the blocks of such a series do not
 * reach an output).
 *
 * Alignment: z, u, Sd, So, Pd, Po, gRs and gOs on 16-byte boundaries, offsets, gE, gB_part and goffset_part on 8,
 * everything else on its element size.  Errors as above, with B < 0 also CGPS_ERR_ARG; all before anything is
 * launched.  B = 0 or R = 0 returns CGPS_OK and touches nothing.  No workspace. */
int cgps_leg_glm_evidence_adjoint(const void* z, const void* u, const void* Sd, const void* So, const void* Pd,
                                  const void* Po, const void* ys, const unsigned char* pattern, const void* offset,
                                  const void* extra, const void* Bmat, const int64_t* offsets, const double* gE, int64_t B,
                                  int64_t R, int d, int obs, int dtype, int family, void* gRs, void* gOs, void* g_extra,
                                  double* gB_part, double* goffset_part, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CGPS_GLM_GRAD_H */
