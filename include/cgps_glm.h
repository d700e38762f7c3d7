/* libcgps -- the extension entry points for observations that are not Gaussian (counts, binary outcomes) under a LEG
 * prior.  A header of its own beside cgps.h: the symbols here are exported by the same libcgps.so, follow the
 * conventions of cgps.h (device pointers, C-contiguous arrays, CGPS_F32 / CGPS_F64, error codes, cgps_last_error, a
 * HIP stream as void*, nothing allocated, freed or synchronised) and are held to the same memory contract.
 * CGPS_VERSION is that of cgps.h.
 */
#ifndef CGPS_GLM_H
#define CGPS_GLM_H

#include "cgps.h"

#ifdef __cplusplus
extern "C" {
#endif

/* observation families: log p(y | eta), without the term that does not depend on eta */
enum {
  CGPS_GLM_POISSON = 0,   /* y eta - exp(eta)                     (the caller adds -lgamma(y + 1)) */
  CGPS_GLM_BERNOULLI = 1, /* y eta - log(1 + exp(eta)) */
  CGPS_GLM_GAUSSIAN = 2   /* -(y - eta)^2 / (2 s) - log(2 pi s) / 2, s the entry's variance */
};

/* flags of a series' state (state[b][2], a sum of these as a double) */
enum {
  CGPS_GLM_CONVERGED = 1, /* the accepted gain, or the bound on any gain along the proposal, was <= tol (1 + |psi|) */
  CGPS_GLM_STALLED = 2    /* no candidate step was finite and not below the current objective, and the bound is above
                             the tolerance: the series keeps its z */
};

#define CGPS_GLM_STATE 4       /* doubles per series in state_in / state_out */
#define CGPS_GLM_CANDIDATES 12 /* step lengths tried: 1, 1/2, .., 2^-11 */

/* One damped Newton step towards the mode of
 *     psi_b(z) = sum over observed (i, c) of log p(y_ic | eta_ic) - 1/2 z^T K_b z,
 *     eta_ic = Bmat[c,:] z_i + offset[c] + log_exposure[i][c],
 * for B independent series at once, K_b the prior precision of series b (blocks Rs, Os of the concatenated batch, as
 * cgps_peg_precision_seg writes them; the entry of Os between two series is never read).  One workgroup per series;
 * every sum runs in a fixed order, so a series' results do not depend on the rest of the batch.  Out of place.
 *
 * Read (never written):
 *   z [R][d]           the current point of every series, R = offsets[B] rows in all
 *   prop [R][d]        the Newton proposal J^-1 rhs of the previous call's J_Rs, Os and rhs; NULL on the first call
 *   Rs [R][d][d], Os [R-1][d][d]   the prior precision blocks (Os may be NULL when R = 1)
 *   ys [R][obs]        observations, in the dtype of the call; an unobserved entry is never read
 *   pattern [R]        bytes, bit c of pattern[i] set = entry (i, c) is observed; NULL = everything is
 *   offset [obs]       or NULL (zeros)
 *   extra [R][obs]     CGPS_GLM_GAUSSIAN: the variances s (required).  Other families: log_exposure, or NULL (zeros).
 *                      An unobserved entry is never read.
 *   Bmat [obs][d]      the observation matrix
 *   offsets [B+1]      int64, rows of series b are offsets[b] .. offsets[b+1] - 1; clamped to 0 .. R
 *   state_in [B][4]    doubles {psi, iterations, flags, accepted step length} of the previous call; not read (may be
 *                      NULL) when prop is NULL
 * Written (every element, by every call):
 *   z_out [R][d]       z + alpha (prop - z), alpha the largest of 1, 1/2, .., 2^-11 whose objective is finite and not
 *                      below psi(z); z itself on the first call, for a frozen series and when no candidate qualifies
 *   J_Rs [R][d][d]     Rs + B^T W B at z_out (with Os the blocks of J)
 *   rhs [R][d]         B^T (W B z_out + g) at z_out, so that J^-1 rhs is the next proposal
 *   state_out [B][4]   psi(z_out); iterations (0 after the first call, + 1 for every step a series took part in); flags;
 *                      the accepted alpha (0: none)
 * A series whose flags are not 0 is frozen: prop is not read for it, z_out = z, its state is copied.
 * tol: the series is flagged CGPS_GLM_CONVERGED once the accepted gain is <= tol (1 + |psi|).
 *
 * Alignment: z, prop, Rs, Os, z_out, J_Rs and rhs on 16-byte boundaries, state_in and state_out on 8, everything else
 * on its element size.  A null required pointer, a misaligned one (both named in cgps_last_error()), B < 0, R < 0,
 * an unknown family, or CGPS_GLM_GAUSSIAN without extra are CGPS_ERR_ARG; obs outside 1..8, d outside 1..8 or an
 * unknown dtype are CGPS_ERR_UNSUPPORTED; all before anything is launched.  B = 0 or R = 0 returns CGPS_OK and touches
 * nothing.  No workspace. */
int cgps_leg_glm_step(const void* z, const void* prop, const void* Rs, const void* Os, const void* ys,
                      const unsigned char* pattern, const void* offset, const void* extra, const void* Bmat,
                      const int64_t* offsets, int64_t B, int64_t R, int d, int obs, int dtype, int family, double tol,
                      const double* state_in, void* z_out, void* J_Rs, void* rhs, double* state_out, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* CGPS_GLM_H */
