// cgps_leg_glm_predict.hip -- predictions on the response scale from a latent Gaussian (cgps_leg_glm_predict:
// include/cgps_glm_predict.h, kernel in cgps_leg_glm_predict.h).  A translation unit of its own, beside
// cgps_leg_glm_grad.hip: one kernel x rank x family x precision.
#include "cgps_host.h"
#include "../../include/cgps_glm_predict.h"
#include "cgps_leg_glm_predict.h"

using namespace cgps_host;

extern "C" {

int cgps_leg_glm_predict(const void* zm, const void* zc, const void* ys, const unsigned char* pattern, const void* offset,
                         const void* extra, const void* Bmat, int64_t P, int d, int obs, int dtype, int family,
                         void* eta_mean, void* eta_var, void* mean, void* var, void* logpdf, void* stream) {
  const char* me = "cgps_leg_glm_predict";
  if (P < 0) return fail(CGPS_ERR_ARG, "%s: P = %lld rows", me, (long long)P);
  if (family != CGPS_GLM_POISSON && family != CGPS_GLM_BERNOULLI && family != CGPS_GLM_GAUSSIAN)
    return fail(CGPS_ERR_ARG, "%s: family = %d, none of 0 (Poisson), 1 (Bernoulli), 2 (Gaussian)", me, family);
  if (obs < 1 || obs > 8) return fail(CGPS_ERR_UNSUPPORTED, "%s: obs = %d outside 1..8", me, obs);
  if (dtype != CGPS_F32 && dtype != CGPS_F64) return fail(CGPS_ERR_UNSUPPORTED, "dtype %d not supported", dtype);
  if (d < 1 || d > 8) return fail(CGPS_ERR_UNSUPPORTED, "block size d=%d outside 1..8", d);
  if (P > 2147483647LL * (cgps::GLM_PREDICT_THREADS / 8))
    return fail(CGPS_ERR_ARG, "%s: P = %lld rows, more than one launch takes", me, (long long)P);
  if (P == 0) return CGPS_OK;
  const PtrArg required[] = {{"zm", zm, 0},   {"zc", zc, 0},     {"Bmat", Bmat, 0}, {"eta_mean", eta_mean, 0}, {"eta_var", eta_var, 0},
                             {"mean", mean, 0}, {"var", var, 0}};
  for (const PtrArg& a : required)
    if (!a.p) return fail(CGPS_ERR_ARG, "%s: %s = NULL", me, a.name);
  if (family == CGPS_GLM_GAUSSIAN && !extra) return fail(CGPS_ERR_ARG, "%s: extra = NULL (the variances of the Gaussian family)", me);
  if (ys && !logpdf) return fail(CGPS_ERR_ARG, "%s: logpdf = NULL with ys given", me);
  if (!ys && logpdf) return fail(CGPS_ERR_ARG, "%s: ys = NULL with logpdf given", me);
  const size_t es = elem_bytes(dtype);
  if (int rc = check_alignment(me, {{"zm", zm, es}, {"zc", zc, ALIGN_VEC}, {"ys", ys, es}, {"offset", offset, es},
                                    {"extra", extra, es}, {"Bmat", Bmat, es}, {"eta_mean", eta_mean, es},
                                    {"eta_var", eta_var, es}, {"mean", mean, es}, {"var", var, es}, {"logpdf", logpdf, es}}))
    return rc;
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    cgps::launch_glm_predict<T, D>((const T*)zm, (const T*)zc, (const T*)ys, pattern, (const T*)offset, (const T*)extra,
                                   (const T*)Bmat, P, obs, family, (T*)eta_mean, (T*)eta_var, (T*)mean, (T*)var, (T*)logpdf,
                                   (hipStream_t)stream);
    return check_launch("LEG GLM predictions");
  });
}

}  // extern "C"
