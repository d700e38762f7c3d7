// cgps_leg_glm_grad.hip -- the gradient of the Laplace evidence at the mode (cgps_leg_glm_evidence_rhs,
// cgps_leg_glm_evidence_adjoint: include/cgps_glm_grad.h, kernels in cgps_leg_glm_grad.h).  A translation unit of its
// own, beside cgps_leg_glm.hip: three kernels x rank x channel form x precision.
#include "cgps_host.h"
#include "../../include/cgps_glm_grad.h"
#include "cgps_leg_glm_grad.h"

using namespace cgps_host;

namespace {

// what both entries ask of their scalar arguments; CGPS_OK, or the error with `me` in its text
int check_glm_grad_scalars(const char* me, int64_t B, int64_t R, int d, int obs, int dtype, int family) {
  if (B < 0 || R < 0) return fail(CGPS_ERR_ARG, "%s: B = %lld series, R = %lld rows", me, (long long)B, (long long)R);
  if (family != CGPS_GLM_POISSON && family != CGPS_GLM_BERNOULLI && family != CGPS_GLM_GAUSSIAN)
    return fail(CGPS_ERR_ARG, "%s: family = %d, none of 0 (Poisson), 1 (Bernoulli), 2 (Gaussian)", me, family);
  if (obs < 1 || obs > 8) return fail(CGPS_ERR_UNSUPPORTED, "%s: obs = %d outside 1..8", me, obs);
  if (dtype != CGPS_F32 && dtype != CGPS_F64) return fail(CGPS_ERR_UNSUPPORTED, "dtype %d not supported", dtype);
  if (d < 1 || d > 8) return fail(CGPS_ERR_UNSUPPORTED, "block size d=%d outside 1..8", d);
  if (B > 2147483647LL) return fail(CGPS_ERR_ARG, "%s: B = %lld series, more than one launch takes", me, (long long)B);
  return CGPS_OK;
}

}  // namespace

extern "C" {

int cgps_leg_glm_evidence_rhs(const void* z, const void* Sd, const void* ys, const unsigned char* pattern,
                              const void* offset, const void* extra, const void* Bmat, int64_t R, int d, int obs, int dtype,
                              int family, void* s, void* stream) {
  const char* me = "cgps_leg_glm_evidence_rhs";
  if (int rc = check_glm_grad_scalars(me, 1, R, d, obs, dtype, family)) return rc;
  if (R == 0) return CGPS_OK;
  const PtrArg required[] = {{"z", z, 0}, {"Sd", Sd, 0}, {"ys", ys, 0}, {"Bmat", Bmat, 0}, {"s", s, 0}};
  for (const PtrArg& a : required)
    if (!a.p) return fail(CGPS_ERR_ARG, "%s: %s = NULL", me, a.name);
  if (family == CGPS_GLM_GAUSSIAN && !extra) return fail(CGPS_ERR_ARG, "%s: extra = NULL (the variances of the Gaussian family)", me);
  const size_t es = elem_bytes(dtype);
  if (int rc = check_alignment(me, {{"z", z, ALIGN_VEC}, {"Sd", Sd, ALIGN_VEC}, {"ys", ys, es}, {"offset", offset, es},
                                    {"extra", extra, es}, {"Bmat", Bmat, es}, {"s", s, ALIGN_VEC}}))
    return rc;
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    cgps::launch_glm_evidence_rhs<T, D>((const T*)z, (const T*)Sd, (const T*)ys, pattern, (const T*)offset, (const T*)extra,
                                        (const T*)Bmat, R, obs, family, (T*)s, (hipStream_t)stream);
    return check_launch("LEG Laplace evidence rhs");
  });
}

int cgps_leg_glm_evidence_adjoint(const void* z, const void* u, const void* Sd, const void* So, const void* Pd,
                                  const void* Po, const void* ys, const unsigned char* pattern, const void* offset,
                                  const void* extra, const void* Bmat, const int64_t* offsets, const double* gE, int64_t B,
                                  int64_t R, int d, int obs, int dtype, int family, void* gRs, void* gOs, void* g_extra,
                                  double* gB_part, double* goffset_part, void* stream) {
  const char* me = "cgps_leg_glm_evidence_adjoint";
  if (int rc = check_glm_grad_scalars(me, B, R, d, obs, dtype, family)) return rc;
  if (R == 0 || B == 0) return CGPS_OK;
  const PtrArg required[] = {{"z", z, 0}, {"u", u, 0}, {"Sd", Sd, 0}, {"Pd", Pd, 0}, {"ys", ys, 0}, {"Bmat", Bmat, 0},
                             {"offsets", offsets, 0}, {"gE", gE, 0}, {"gRs", gRs, 0}, {"g_extra", g_extra, 0},
                             {"gB_part", gB_part, 0}, {"goffset_part", goffset_part, 0}};
  for (const PtrArg& a : required)
    if (!a.p) return fail(CGPS_ERR_ARG, "%s: %s = NULL", me, a.name);
  if (R > 1) {
    const PtrArg coupled[] = {{"So", So, 0}, {"Po", Po, 0}, {"gOs", gOs, 0}};
    for (const PtrArg& a : coupled)
      if (!a.p) return fail(CGPS_ERR_ARG, "%s: %s = NULL with R = %lld rows", me, a.name, (long long)R);
  }
  if (family == CGPS_GLM_GAUSSIAN && !extra) return fail(CGPS_ERR_ARG, "%s: extra = NULL (the variances of the Gaussian family)", me);
  const size_t es = elem_bytes(dtype);
  if (int rc = check_alignment(me, {{"z", z, ALIGN_VEC}, {"u", u, ALIGN_VEC}, {"Sd", Sd, ALIGN_VEC}, {"So", So, ALIGN_VEC},
                                    {"Pd", Pd, ALIGN_VEC}, {"Po", Po, ALIGN_VEC}, {"ys", ys, es}, {"offset", offset, es},
                                    {"extra", extra, es}, {"Bmat", Bmat, es}, {"offsets", offsets, 8}, {"gE", gE, 8},
                                    {"gRs", gRs, ALIGN_VEC}, {"gOs", gOs, ALIGN_VEC}, {"g_extra", g_extra, es},
                                    {"gB_part", gB_part, 8}, {"goffset_part", goffset_part, 8}}))
    return rc;
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    cgps::launch_glm_evidence_adjoint<T, D>((const T*)z, (const T*)u, (const T*)Sd, (const T*)So, (const T*)Pd, (const T*)Po,
                                            (const T*)ys, pattern, (const T*)offset, (const T*)extra, (const T*)Bmat, offsets,
                                            gE, B, R, obs, family, (T*)gRs, (T*)gOs, (T*)g_extra, gB_part, goffset_part,
                                            (hipStream_t)stream);
    return check_launch("LEG Laplace evidence adjoint");
  });
}

}  // extern "C"
