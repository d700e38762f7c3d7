// cgps_leg_glm.hip -- the damped Newton step of the Laplace approximation for count and binary observations under a
// LEG prior (cgps_leg_glm_step: include/cgps_glm.h, kernel in cgps_leg_glm.h).  A translation unit of its own: 80
// instantiations (rank x channel form x precision) that compile next to the other units.
#include "cgps_host.h"
#include "../../include/cgps_glm.h"
#include "cgps_leg_glm.h"

using namespace cgps_host;

static_assert(CGPS_GLM_STATE == cgps::GLM_STATE && CGPS_GLM_CANDIDATES == cgps::GLM_CANDIDATES, "cgps_glm.h and cgps_leg_glm.h");
static_assert(CGPS_GLM_POISSON == cgps::GLM_POISSON && CGPS_GLM_BERNOULLI == cgps::GLM_BERNOULLI &&
              CGPS_GLM_GAUSSIAN == cgps::GLM_GAUSSIAN && CGPS_GLM_CONVERGED == cgps::GLM_CONVERGED &&
              CGPS_GLM_STALLED == cgps::GLM_STALLED, "cgps_glm.h and cgps_leg_glm.h");

extern "C" {

int cgps_leg_glm_step(const void* z, const void* prop, const void* Rs, const void* Os, const void* ys,
                      const unsigned char* pattern, const void* offset, const void* extra, const void* Bmat,
                      const int64_t* offsets, int64_t B, int64_t R, int d, int obs, int dtype, int family, double tol,
                      const double* state_in, void* z_out, void* J_Rs, void* rhs, double* state_out, void* stream) {
  const char* me = "cgps_leg_glm_step";
  if (B < 0 || R < 0) return fail(CGPS_ERR_ARG, "%s: B = %lld series, R = %lld rows", me, (long long)B, (long long)R);
  if (family != CGPS_GLM_POISSON && family != CGPS_GLM_BERNOULLI && family != CGPS_GLM_GAUSSIAN)
    return fail(CGPS_ERR_ARG, "%s: family = %d, none of 0 (Poisson), 1 (Bernoulli), 2 (Gaussian)", me, family);
  if (obs < 1 || obs > 8) return fail(CGPS_ERR_UNSUPPORTED, "%s: obs = %d outside 1..8", me, obs);
  if (dtype != CGPS_F32 && dtype != CGPS_F64) return fail(CGPS_ERR_UNSUPPORTED, "dtype %d not supported", dtype);
  if (d < 1 || d > 8) return fail(CGPS_ERR_UNSUPPORTED, "block size d=%d outside 1..8", d);
  if (B > 2147483647LL) return fail(CGPS_ERR_ARG, "%s: B = %lld series, more than one launch takes", me, (long long)B);
  if (R == 0 || B == 0) return CGPS_OK;
  const PtrArg required[] = {{"z", z, 0}, {"Rs", Rs, 0}, {"ys", ys, 0}, {"Bmat", Bmat, 0}, {"offsets", offsets, 0},
                             {"z_out", z_out, 0}, {"J_Rs", J_Rs, 0}, {"rhs", rhs, 0}, {"state_out", state_out, 0}};
  for (const PtrArg& a : required)
    if (!a.p) return fail(CGPS_ERR_ARG, "%s: %s = NULL", me, a.name);
  if (R > 1 && !Os) return fail(CGPS_ERR_ARG, "%s: Os = NULL with R = %lld rows", me, (long long)R);
  if (prop && !state_in) return fail(CGPS_ERR_ARG, "%s: state_in = NULL with a proposal", me);
  if (family == CGPS_GLM_GAUSSIAN && !extra) return fail(CGPS_ERR_ARG, "%s: extra = NULL (the variances of the Gaussian family)", me);
  const size_t es = elem_bytes(dtype);
  if (int rc = check_alignment(me, {{"z", z, ALIGN_VEC}, {"prop", prop, ALIGN_VEC}, {"Rs", Rs, ALIGN_VEC}, {"Os", Os, ALIGN_VEC},
                                    {"ys", ys, es}, {"offset", offset, es}, {"extra", extra, es}, {"Bmat", Bmat, es},
                                    {"offsets", offsets, 8}, {"state_in", state_in, 8}, {"z_out", z_out, ALIGN_VEC},
                                    {"J_Rs", J_Rs, ALIGN_VEC}, {"rhs", rhs, ALIGN_VEC}, {"state_out", state_out, 8}}))
    return rc;
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    cgps::launch_glm_step<T, D>((const T*)z, (const T*)prop, (const T*)Rs, (const T*)Os, (const T*)ys, pattern,
                                (const T*)offset, (const T*)extra, (const T*)Bmat, offsets, B, R, obs, family, tol, state_in,
                                (T*)z_out, (T*)J_Rs, (T*)rhs, state_out, (hipStream_t)stream);
    return check_launch("LEG Laplace step");
  });
}

}  // extern "C"
