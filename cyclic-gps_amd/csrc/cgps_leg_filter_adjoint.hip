// cgps_leg_filter_adjoint.hip -- gradients through the LEG filter (cgps_leg_filter_adjoint.h).  A translation
// unit of its own: 80 fully unrolled instantiations of the reverse walk (d 1..8, five forms of the channel axis, two
// precisions) and 16 each of the gap pre-pass and the Frechet pass.
#include "cgps_host.h"
#include "cgps_leg_filter_adjoint.h"

using namespace cgps_host;

static int adjoint_sizes(const char* name, int64_t B, int64_t R, int64_t M, int d, int obs, int dtype) {
  if (B < 0 || R < 0 || B > ((int64_t)1 << 36) || R > ((int64_t)1 << 36))
    return fail(CGPS_ERR_ARG, "%s: B = %lld series, R = %lld rows", name, (long long)B, (long long)R);
  if (M < 1 || M > 65535) return fail(CGPS_ERR_ARG, "%s: M = %lld models, outside 1..65535", name, (long long)M);
  if (obs < 1 || obs > 8) return fail(CGPS_ERR_ARG, "%s: obs = %d outside 1..8", name, obs);
  if (d < 1 || d > 8) return fail(CGPS_ERR_ARG, "%s: block size d = %d outside 1..8", name, d);
  if (dtype != CGPS_F32 && dtype != CGPS_F64) return fail(CGPS_ERR_UNSUPPORTED, "dtype %d not supported", dtype);
  return CGPS_OK;
}

extern "C" {

int cgps_leg_filter_adjoint_workspace_bytes(int64_t R, int64_t B, int64_t M, int d, int obs, int dtype, size_t* bytes) {
  if (!bytes) return fail(CGPS_ERR_ARG, "cgps_leg_filter_adjoint_workspace_bytes: null pointer");
  if (int rc = adjoint_sizes("cgps_leg_filter_adjoint_workspace_bytes", B, R, M, d, obs, dtype)) return rc;
  *bytes = filter_adjoint_ws_bytes(R, B, M, d, obs, dtype == CGPS_F32 ? 4 : 8);
  return CGPS_OK;
}

int cgps_leg_filter_adjoint(const void* xs, const uint8_t* pattern, const void* noise_var, const int64_t* row_offsets,
                            int64_t B, int64_t R, int64_t M, const void* G, const void* Bmat, const void* LLT, int d,
                            int obs, int dtype, const void* gap, const void* z_mean, const void* z_cov, const void* m0,
                            const void* P0, const void* g_mean, const void* g_cov, const void* g_logpdf,
                            const void* g_z_mean, const void* g_z_cov, void* ws, size_t ws_bytes, void* g_xs,
                            void* g_noise_var, void* g_Bmat, void* g_LLT, void* g_m0, void* g_P0, void* g_G_partial,
                            void* g_gap, void* stream) {
  if (int rc = adjoint_sizes("cgps_leg_filter_adjoint", B, R, M, d, obs, dtype)) return rc;
  if ((m0 != nullptr) != (P0 != nullptr))
    return fail(CGPS_ERR_ARG, "cgps_leg_filter_adjoint: m0 and P0 come together or not at all");
  if (R == 0 || B == 0) return CGPS_OK;
  if (!xs || !row_offsets || !G || !Bmat || !LLT || !gap || !z_mean || !z_cov || !ws || !g_xs || !g_noise_var || !g_Bmat ||
      !g_LLT || !g_m0 || !g_P0 || !g_G_partial || !g_gap)
    return fail(CGPS_ERR_ARG, "cgps_leg_filter_adjoint: null pointer");
  const size_t need = filter_adjoint_ws_bytes(R, B, M, d, obs, dtype == CGPS_F32 ? 4 : 8);
  if (ws_bytes < need)
    return fail(CGPS_ERR_ARG, "cgps_leg_filter_adjoint: workspace of %zu bytes, %zu needed", ws_bytes, need);
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_leg_filter_adjoint", {{"ws", ws, ALIGN_WS}})) return rc;
    cgps::launch_filter_adjoint<T, D>((const T*)xs, pattern, (const T*)noise_var, row_offsets, B, R, M, (const T*)G,
                                      (const T*)Bmat, (const T*)LLT, obs, (const T*)gap, (const T*)z_mean,
                                      (const T*)z_cov, (const T*)m0, (const T*)P0, (const T*)g_mean, (const T*)g_cov,
                                      (const T*)g_logpdf, (const T*)g_z_mean, (const T*)g_z_cov, (T*)ws, (T*)g_xs,
                                      (T*)g_noise_var, (T*)g_Bmat, (T*)g_LLT, (T*)g_m0, (T*)g_P0, (T*)g_G_partial,
                                      (T*)g_gap, (hipStream_t)stream);
    return check_launch("LEG filter adjoint");
  });
}

}  // extern "C"
