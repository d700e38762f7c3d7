// cgps_leg_obs.hip -- the fused LEG reductions for series whose rows differ in their observation model.  Missing
// observations: every row names the entry of a table of diagonal terms it adds (chunk_reduce_kernel<.., SRC = 2>,
// cgps_tile.h; for many series in one launch leg_batch_kernel<.., LEG_ROWS_TABLE>, cgps_tile_leg_batch.h).  Noise variances
// of their own: every row adds a weighted sum of a basis shared by all rows (chunk_reduce_kernel<.., SRC = 3>; for many
// series in one launch leg_batch_kernel<.., LEG_ROWS_WEIGHTED>).  Both for M models over the same batch as well
// (LEG_ROWS_MODELS_TABLE, LEG_ROWS_MODELS_WEIGHTED: grid (B, 2, M)).
// The leave-one-out predictives of such series from their posterior (cgps_leg_loo: cgps_leg_loo.h) live here too.
// A translation unit of its own: these are the heaviest stage-1 instantiations of the library and compile next to
// cgps_mahal.hip, not after it.
#include "cgps_host.h"
#include "cgps_tile.h"
#include "cgps_tile_leg_batch.h"
#include "cgps_leg_loo.h"

using namespace cgps_host;

namespace cgps_host {
hipError_t leg_obs_reset_counters(hipStream_t st) { return cgps::fold_reset_counters(st); }
}  // namespace cgps_host

extern "C" {

int cgps_leg_mahal_logdet_pair_obs(const void* ts, const void* G, const void* A_table, int P, const unsigned char* pattern,
                                   const void* v, int64_t N, int d, int dtype, void* ws, size_t ws_bytes, double* out4,
                                   int* info2, void* stream) {
  if (bad_common(N, d) || !ts || !G || !A_table || !pattern || !ws || !out4 || !info2)
    return fail(CGPS_ERR_ARG, "cgps_leg_mahal_logdet_pair_obs: null pointer or N < 1");
  if (P < 1 || P > 256) return fail(CGPS_ERR_ARG, "cgps_leg_mahal_logdet_pair_obs: P = %d table entries, outside 1..256", P);
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_leg_mahal_logdet_pair_obs", {{"ts", ts, elem_bytes(dtype)}, {"G", G, elem_bytes(dtype)}, {"A_table", A_table, elem_bytes(dtype)},
                                                                  {"v", v, elem_bytes(dtype)}, {"ws", ws, ALIGN_WS}, {"out4", out4, 8}, {"info2", info2, 4}})) return rc;
    if constexpr (cgps::leg_source_supported<T, D>())
      if (ws_bytes < leg_pair_ws_bytes(N, D, sizeof(T)))
        return fail(CGPS_ERR_ARG, "workspace too small for cgps_leg_mahal_logdet_pair_obs (that of cgps_leg_mahal_logdet_pair): %zu < %zu", ws_bytes,
                    leg_pair_ws_bytes(N, D, sizeof(T)));
    const int rc = cgps::run_tile_leg<T, D, 2>((const T*)ts, (const T*)G, (const T*)A_table, (const T*)v, N, (char*)ws, ws_bytes,
                                               out4, info2, (hipStream_t)stream, true, pattern, P);
    if (rc == -1) return fail(CGPS_ERR_ARG, "workspace too small for cgps_leg_mahal_logdet_pair_obs (that of cgps_leg_mahal_logdet_pair)");
    if (rc == -2) return fail(CGPS_ERR_UNSUPPORTED, "cgps_leg_mahal_logdet_pair_obs: not built for this block size (d = 8, fp64 d = 6) or CGPS_NO_FOLD=1");
    return check_launch("LEG tile reduction (pair, per-row observation pattern)");
  });
}

int cgps_leg_mahal_logdet_pair_w(const void* ts, const void* G, const void* basis, int Kb, const void* weights, const void* v,
                                 int64_t N, int d, int dtype, void* ws, size_t ws_bytes, double* out4, int* info2, void* stream) {
  if (bad_common(N, d) || !ts || !G || !basis || !weights || !ws || !out4 || !info2)
    return fail(CGPS_ERR_ARG, "cgps_leg_mahal_logdet_pair_w: null pointer or N < 1");
  if (Kb < 1 || Kb > 64) return fail(CGPS_ERR_ARG, "cgps_leg_mahal_logdet_pair_w: Kb = %d basis blocks, outside 1..64", Kb);
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_leg_mahal_logdet_pair_w", {{"ts", ts, elem_bytes(dtype)}, {"G", G, elem_bytes(dtype)}, {"basis", basis, elem_bytes(dtype)},
                                                                {"weights", weights, elem_bytes(dtype)}, {"v", v, elem_bytes(dtype)}, {"ws", ws, ALIGN_WS}, {"out4", out4, 8}, {"info2", info2, 4}})) return rc;
    if constexpr (cgps::leg_source_supported<T, D>())
      if (ws_bytes < leg_pair_ws_bytes(N, D, sizeof(T)))
        return fail(CGPS_ERR_ARG, "workspace too small for cgps_leg_mahal_logdet_pair_w (that of cgps_leg_mahal_logdet_pair): %zu < %zu", ws_bytes,
                    leg_pair_ws_bytes(N, D, sizeof(T)));
    const int rc = cgps::run_tile_leg<T, D, 3>((const T*)ts, (const T*)G, (const T*)basis, (const T*)v, N, (char*)ws, ws_bytes,
                                               out4, info2, (hipStream_t)stream, true, (const unsigned char*)weights, Kb);
    if (rc == -1) return fail(CGPS_ERR_ARG, "workspace too small for cgps_leg_mahal_logdet_pair_w (that of cgps_leg_mahal_logdet_pair)");
    if (rc == -2) return fail(CGPS_ERR_UNSUPPORTED, "cgps_leg_mahal_logdet_pair_w: not built for this block size (d = 8, fp64 d = 6) or CGPS_NO_FOLD=1");
    return check_launch("LEG tile reduction (pair, per-row weighted basis)");
  });
}

int cgps_leg_loglik_batch_obs(const void* ts, const int64_t* offsets, int64_t B, const void* G, const void* A_table, int P,
                              const unsigned char* pattern, const void* v, const void* q, int d, int dtype, int64_t max_rows,
                              double* out4, int* info2, void* stream) {
  if (P < 1 || P > 256) return fail(CGPS_ERR_ARG, "cgps_leg_loglik_batch_obs: P = %d table entries, outside 1..256", P);
  return leg_rows_entry<cgps::LEG_ROWS_TABLE>("cgps_leg_loglik_batch_obs", "LEG batched reduction (per-row observation pattern)",
                                              !A_table || !pattern, ts, offsets, B, 0, 1, G, A_table, P, pattern, v, q, d,
                                              dtype, max_rows, out4, info2, stream);
}

int cgps_leg_loglik_batch_w(const void* ts, const int64_t* offsets, int64_t B, const void* G, const void* basis, int Kb,
                            const void* weights, const void* v, const void* q, int d, int dtype, int64_t max_rows, double* out4,
                            int* info2, void* stream) {
  if (Kb < 1 || Kb > 64) return fail(CGPS_ERR_ARG, "cgps_leg_loglik_batch_w: Kb = %d basis blocks, outside 1..64", Kb);
  return leg_rows_entry<cgps::LEG_ROWS_WEIGHTED>("cgps_leg_loglik_batch_w", "LEG batched reduction (per-row weighted basis)",
                                                 !basis || !weights, ts, offsets, B, 0, 1, G, basis, Kb, weights, v, q, d,
                                                 dtype, max_rows, out4, info2, stream);
}

int cgps_leg_loglik_models_obs(const void* ts, const int64_t* offsets, int64_t B, int64_t R, int64_t M, const void* G,
                               const void* A_table, int P, const unsigned char* pattern, const void* v, const void* q, int d,
                               int dtype, int64_t max_rows, double* out4, int* info2, void* stream) {
  if (P < 1 || P > 256) return fail(CGPS_ERR_ARG, "cgps_leg_loglik_models_obs: P = %d table entries, outside 1..256", P);
  return leg_rows_entry<cgps::LEG_ROWS_MODELS_TABLE>(
      "cgps_leg_loglik_models_obs", "LEG batched reduction (models, per-row observation pattern)", !A_table || !pattern, ts,
      offsets, B, R, M, G, A_table, P, pattern, v, q, d, dtype, max_rows, out4, info2, stream);
}

int cgps_leg_loglik_models_w(const void* ts, const int64_t* offsets, int64_t B, int64_t R, int64_t M, const void* G,
                             const void* basis, int Kb, const void* weights, const void* v, const void* q, int d, int dtype,
                             int64_t max_rows, double* out4, int* info2, void* stream) {
  if (Kb < 1 || Kb > 64) return fail(CGPS_ERR_ARG, "cgps_leg_loglik_models_w: Kb = %d basis blocks, outside 1..64", Kb);
  return leg_rows_entry<cgps::LEG_ROWS_MODELS_WEIGHTED>(
      "cgps_leg_loglik_models_w", "LEG batched reduction (models, per-row weighted basis)", !basis || !weights, ts, offsets, B,
      R, M, G, basis, Kb, weights, v, q, d, dtype, max_rows, out4, info2, stream);
}

int cgps_leg_loo(const void* xs, const uint8_t* pattern, const void* noise_var, const int64_t* row_offsets, int64_t B,
                 int64_t R, int64_t M, const void* Bmat, const void* LLT, int d, int obs, int dtype, const void* ip_mean,
                 const void* ip_cov_diag, int leave, void* out_mean, void* out_var, void* out_logpdf, double* out_score,
                 int* info, void* stream) {
  if (B < 0 || R < 0) return fail(CGPS_ERR_ARG, "cgps_leg_loo: B = %lld series, R = %lld rows", (long long)B, (long long)R);
  if (M < 1 || M > 65535) return fail(CGPS_ERR_ARG, "cgps_leg_loo: M = %lld models, outside 1..65535", (long long)M);
  if (leave != cgps::LOO_ENTRY && leave != cgps::LOO_ROW)
    return fail(CGPS_ERR_ARG, "cgps_leg_loo: leave = %d, neither 0 (entry) nor 1 (row)", leave);
  if (obs < 1 || obs > 8) return fail(CGPS_ERR_UNSUPPORTED, "cgps_leg_loo: obs = %d outside 1..8", obs);
  if (dtype != CGPS_F32 && dtype != CGPS_F64) return fail(CGPS_ERR_UNSUPPORTED, "dtype %d not supported", dtype);
  if (d < 1 || d > 8) return fail(CGPS_ERR_UNSUPPORTED, "block size d=%d outside 1..8", d);
  if (R == 0 || B == 0) return CGPS_OK;
  if (!xs || !row_offsets || !Bmat || !LLT || !ip_mean || !ip_cov_diag || !out_mean || !out_var || !out_logpdf ||
      !out_score || !info)
    return fail(CGPS_ERR_ARG, "cgps_leg_loo: null pointer");
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    (void)hipMemsetAsync(info, 0, sizeof(int), (hipStream_t)stream);
    cgps::launch_loo<T, D>((const T*)xs, pattern, (const T*)noise_var, row_offsets, B, R, M, (const T*)Bmat, (const T*)LLT,
                           obs, (const T*)ip_mean, (const T*)ip_cov_diag, leave, (T*)out_mean, (T*)out_var, (T*)out_logpdf,
                           out_score, info, (hipStream_t)stream);
    return check_launch("LEG leave-one-out predictives");
  });
}

}  // extern "C"
