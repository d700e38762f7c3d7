// cgps_leg_filter.hip -- one-step-ahead predictives and filtered states of LEG series (cgps_leg_filter.h).
// A translation unit of its own: 80 fully unrolled instantiations of the walking kernel (d 1..8, five forms of the
// channel axis, two precisions) and 16 of the gap pre-pass, which compile next to the other units, not after them.
// The time-parallel form (cgps_leg_filter_scan.h) adds as many chunk kernels and 16 of each sweep kernel.
#include "cgps_host.h"
#include "cgps_leg_filter.h"
#include "cgps_leg_filter_scan.h"

using namespace cgps_host;

// The checks cgps_leg_filter and cgps_leg_filter_scan share, in the order in which they fire; `name` is the entry's, for
// the messages: filter_args before the entry's test for an empty call, filter_rows_fit after it.
static int filter_args(const char* name, int64_t B, int64_t R, int64_t M, int d, int obs, int dtype, const void* t0,
                       const void* m0, const void* P0) {
  if (B < 0 || R < 0) return fail(CGPS_ERR_ARG, "%s: B = %lld series, R = %lld rows", name, (long long)B, (long long)R);
  if (M < 1 || M > 65535) return fail(CGPS_ERR_ARG, "%s: M = %lld models, outside 1..65535", name, (long long)M);
  if (obs < 1 || obs > 8) return fail(CGPS_ERR_UNSUPPORTED, "%s: obs = %d outside 1..8", name, obs);
  if (dtype != CGPS_F32 && dtype != CGPS_F64) return fail(CGPS_ERR_UNSUPPORTED, "dtype %d not supported", dtype);
  if (d < 1 || d > 8) return fail(CGPS_ERR_UNSUPPORTED, "block size d=%d outside 1..8", d);
  if ((t0 != nullptr) != (m0 != nullptr) || (t0 != nullptr) != (P0 != nullptr))
    return fail(CGPS_ERR_ARG, "%s: t0, m0 and P0 come together or not at all", name);
  return CGPS_OK;
}
static int filter_rows_fit(const char* name, int64_t B, int64_t R) {
  if (B > ((int64_t)1 << 36) || R > ((int64_t)1 << 36))
    return fail(CGPS_ERR_ARG, "%s: B = %lld series or R = %lld rows, too many for one launch", name, (long long)B,
                (long long)R);
  return CGPS_OK;
}

extern "C" {

int cgps_leg_filter(const void* ts, const void* xs, const uint8_t* pattern, const void* noise_var,
                    const int64_t* row_offsets, int64_t B, int64_t R, int64_t M, const void* G, const void* Bmat,
                    const void* LLT, int d, int obs, int dtype, const void* t0, const void* m0, const void* P0,
                    void* pred_mean, void* pred_cov, void* logpdf, void* z_mean, void* z_cov, double* loglik, void* m_end,
                    void* P_end, int* info, void* stream) {
  if (int rc = filter_args("cgps_leg_filter", B, R, M, d, obs, dtype, t0, m0, P0)) return rc;
  if (R == 0 || B == 0) return CGPS_OK;
  if (int rc = filter_rows_fit("cgps_leg_filter", B, R)) return rc;
  if (!ts || !xs || !row_offsets || !G || !Bmat || !LLT || !pred_mean || !pred_cov || !logpdf || !z_mean || !z_cov ||
      !loglik || !m_end || !P_end || !info)
    return fail(CGPS_ERR_ARG, "cgps_leg_filter: null pointer");
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    (void)hipMemsetAsync(info, 0, sizeof(int), (hipStream_t)stream);
    cgps::launch_filter<T, D>((const T*)ts, (const T*)xs, pattern, (const T*)noise_var, row_offsets, B, R, M, (const T*)G,
                              (const T*)Bmat, (const T*)LLT, obs, (const T*)t0, (const T*)m0, (const T*)P0,
                              (T*)pred_mean, (T*)pred_cov, (T*)logpdf, (T*)z_mean, (T*)z_cov, loglik, (T*)m_end,
                              (T*)P_end, info, (hipStream_t)stream);
    return check_launch("LEG one-step-ahead predictives");
  });
}

int cgps_leg_filter_scan_workspace_bytes(int64_t n_chunks, int64_t M, int d, int dtype, int64_t fanout, size_t* bytes) {
  if (!bytes) return fail(CGPS_ERR_ARG, "cgps_leg_filter_scan_workspace_bytes: null pointer");
  if (n_chunks < 0 || n_chunks > ((int64_t)1 << 36) || M < 1 || M > 65535 || fanout < 2)
    return fail(CGPS_ERR_ARG, "cgps_leg_filter_scan_workspace_bytes: %lld chunks, M = %lld models, fanout %lld",
                (long long)n_chunks, (long long)M, (long long)fanout);
  if (dtype != CGPS_F32 && dtype != CGPS_F64) return fail(CGPS_ERR_UNSUPPORTED, "dtype %d not supported", dtype);
  if (d < 1 || d > 8) return fail(CGPS_ERR_UNSUPPORTED, "block size d=%d outside 1..8", d);
  *bytes = filter_scan_ws(n_chunks, M, d, dtype == CGPS_F32 ? 4 : 8, fanout).total;
  return CGPS_OK;
}

int cgps_leg_filter_scan(const void* ts, const void* xs, const uint8_t* pattern, const void* noise_var,
                         const int64_t* row_offsets, int64_t B, int64_t R, int64_t M, const void* G, const void* Bmat,
                         const void* LLT, int d, int obs, int dtype, const void* t0, const void* m0, const void* P0,
                         const int64_t* chunk_offsets, const int64_t* chunk_series, const int64_t* series_chunks,
                         int64_t n_chunks, int64_t chunk_rows, int64_t fanout, void* ws, size_t ws_bytes,
                         void* pred_mean, void* pred_cov, void* logpdf, void* z_mean, void* z_cov, double* loglik,
                         void* m_end, void* P_end, int* info, void* stream) {
  if (int rc = filter_args("cgps_leg_filter_scan", B, R, M, d, obs, dtype, t0, m0, P0)) return rc;
  if (chunk_rows < 1 || fanout < 2)
    return fail(CGPS_ERR_ARG, "cgps_leg_filter_scan: chunk_rows = %lld (at least 1), fanout = %lld (at least 2)",
                (long long)chunk_rows, (long long)fanout);
  if (R == 0 || B == 0) return CGPS_OK;
  if (int rc = filter_rows_fit("cgps_leg_filter_scan", B, R)) return rc;
  // every series has a chunk, every chunk a row, and no chunk more than chunk_rows of them
  if (n_chunks < B || n_chunks > R || n_chunks < (R + chunk_rows - 1) / chunk_rows)
    return fail(CGPS_ERR_ARG, "cgps_leg_filter_scan: %lld chunks of at most %lld rows for %lld series of %lld rows",
                (long long)n_chunks, (long long)chunk_rows, (long long)B, (long long)R);
  if (!ts || !xs || !row_offsets || !G || !Bmat || !LLT || !chunk_offsets || !chunk_series || !series_chunks || !ws ||
      !pred_mean || !pred_cov || !logpdf || !z_mean || !z_cov || !loglik || !m_end || !P_end || !info)
    return fail(CGPS_ERR_ARG, "cgps_leg_filter_scan: null pointer");
  const FilterScanWs w = filter_scan_ws(n_chunks, M, d, dtype == CGPS_F32 ? 4 : 8, fanout);
  if (ws_bytes < w.total)
    return fail(CGPS_ERR_ARG, "cgps_leg_filter_scan: workspace of %zu bytes, %zu needed", ws_bytes, w.total);
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_leg_filter_scan", {{"ws", ws, ALIGN_WS}})) return rc;
    (void)hipMemsetAsync(info, 0, sizeof(int), (hipStream_t)stream);
    cgps::launch_filter_scan<T, D>((const T*)ts, (const T*)xs, pattern, (const T*)noise_var, B, R, M, (const T*)G,
                                   (const T*)Bmat, (const T*)LLT, obs, (const T*)t0, (const T*)m0, (const T*)P0,
                                   chunk_offsets, chunk_series, series_chunks, n_chunks, fanout, (char*)ws, w,
                                   (T*)pred_mean, (T*)pred_cov, (T*)logpdf, (T*)z_mean, (T*)z_cov, loglik, (T*)m_end,
                                   (T*)P_end, info, (hipStream_t)stream);
    return check_launch("LEG time-parallel filter");
  });
}

}  // extern "C"
