// cgps_leg.hip -- operand assembly for LEG models
// One translation unit of libcgps (include/cgps.h); host code only decides sizes/offsets and
// enqueues kernels on the caller's stream: nothing here allocates, copies to the host or synchronises.
#include "cgps_host.h"
#include "cgps_leg.h"

using namespace cgps_host;

extern "C" {

int cgps_peg_precision(const void* ts, const void* G, int64_t N, int d, int dtype, void* Rs, void* Os, int* info,
                       void* stream) {
  if (bad_common(N, d) || !ts || !G || !Rs || (N > 1 && !Os) || !info)
    return fail(CGPS_ERR_ARG, "cgps_peg_precision: null pointer or N < 1");
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_peg_precision", {{"ts", ts, elem_bytes(dtype)}, {"G", G, elem_bytes(dtype)}, {"Rs", Rs, ALIGN_VEC}, {"Os", Os, ALIGN_VEC}, {"info", info, 4}})) return rc;
    hipStream_t st = (hipStream_t)stream;
    (void)hipMemsetAsync(info, 0, sizeof(int), st);
    const int64_t nb = (N + cgps::LEG_THREADS - 1) / cgps::LEG_THREADS;
    hipLaunchKernelGGL((cgps::peg_precision_kernel<T, D>), dim3((unsigned)nb), dim3(cgps::LEG_THREADS), 0, st,
                       (const T*)ts, (const T*)G, N, (T*)Rs, (T*)Os, info);
    return check_launch("peg_precision");
  });
}

int cgps_peg_precision_adjoint(const void* ts, const void* G, int64_t N, int d, int dtype, const void* gRs,
                               const void* gOs, void* gG_partial, void* gtau, void* stream) {
  if (bad_common(N, d) || N < 2 || !ts || !G || !gRs || !gOs || !gG_partial)
    return fail(CGPS_ERR_ARG, "cgps_peg_precision_adjoint: null pointer or N < 2");
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_peg_precision_adjoint", {{"ts", ts, elem_bytes(dtype)}, {"G", G, elem_bytes(dtype)}, {"gRs", gRs, ALIGN_VEC}, {"gOs", gOs, ALIGN_VEC}, {"gG_partial", gG_partial, elem_bytes(dtype)}, {"gtau", gtau, elem_bytes(dtype)}})) return rc;
    const int64_t nb = (N - 1 + cgps::LEG_THREADS - 1) / cgps::LEG_THREADS;
    hipLaunchKernelGGL((cgps::peg_precision_adjoint_kernel<T, D>), dim3((unsigned)nb), dim3(cgps::LEG_THREADS), 0,
                       (hipStream_t)stream, (const T*)ts, (const T*)G, N, (const T*)gRs, (const T*)gOs, (T*)gG_partial,
                       (T*)gtau);
    return check_launch("peg_precision_adjoint");
  });
}

int cgps_peg_precision_seg(const void* ts, const void* G, const unsigned char* cut, int64_t N, int d, int dtype, void* Rs,
                           void* Os, int* info, void* stream) {
  if (bad_common(N, d) || !ts || !G || (N > 1 && (!Os || !cut)) || !Rs || !info)
    return fail(CGPS_ERR_ARG, "cgps_peg_precision_seg: null pointer or N < 1");
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_peg_precision_seg", {{"ts", ts, elem_bytes(dtype)}, {"G", G, elem_bytes(dtype)}, {"Rs", Rs, ALIGN_VEC}, {"Os", Os, ALIGN_VEC}, {"info", info, 4}})) return rc;
    hipStream_t st = (hipStream_t)stream;
    (void)hipMemsetAsync(info, 0, sizeof(int), st);
    const int64_t nb = (N + cgps::LEG_THREADS - 1) / cgps::LEG_THREADS;
    hipLaunchKernelGGL((cgps::peg_precision_kernel<T, D>), dim3((unsigned)nb), dim3(cgps::LEG_THREADS), 0, st,
                       (const T*)ts, (const T*)G, N, (T*)Rs, (T*)Os, info, cut);
    return check_launch("peg_precision_seg");
  });
}

int cgps_peg_precision_adjoint_seg(const void* ts, const void* G, const unsigned char* cut, int64_t N, int d, int dtype,
                                   const void* gRs, const void* gOs, void* gG_partial, void* gtau, void* stream) {
  if (bad_common(N, d) || N < 2 || !ts || !G || !cut || !gRs || !gOs || !gG_partial)
    return fail(CGPS_ERR_ARG, "cgps_peg_precision_adjoint_seg: null pointer or N < 2");
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_peg_precision_adjoint_seg", {{"ts", ts, elem_bytes(dtype)}, {"G", G, elem_bytes(dtype)}, {"gRs", gRs, ALIGN_VEC}, {"gOs", gOs, ALIGN_VEC}, {"gG_partial", gG_partial, elem_bytes(dtype)}, {"gtau", gtau, elem_bytes(dtype)}})) return rc;
    const int64_t nb = (N - 1 + cgps::LEG_THREADS - 1) / cgps::LEG_THREADS;
    hipLaunchKernelGGL((cgps::peg_precision_adjoint_kernel<T, D>), dim3((unsigned)nb), dim3(cgps::LEG_THREADS), 0,
                       (hipStream_t)stream, (const T*)ts, (const T*)G, N, (const T*)gRs, (const T*)gOs, (T*)gG_partial,
                       (T*)gtau, cut);
    return check_launch("peg_precision_adjoint_seg");
  });
}

int cgps_peg_precision_models(const void* ts, const void* G, const unsigned char* cut, int64_t R, int64_t M, int d, int dtype,
                              void* Rs, void* Os, int* info, void* stream) {
  if (M < 1 || M > 65535) return fail(CGPS_ERR_ARG, "cgps_peg_precision_models: M = %lld models, outside 1..65535", (long long)M);
  if (bad_common(R, d) || !ts || !G || !Rs || (M * R > 1 && !Os) || !info)
    return fail(CGPS_ERR_ARG, "cgps_peg_precision_models: null pointer or R < 1");
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_peg_precision_models", {{"ts", ts, elem_bytes(dtype)}, {"G", G, elem_bytes(dtype)}, {"Rs", Rs, ALIGN_VEC}, {"Os", Os, ALIGN_VEC}, {"info", info, 4}})) return rc;
    if constexpr (!cgps::peg_models_supported<T, D>()) {
      return fail(CGPS_ERR_UNSUPPORTED, "cgps_peg_precision_models: not built for this block size (d = 8, fp64 d = 6)");
    } else {
      hipStream_t st = (hipStream_t)stream;
      const int64_t nb = (R + cgps::LEG_THREADS - 1) / cgps::LEG_THREADS;
      if (nb > 0x7fffffffLL) return fail(CGPS_ERR_ARG, "cgps_peg_precision_models: R = %lld rows, too many for one launch", (long long)R);
      (void)hipMemsetAsync(info, 0, sizeof(int), st);
      hipLaunchKernelGGL((cgps::peg_precision_kernel<T, D, cgps::PEG_TERM_NONE, true>), dim3((unsigned)nb, (unsigned)M),
                         dim3(cgps::LEG_THREADS), 0, st, (const T*)ts, (const T*)G, R, (T*)Rs, (T*)Os, info, cut);
      return check_launch("peg_precision_models");
    }
  });
}

int cgps_peg_precision_adjoint_models(const void* ts, const void* G, const unsigned char* cut, int64_t R, int64_t M, int d,
                                      int dtype, const void* gRs, const void* gOs, void* gG_partial, void* gtau,
                                      void* stream) {
  if (M < 1 || M > 65535)
    return fail(CGPS_ERR_ARG, "cgps_peg_precision_adjoint_models: M = %lld models, outside 1..65535", (long long)M);
  if (bad_common(R, d) || R < 2 || !ts || !G || !gRs || !gOs || !gG_partial)
    return fail(CGPS_ERR_ARG, "cgps_peg_precision_adjoint_models: null pointer or R < 2");
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_peg_precision_adjoint_models", {{"ts", ts, elem_bytes(dtype)}, {"G", G, elem_bytes(dtype)}, {"gRs", gRs, ALIGN_VEC}, {"gOs", gOs, ALIGN_VEC}, {"gG_partial", gG_partial, elem_bytes(dtype)}, {"gtau", gtau, elem_bytes(dtype)}})) return rc;
    if constexpr (!cgps::peg_models_supported<T, D>()) {
      return fail(CGPS_ERR_UNSUPPORTED, "cgps_peg_precision_adjoint_models: not built for this block size (d = 8, fp64 d = 6)");
    } else {
      const int64_t nb = (R - 1 + cgps::LEG_THREADS - 1) / cgps::LEG_THREADS;
      if (nb > 0x7fffffffLL)
        return fail(CGPS_ERR_ARG, "cgps_peg_precision_adjoint_models: R = %lld rows, too many for one launch", (long long)R);
      hipLaunchKernelGGL((cgps::peg_precision_adjoint_kernel<T, D, true>), dim3((unsigned)nb, (unsigned)M),
                         dim3(cgps::LEG_THREADS), 0, (hipStream_t)stream, (const T*)ts, (const T*)G, R, (const T*)gRs,
                         (const T*)gOs, (T*)gG_partial, (T*)gtau, cut);
      return check_launch("peg_precision_adjoint_models");
    }
  });
}

int cgps_leg_intercast(const void* ts, int64_t n, const void* target_ts, int64_t p, const void* G, int d, int dtype,
                       const void* ip_mean, const void* ip_cov_diag, const void* ip_cov_offdiag, void* out_mean,
                       void* out_cov, void* stream) {
  if (bad_common(n, d) || p < 0 || !ts || !G || !ip_mean || !ip_cov_diag || (n > 1 && !ip_cov_offdiag) ||
      (p > 0 && (!target_ts || !out_mean || !out_cov)))
    return fail(CGPS_ERR_ARG, "cgps_leg_intercast: null pointer, n < 1 or p < 0");
  if (p == 0) return CGPS_OK;
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_leg_intercast", {{"ts", ts, elem_bytes(dtype)}, {"target_ts", target_ts, elem_bytes(dtype)}, {"G", G, elem_bytes(dtype)}, {"ip_mean", ip_mean, elem_bytes(dtype)}, {"ip_cov_diag", ip_cov_diag, ALIGN_VEC}, {"ip_cov_offdiag", ip_cov_offdiag, ALIGN_VEC}, {"out_mean", out_mean, elem_bytes(dtype)}, {"out_cov", out_cov, ALIGN_VEC}})) return rc;
    const int64_t nb = (p + cgps::LEG_THREADS - 1) / cgps::LEG_THREADS;
    hipLaunchKernelGGL((cgps::leg_intercast_kernel<T, D>), dim3((unsigned)nb), dim3(cgps::LEG_THREADS), 0,
                       (hipStream_t)stream, (const T*)ts, n, (const T*)target_ts, p, (const T*)G, (const T*)ip_mean,
                       (const T*)ip_cov_diag, (const T*)ip_cov_offdiag, (T*)out_mean, (T*)out_cov);
    return check_launch("leg_intercast");
  });
}

int cgps_leg_intercast_seg(const void* ts, const int64_t* row_offsets, const void* target_ts, const int64_t* target_offsets,
                           int64_t B, int64_t P, const void* G, int d, int dtype, const void* ip_mean,
                           const void* ip_cov_diag, const void* ip_cov_offdiag, void* out_mean, void* out_cov,
                           void* stream) {
  if (B < 0 || P < 0) return fail(CGPS_ERR_ARG, "cgps_leg_intercast_seg: B < 0 or P < 0");
  if (B == 0 || P == 0) return CGPS_OK;
  // (ip_cov_offdiag may be null: a batch of one one-row series has no off-diagonal block)
  if (!ts || !row_offsets || !target_ts || !target_offsets || !G || !ip_mean || !ip_cov_diag || !out_mean || !out_cov)
    return fail(CGPS_ERR_ARG, "cgps_leg_intercast_seg: null pointer");
  if (B > 0x7fffffffLL) return fail(CGPS_ERR_ARG, "cgps_leg_intercast_seg: B = %lld series, at most 2^31 - 1", (long long)B);
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_leg_intercast_seg", {{"ts", ts, elem_bytes(dtype)}, {"row_offsets", row_offsets, 8}, {"target_ts", target_ts, elem_bytes(dtype)}, {"target_offsets", target_offsets, 8}, {"G", G, elem_bytes(dtype)}, {"ip_mean", ip_mean, elem_bytes(dtype)}, {"ip_cov_diag", ip_cov_diag, ALIGN_VEC}, {"ip_cov_offdiag", ip_cov_offdiag, ALIGN_VEC}, {"out_mean", out_mean, elem_bytes(dtype)}, {"out_cov", out_cov, ALIGN_VEC}})) return rc;
    const int64_t nb = (P + cgps::LEG_THREADS - 1) / cgps::LEG_THREADS;
    if (nb > 0x7fffffffLL) return fail(CGPS_ERR_ARG, "cgps_leg_intercast_seg: P = %lld targets, too many for one launch", (long long)P);
    hipLaunchKernelGGL((cgps::leg_intercast_seg_kernel<T, D>), dim3((unsigned)nb), dim3(cgps::LEG_THREADS), 0,
                       (hipStream_t)stream, (const T*)ts, row_offsets, (const T*)target_ts, target_offsets, B, P,
                       (const T*)G, (const T*)ip_mean, (const T*)ip_cov_diag, (const T*)ip_cov_offdiag, (T*)out_mean,
                       (T*)out_cov);
    return check_launch("leg_intercast_seg");
  });
}

int cgps_leg_posterior_blocks_seg(const void* ts, const void* G, const unsigned char* cut, int64_t N, int d, int dtype,
                                  int source, const void* term, int entries, const void* rows, void* K_Rs, void* Os,
                                  int* info, void* stream) {
  if (bad_common(N, d) || !ts || !G || !term || !K_Rs || (N > 1 && !Os) || !info)
    return fail(CGPS_ERR_ARG, "cgps_leg_posterior_blocks_seg: null pointer or N < 1");
  if (source < CGPS_ROWS_PLAIN || source > CGPS_ROWS_WEIGHTED)
    return fail(CGPS_ERR_ARG, "cgps_leg_posterior_blocks_seg: source = %d, outside 0..2", source);
  if (source != CGPS_ROWS_PLAIN && !rows) return fail(CGPS_ERR_ARG, "cgps_leg_posterior_blocks_seg: null pattern or weights");
  if (source == CGPS_ROWS_TABLE && (entries < 1 || entries > 256))
    return fail(CGPS_ERR_ARG, "cgps_leg_posterior_blocks_seg: %d table entries, outside 1..256", entries);
  if (source == CGPS_ROWS_WEIGHTED && (entries < 1 || entries > 64))
    return fail(CGPS_ERR_ARG, "cgps_leg_posterior_blocks_seg: Kb = %d basis blocks, outside 1..64", entries);
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_leg_posterior_blocks_seg", {{"ts", ts, elem_bytes(dtype)}, {"G", G, elem_bytes(dtype)}, {"term", term, ALIGN_VEC}, {"K_Rs", K_Rs, ALIGN_VEC}, {"Os", Os, ALIGN_VEC}, {"info", info, 4}})) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = (N + cgps::LEG_THREADS - 1) / cgps::LEG_THREADS;
    if (nb > 0x7fffffffLL) return fail(CGPS_ERR_ARG, "cgps_leg_posterior_blocks_seg: N = %lld rows, too many for one launch", (long long)N);
    (void)hipMemsetAsync(info, 0, sizeof(int), st);
    const dim3 grid((unsigned)nb), block(cgps::LEG_THREADS);
    if (source == CGPS_ROWS_PLAIN)
      hipLaunchKernelGGL((cgps::peg_precision_kernel<T, D, cgps::PEG_TERM_PLAIN>), grid, block, 0, st, (const T*)ts, (const T*)G,
                         N, (T*)K_Rs, (T*)Os, info, cut, (const T*)term, rows, entries);
    else if (source == CGPS_ROWS_TABLE)
      hipLaunchKernelGGL((cgps::peg_precision_kernel<T, D, cgps::PEG_TERM_TABLE>), grid, block, 0, st, (const T*)ts, (const T*)G,
                         N, (T*)K_Rs, (T*)Os, info, cut, (const T*)term, rows, entries);
    else
      hipLaunchKernelGGL((cgps::peg_precision_kernel<T, D, cgps::PEG_TERM_WEIGHTED>), grid, block, 0, st, (const T*)ts,
                         (const T*)G, N, (T*)K_Rs, (T*)Os, info, cut, (const T*)term, rows, entries);
    return check_launch("leg_posterior_blocks_seg");
  });
}

int cgps_leg_posterior_blocks_models(const void* ts, const void* G, const unsigned char* cut, int64_t R, int64_t M, int d,
                                     int dtype, int source, const void* term, int entries, const void* rows, void* K_Rs,
                                     void* Os, int* info, void* stream) {
  if (M < 1 || M > 65535)
    return fail(CGPS_ERR_ARG, "cgps_leg_posterior_blocks_models: M = %lld models, outside 1..65535", (long long)M);
  if (bad_common(R, d) || !ts || !G || !term || !K_Rs || (M * R > 1 && !Os) || !info)
    return fail(CGPS_ERR_ARG, "cgps_leg_posterior_blocks_models: null pointer or R < 1");
  if (source < CGPS_ROWS_PLAIN || source > CGPS_ROWS_WEIGHTED)
    return fail(CGPS_ERR_ARG, "cgps_leg_posterior_blocks_models: source = %d, outside 0..2", source);
  if (source != CGPS_ROWS_PLAIN && !rows) return fail(CGPS_ERR_ARG, "cgps_leg_posterior_blocks_models: null pattern or weights");
  if (source == CGPS_ROWS_TABLE && (entries < 1 || entries > 256))
    return fail(CGPS_ERR_ARG, "cgps_leg_posterior_blocks_models: %d table entries, outside 1..256", entries);
  if (source == CGPS_ROWS_WEIGHTED && (entries < 1 || entries > 64))
    return fail(CGPS_ERR_ARG, "cgps_leg_posterior_blocks_models: Kb = %d basis blocks, outside 1..64", entries);
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_leg_posterior_blocks_models", {{"ts", ts, elem_bytes(dtype)}, {"G", G, elem_bytes(dtype)}, {"term", term, ALIGN_VEC}, {"K_Rs", K_Rs, ALIGN_VEC}, {"Os", Os, ALIGN_VEC}, {"info", info, 4}})) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t nb = (R + cgps::LEG_THREADS - 1) / cgps::LEG_THREADS;
    if (nb > 0x7fffffffLL)
      return fail(CGPS_ERR_ARG, "cgps_leg_posterior_blocks_models: R = %lld rows, too many for one launch", (long long)R);
    (void)hipMemsetAsync(info, 0, sizeof(int), st);
    const dim3 grid((unsigned)nb, (unsigned)M), block(cgps::LEG_THREADS);
    if (source == CGPS_ROWS_PLAIN)
      hipLaunchKernelGGL((cgps::peg_precision_kernel<T, D, cgps::PEG_TERM_PLAIN, true>), grid, block, 0, st, (const T*)ts,
                         (const T*)G, R, (T*)K_Rs, (T*)Os, info, cut, (const T*)term, rows, entries);
    else if (source == CGPS_ROWS_TABLE)
      hipLaunchKernelGGL((cgps::peg_precision_kernel<T, D, cgps::PEG_TERM_TABLE, true>), grid, block, 0, st, (const T*)ts,
                         (const T*)G, R, (T*)K_Rs, (T*)Os, info, cut, (const T*)term, rows, entries);
    else
      hipLaunchKernelGGL((cgps::peg_precision_kernel<T, D, cgps::PEG_TERM_WEIGHTED, true>), grid, block, 0, st, (const T*)ts,
                         (const T*)G, R, (T*)K_Rs, (T*)Os, info, cut, (const T*)term, rows, entries);
    return check_launch("leg_posterior_blocks_models");
  });
}

int cgps_leg_intercast_models(const void* ts, const int64_t* row_offsets, const void* target_ts, const int64_t* target_offsets,
                              int64_t B, int64_t P, int64_t M, const void* G, int d, int dtype, const void* ip_mean,
                              const void* ip_cov_diag, const void* ip_cov_offdiag, void* out_mean, void* out_cov,
                              void* stream) {
  if (M < 1 || M > 65535)
    return fail(CGPS_ERR_ARG, "cgps_leg_intercast_models: M = %lld models, outside 1..65535", (long long)M);
  if (B < 0 || P < 0) return fail(CGPS_ERR_ARG, "cgps_leg_intercast_models: B < 0 or P < 0");
  if (B == 0 || P == 0) return CGPS_OK;
  // (ip_cov_offdiag may be null: one model on a batch of one one-row series has no off-diagonal block)
  if (!ts || !row_offsets || !target_ts || !target_offsets || !G || !ip_mean || !ip_cov_diag || !out_mean || !out_cov)
    return fail(CGPS_ERR_ARG, "cgps_leg_intercast_models: null pointer");
  if (B > 0x7fffffffLL) return fail(CGPS_ERR_ARG, "cgps_leg_intercast_models: B = %lld series, at most 2^31 - 1", (long long)B);
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_leg_intercast_models", {{"ts", ts, elem_bytes(dtype)}, {"row_offsets", row_offsets, 8}, {"target_ts", target_ts, elem_bytes(dtype)}, {"target_offsets", target_offsets, 8}, {"G", G, elem_bytes(dtype)}, {"ip_mean", ip_mean, elem_bytes(dtype)}, {"ip_cov_diag", ip_cov_diag, ALIGN_VEC}, {"ip_cov_offdiag", ip_cov_offdiag, ALIGN_VEC}, {"out_mean", out_mean, elem_bytes(dtype)}, {"out_cov", out_cov, ALIGN_VEC}})) return rc;
    const int64_t nb = (P + cgps::LEG_THREADS - 1) / cgps::LEG_THREADS;
    if (nb > 0x7fffffffLL)
      return fail(CGPS_ERR_ARG, "cgps_leg_intercast_models: P = %lld targets, too many for one launch", (long long)P);
    hipLaunchKernelGGL((cgps::leg_intercast_seg_kernel<T, D, true>), dim3((unsigned)nb, (unsigned)M), dim3(cgps::LEG_THREADS),
                       0, (hipStream_t)stream, (const T*)ts, row_offsets, (const T*)target_ts, target_offsets, B, P,
                       (const T*)G, (const T*)ip_mean, (const T*)ip_cov_diag, (const T*)ip_cov_offdiag, (T*)out_mean,
                       (T*)out_cov);
    return check_launch("leg_intercast_models");
  });
}

}  // extern "C"
