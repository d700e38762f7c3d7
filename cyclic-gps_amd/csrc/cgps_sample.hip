// cgps_sample.hip -- counter-based standard normals, samples from N(mean, J^-1) off a stored factor, and the
// perturbed right-hand sides of the batched LEG draws, for one model and for many (cgps_leg_perturb.h), and replicated
// observations given latent paths (cgps_leg_replicate.h)
// One translation unit of libcgps (include/cgps.h); host code only decides sizes/offsets and
// enqueues kernels on the caller's stream: nothing here allocates, copies to the host or synchronises.
#include "cgps_host.h"
#include "cgps_leg_perturb.h"
#include "cgps_leg_replicate.h"
#include "cgps_sample_tile.h"

using namespace cgps_host;

namespace cgps {
// out [rows][cols]: one lane per (row, column group)
template <typename T>
__global__ __launch_bounds__(256) void normal_fill_kernel(T* __restrict__ out, int64_t rows, int64_t cols, int64_t groups,
                                                          uint64_t seed, uint32_t stream) {
  constexpr int GC = RngGroup<T>::COLS;
  const int64_t items = rows * groups, step = (int64_t)gridDim.x * blockDim.x;
  for (int64_t it = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += step) {
    const int64_t r = it / groups, g = it - r * groups;
    T z[GC];
    normal_group(seed, stream, (uint64_t)r, (uint32_t)g, z);
    T* p = out + r * cols + g * GC;
#pragma unroll
    for (int u = 0; u < GC; ++u)
      if (g * GC + u < cols) p[u] = z[u];
  }
}
}  // namespace cgps

namespace {
template <typename T>
int run_normal_fill(T* out, int64_t rows, int64_t cols, uint64_t seed, uint32_t stream_id, hipStream_t st) {
  constexpr int GC = cgps::RngGroup<T>::COLS;
  const int64_t groups = (cols + GC - 1) / GC;
  if (groups > (int64_t)1 << 32) return fail(CGPS_ERR_ARG, "cgps_normal_fill: more than 2^32 column groups");
  const int64_t blocks = (rows * groups + 255) / 256, cap = (int64_t)1 << 20;
  hipLaunchKernelGGL((cgps::normal_fill_kernel<T>), dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, st, out, rows,
                     cols, groups, seed, stream_id);
  return check_launch("normal fill");
}

template <typename T, int D, int MC>
int run_sample(const T* Dp, const T* Fp, const T* Gp, int64_t N, int64_t nrhs, const T* mean, uint64_t seed, uint32_t stream_id,
               T* x, char* ws, size_t ws_bytes, hipStream_t st) {
  constexpr int TSL = cgps::solve_m_tile_log2<MC>(), NT = (1 << TSL) / 2, CS = cgps::solve_m_col_splits<MC>();
  const SampleWs w = sample_ws(N, D, sizeof(T), nrhs);
  if (ws_bytes < w.total) return fail(CGPS_ERR_ARG, "workspace too small: %zu < %zu", ws_bytes, w.total);
  const size_t lds = cgps::solve_m_lds_bytes<T, D, MC>();
  static PerDevice<int> done;
  done.get([&](int) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cgps::sample_tile_m_kernel<T, D, MC>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    return 1;
  });
  Layout L;
  make_layout(N, L);
  SolvePasses P;                    // the one regular kernel form for every pass (no latency-bound variants)
  plan_panel_sweep(L, P, MC, false, false);
  T* bufs[2] = {at<T>(ws, w.buf[0]), at<T>(ws, w.buf[1])};
  const size_t slice[2] = {w.slice[0] / sizeof(T), w.slice[1] / sizeof(T)};
  for (int64_t c = 0; c < w.chunks; c += w.group) {        // one group unless nrhs > 8 SAMPLE_CHUNK_GROUP
    const int64_t gc = w.chunks - c < w.group ? w.chunks - c : w.group, col0 = c * MC;
    const T* xc = nullptr;
    size_t xc_stride = 0;
    for (int p = P.np - 1; p >= 0; --p) {
      const bool last = p == 0;
      T* X = last ? x + col0 : bufs[P.buf(p)];
      const size_t stride = last ? (size_t)MC : slice[P.buf(p)];
      hipLaunchKernelGGL((cgps::sample_tile_m_kernel<T, D, MC>), dim3((unsigned)P.tiles[p], (unsigned)gc), dim3(NT * CS), lds, st,
                         Dp, Fp, Gp, P.lv[p], seed, stream_id, col0, nrhs, xc, xc_stride, P.rows[p], X, stride,
                         last ? nrhs : (int64_t)MC, last ? mean : nullptr);
      xc = X;
      xc_stride = stride;
    }
  }
  return check_launch("sample");
}

template <typename T, int D, int HSRC>
int run_perturbation(const T* ts, int64_t R, const T* G, const int64_t* roff, const int64_t* ids, int64_t B, const T* hterm,
                     int entries, int obs, const unsigned char* rows, const T* v, int64_t nrhs, uint64_t seed,
                     uint32_t stream_id, T* out, int* info, hipStream_t st) {
  constexpr int GC = cgps::RngGroup<T>::COLS;
  const int64_t groups = (nrhs + GC - 1) / GC, nb = (R + cgps::LEG_THREADS - 1) / cgps::LEG_THREADS;
  const int64_t chunks = (groups + cgps::PERT_CHUNK_GROUPS - 1) / cgps::PERT_CHUNK_GROUPS;
  (void)hipMemsetAsync(info, 0, sizeof(int), st);
  hipLaunchKernelGGL((cgps::leg_perturbation_kernel<T, D, HSRC>), dim3((unsigned)nb, (unsigned)(chunks < 65535 ? chunks : 65535)),
                     dim3(cgps::LEG_THREADS), 0, st, ts, R, G, roff, ids, B, hterm, entries, obs, rows, v, nrhs, groups, seed,
                     stream_id, out, info);
  return check_launch("leg_perturbation_seg");
}

template <typename T, int D, int HSRC>
int run_perturbation_models(const T* ts, int64_t R, int64_t M, const T* G, const int64_t* roff, const int64_t* ids, int64_t B,
                            const T* hterm, int entries, int obs, const unsigned char* rows, const T* v, int64_t nrhs,
                            uint64_t seed, const int64_t* stream_ids, T* out, int* info, hipStream_t st) {
  constexpr int GC = cgps::RngGroup<T>::COLS;
  const int64_t groups = (nrhs + GC - 1) / GC, nb = (R + cgps::LEG_THREADS - 1) / cgps::LEG_THREADS;
  const int64_t chunks = (groups + cgps::PERT_CHUNK_GROUPS - 1) / cgps::PERT_CHUNK_GROUPS;
  const size_t hstride = (size_t)D * obs * (HSRC == cgps::PERT_H_TABLE ? (size_t)entries : HSRC == cgps::PERT_H_ROWS ? (size_t)R : 1);
  (void)hipMemsetAsync(info, 0, sizeof(int), st);
  hipLaunchKernelGGL((cgps::leg_perturbation_models_kernel<T, D, HSRC>),
                     dim3((unsigned)nb, (unsigned)(chunks < 65535 ? chunks : 65535), (unsigned)M), dim3(cgps::LEG_THREADS), 0, st,
                     ts, R, G, roff, ids, B, hterm, hstride, entries, obs, rows, v, nrhs, groups, seed, stream_ids, out, info);
  return check_launch("leg_perturbation_models");
}

template <typename T>
int run_observations(const T* z, const uint8_t* pattern, const T* noise, const int64_t* roff, const int64_t* ids, int64_t B,
                     int64_t R, int64_t M, const T* Bmat, const T* LLT, int d, int obs, int64_t nrhs, uint64_t seed,
                     const int64_t* stream_ids, T* x, int* info, hipStream_t st) {
  constexpr int GC = cgps::RngGroup<T>::COLS;
  const int64_t groups = (nrhs + GC - 1) / GC, nb = (R + cgps::LEG_THREADS - 1) / cgps::LEG_THREADS;
  const int64_t chunks = (groups + cgps::REPL_CHUNK_GROUPS - 1) / cgps::REPL_CHUNK_GROUPS;
  const dim3 grid((unsigned)nb, (unsigned)(chunks < 65535 ? chunks : 65535), (unsigned)M), block(cgps::LEG_THREADS);
  (void)hipMemsetAsync(info, 0, sizeof(int), st);
  dispatch_obs(obs, [&](auto oc) {
    hipLaunchKernelGGL((cgps::leg_observations_kernel<T, decltype(oc)::value>), grid, block, 0, st, z, R, d, Bmat, LLT, obs,
                       pattern, noise, roff, ids, B, nrhs, groups, seed, stream_ids, x, info);
  });
  return check_launch("leg_observations");
}
}  // namespace

extern "C" {

int cgps_normal_fill(void* out, int64_t rows, int64_t cols, int dtype, uint64_t seed, uint32_t stream_id, void* stream) {
  if (!out || rows < 1 || cols < 1) return fail(CGPS_ERR_ARG, "cgps_normal_fill: null pointer, rows < 1 or cols < 1");
  if (dtype == CGPS_F32) return run_normal_fill<float>((float*)out, rows, cols, seed, stream_id, (hipStream_t)stream);
  if (dtype == CGPS_F64) return run_normal_fill<double>((double*)out, rows, cols, seed, stream_id, (hipStream_t)stream);
  return fail(CGPS_ERR_UNSUPPORTED, "dtype %d not supported", dtype);
}

int cgps_sample_workspace_bytes(int64_t N, int d, int dtype, int64_t nrhs, size_t* bytes) {
  if (bad_common(N, d) || !bytes || nrhs < 1) return fail(CGPS_ERR_ARG, "cgps_sample_workspace_bytes: bad argument");
  if (d > 8) return fail(CGPS_ERR_UNSUPPORTED, "block size d=%d outside 1..8", d);
  if (dtype != CGPS_F32 && dtype != CGPS_F64) return fail(CGPS_ERR_UNSUPPORTED, "dtype %d not supported", dtype);
  *bytes = sample_ws(N, d, dtype == CGPS_F32 ? 4 : 8, nrhs).total;
  return CGPS_OK;
}

int cgps_sample(const void* Dp, const void* Fp, const void* Gp, int64_t N, int d, int dtype, int64_t nrhs, const void* mean,
                uint64_t seed, uint32_t stream_id, void* x, void* ws, size_t ws_bytes, void* stream) {
  if (bad_common(N, d) || nrhs < 1 || !Dp || !Fp || !Gp || !x || !ws)
    return fail(CGPS_ERR_ARG, "cgps_sample: null pointer, N < 1 or nrhs < 1");
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_sample", {{"Dp", Dp, ALIGN_VEC}, {"Fp", Fp, ALIGN_VEC}, {"Gp", Gp, ALIGN_VEC},
                                                 {"mean", mean, ALIGN_VEC}, {"x", x, ALIGN_VEC}, {"ws", ws, ALIGN_WS}}))
      return rc;
    switch (cgps::panel_width(nrhs > 8 ? 8 : (int)nrhs)) {
      case 2: return run_sample<T, D, 2>((const T*)Dp, (const T*)Fp, (const T*)Gp, N, nrhs, (const T*)mean, seed, stream_id, (T*)x,
                                         (char*)ws, ws_bytes, (hipStream_t)stream);
      case 4: return run_sample<T, D, 4>((const T*)Dp, (const T*)Fp, (const T*)Gp, N, nrhs, (const T*)mean, seed, stream_id, (T*)x,
                                         (char*)ws, ws_bytes, (hipStream_t)stream);
      default: return run_sample<T, D, 8>((const T*)Dp, (const T*)Fp, (const T*)Gp, N, nrhs, (const T*)mean, seed, stream_id, (T*)x,
                                          (char*)ws, ws_bytes, (hipStream_t)stream);
    }
  });
}

int cgps_leg_perturbation_seg(const void* ts, int64_t R, const void* G, int d, int dtype, const int64_t* row_offsets,
                              const int64_t* series_ids, int64_t B, int hsource, const void* hterm, int entries, int obs,
                              const unsigned char* rows, const void* v, int64_t nrhs, uint64_t seed, uint32_t stream_id,
                              void* out, int* info, void* stream) {
  if (B < 0 || R < 0) return fail(CGPS_ERR_ARG, "cgps_leg_perturbation_seg: B < 0 or R < 0");
  if (B == 0 || R == 0) return CGPS_OK;
  if (d < 1 || nrhs < 1 || !ts || !G || !row_offsets || !series_ids || !out || !info)
    return fail(CGPS_ERR_ARG, "cgps_leg_perturbation_seg: null pointer, d < 1 or nrhs < 1");
  if (hsource < CGPS_H_NONE || hsource > CGPS_H_ROWS)
    return fail(CGPS_ERR_ARG, "cgps_leg_perturbation_seg: hsource = %d, outside 0..3", hsource);
  if (hsource != CGPS_H_NONE && (!hterm || obs < 1 || obs > 8))
    return fail(CGPS_ERR_ARG, "cgps_leg_perturbation_seg: null hterm or obs = %d outside 1..8", obs);
  if (hsource == CGPS_H_TABLE && (!rows || entries < 1 || entries > 256))
    return fail(CGPS_ERR_ARG, "cgps_leg_perturbation_seg: null pattern or %d table entries, outside 1..256", entries);
  if (B > 0x7fffffffLL || (R + cgps::LEG_THREADS - 1) / cgps::LEG_THREADS > 0x7fffffffLL)
    return fail(CGPS_ERR_ARG, "cgps_leg_perturbation_seg: B = %lld series or R = %lld rows, too many for one launch",
                (long long)B, (long long)R);
  if (nrhs > (int64_t)1 << 32) return fail(CGPS_ERR_ARG, "cgps_leg_perturbation_seg: more than 2^32 columns");
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    auto run = [&](auto hs) {
      return run_perturbation<T, D, decltype(hs)::value>((const T*)ts, R, (const T*)G, row_offsets, series_ids, B, (const T*)hterm,
                                                         entries, obs, rows, (const T*)v, nrhs, seed, stream_id, (T*)out, info,
                                                         (hipStream_t)stream);
    };
    switch (hsource) {
      case CGPS_H_NONE: return run(std::integral_constant<int, cgps::PERT_H_NONE>{});
      case CGPS_H_PLAIN: return run(std::integral_constant<int, cgps::PERT_H_PLAIN>{});
      case CGPS_H_TABLE: return run(std::integral_constant<int, cgps::PERT_H_TABLE>{});
      default: return run(std::integral_constant<int, cgps::PERT_H_ROWS>{});
    }
  });
}

int cgps_leg_perturbation_models(const void* ts, int64_t R, int64_t M, const void* G, int d, int dtype,
                                 const int64_t* row_offsets, const int64_t* series_ids, int64_t B, int hsource,
                                 const void* hterm, int entries, int obs, const unsigned char* rows, const void* v, int64_t nrhs,
                                 uint64_t seed, const int64_t* stream_ids, void* out, int* info, void* stream) {
  if (B < 0 || R < 0) return fail(CGPS_ERR_ARG, "cgps_leg_perturbation_models: B < 0 or R < 0");
  if (M < 1 || M > 65535) return fail(CGPS_ERR_ARG, "cgps_leg_perturbation_models: M = %lld models, outside 1..65535", (long long)M);
  if (B == 0 || R == 0) return CGPS_OK;
  if (nrhs < 1 || !ts || !G || !row_offsets || !series_ids || !stream_ids || !out || !info)
    return fail(CGPS_ERR_ARG, "cgps_leg_perturbation_models: null pointer or nrhs < 1");
  if (hsource < CGPS_H_NONE || hsource > CGPS_H_ROWS)
    return fail(CGPS_ERR_ARG, "cgps_leg_perturbation_models: hsource = %d, outside 0..3", hsource);
  if (hsource != CGPS_H_NONE && (!hterm || obs < 1 || obs > 8))
    return fail(CGPS_ERR_ARG, "cgps_leg_perturbation_models: null hterm or obs = %d outside 1..8", obs);
  if (hsource == CGPS_H_TABLE && (!rows || entries < 1 || entries > 256))
    return fail(CGPS_ERR_ARG, "cgps_leg_perturbation_models: null pattern or %d table entries, outside 1..256", entries);
  if (B > 0x7fffffffLL || (R + cgps::LEG_THREADS - 1) / cgps::LEG_THREADS > 0x7fffffffLL)
    return fail(CGPS_ERR_ARG, "cgps_leg_perturbation_models: B = %lld series or R = %lld rows, too many for one launch",
                (long long)B, (long long)R);
  if (nrhs > (int64_t)1 << 32) return fail(CGPS_ERR_ARG, "cgps_leg_perturbation_models: more than 2^32 columns");
  if (d < 1 || d > 8) return fail(CGPS_ERR_UNSUPPORTED, "cgps_leg_perturbation_models: block size d=%d outside 1..8", d);
  if (dtype != CGPS_F32 && dtype != CGPS_F64) return fail(CGPS_ERR_UNSUPPORTED, "dtype %d not supported", dtype);
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    auto run = [&](auto hs) {
      return run_perturbation_models<T, D, decltype(hs)::value>((const T*)ts, R, M, (const T*)G, row_offsets, series_ids, B,
                                                                (const T*)hterm, entries, obs, rows, (const T*)v, nrhs, seed,
                                                                stream_ids, (T*)out, info, (hipStream_t)stream);
    };
    switch (hsource) {
      case CGPS_H_NONE: return run(std::integral_constant<int, cgps::PERT_H_NONE>{});
      case CGPS_H_PLAIN: return run(std::integral_constant<int, cgps::PERT_H_PLAIN>{});
      case CGPS_H_TABLE: return run(std::integral_constant<int, cgps::PERT_H_TABLE>{});
      default: return run(std::integral_constant<int, cgps::PERT_H_ROWS>{});
    }
  });
}

int cgps_leg_observations(const void* z, const uint8_t* pattern, const void* noise_var, const int64_t* row_offsets,
                          const int64_t* series_ids, int64_t B, int64_t R, int64_t M, const void* Bmat, const void* LLT, int d,
                          int obs, int dtype, int64_t nrhs, uint64_t seed, const int64_t* stream_ids, void* x, int* info,
                          void* stream) {
  if (B < 0 || R < 0) return fail(CGPS_ERR_ARG, "cgps_leg_observations: B = %lld series, R = %lld rows", (long long)B, (long long)R);
  if (M < 1 || M > 65535) return fail(CGPS_ERR_ARG, "cgps_leg_observations: M = %lld models, outside 1..65535", (long long)M);
  if (B == 0 || R == 0) return CGPS_OK;
  if (nrhs < 1 || !z || !row_offsets || !series_ids || !Bmat || !LLT || !stream_ids || !x || !info)
    return fail(CGPS_ERR_ARG, "cgps_leg_observations: null pointer or nrhs < 1");
  if (B > 0x7fffffffLL || (R + cgps::LEG_THREADS - 1) / cgps::LEG_THREADS > 0x7fffffffLL)
    return fail(CGPS_ERR_ARG, "cgps_leg_observations: B = %lld series or R = %lld rows, too many for one launch", (long long)B,
                (long long)R);
  if (nrhs > (int64_t)1 << 32) return fail(CGPS_ERR_ARG, "cgps_leg_observations: more than 2^32 columns");
  if (d < 1 || d > 8) return fail(CGPS_ERR_UNSUPPORTED, "cgps_leg_observations: d = %d outside 1..8", d);
  if (obs < 1 || obs > 8) return fail(CGPS_ERR_UNSUPPORTED, "cgps_leg_observations: obs = %d outside 1..8", obs);
  if (dtype != CGPS_F32 && dtype != CGPS_F64) return fail(CGPS_ERR_UNSUPPORTED, "dtype %d not supported", dtype);
  if (dtype == CGPS_F32)
    return run_observations<float>((const float*)z, pattern, (const float*)noise_var, row_offsets, series_ids, B, R, M,
                                   (const float*)Bmat, (const float*)LLT, d, obs, nrhs, seed, stream_ids, (float*)x, info,
                                   (hipStream_t)stream);
  return run_observations<double>((const double*)z, pattern, (const double*)noise_var, row_offsets, series_ids, B, R, M,
                                  (const double*)Bmat, (const double*)LLT, d, obs, nrhs, seed, stream_ids, (double*)x, info,
                                  (hipStream_t)stream);
}

}  // extern "C"
