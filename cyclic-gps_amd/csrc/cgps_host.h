// Host-side plumbing shared by the translation units of libcgps (one .hip file per group of
// entry points, so that the library builds in parallel): error string, dtype / block-size
// dispatch, per-device one-time setup.  Sizes, offsets and pass lists: cgps_plan.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <mutex>
#include <type_traits>

#include "../../include/cgps.h"
#include "cgps_level.h"
#include "cgps_plan.h"

namespace cgps_host {

// defined once, in cgps_core.hip
extern thread_local char g_err[512];
extern thread_local hipEvent_t g_prof_start, g_prof_stop;
// cgps_leg_obs.hip: zero the arrival counters of that translation unit's fused launches (cgps_reset_counters)
hipError_t leg_obs_reset_counters(hipStream_t st);

inline int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(CGPS_ERR_HIP, "%s: %s", what, hipGetErrorString(e));
  return CGPS_OK;
}

template <typename Fn>
int dispatch(int dtype, int d, Fn&& fn) {
#define CGPS_CASE(DV)                                                        \
  case DV:                                                                   \
    return dtype == CGPS_F32 ? fn(float{}, std::integral_constant<int, DV>{}) \
                             : fn(double{}, std::integral_constant<int, DV>{});
  if (dtype != CGPS_F32 && dtype != CGPS_F64) return fail(CGPS_ERR_UNSUPPORTED, "dtype %d not supported", dtype);
  switch (d) {
    CGPS_CASE(1) CGPS_CASE(2) CGPS_CASE(3) CGPS_CASE(4) CGPS_CASE(5) CGPS_CASE(6) CGPS_CASE(7) CGPS_CASE(8)
    default:
      return fail(CGPS_ERR_UNSUPPORTED, "block size d=%d outside 1..8", d);
  }
#undef CGPS_CASE
}

// The channel axis of the per-row LEG kernels: fn(std::integral_constant<int, O>) with O = obs for 1..4 and O = 8 for
// everything else (5..8: the kernel masks the channels from obs up at run time).
template <typename Fn>
void dispatch_obs(int obs, Fn&& fn) {
  switch (obs) {
    case 1: fn(std::integral_constant<int, 1>{}); break;
    case 2: fn(std::integral_constant<int, 2>{}); break;
    case 3: fn(std::integral_constant<int, 3>{}); break;
    case 4: fn(std::integral_constant<int, 4>{}); break;
    default: fn(std::integral_constant<int, 8>{}); break;
  }
}

// ---- per-device one-time setup -------------------------------------------------------------------
// Function attributes (dynamic-LDS limits) and occupancy-derived grid sizes belong to a device,
// not to the process: a process that drives several GPUs, or two host threads racing the first
// call, must each get them right.  One slot per (kernel family, device), filled under call_once.
constexpr int MAX_DEVICES = 64;
inline int current_device() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return (dev >= 0 && dev < MAX_DEVICES) ? dev : 0;
}
template <typename V>
struct PerDevice {
  std::once_flag once[MAX_DEVICES];
  V value[MAX_DEVICES];
  template <typename Fn>
  const V& get(Fn&& make) {            // make(int device) -> V, run once per device
    const int dev = current_device();
    std::call_once(once[dev], [&] { value[dev] = make(dev); });
    return value[dev];
  }
};
inline int device_cus(int dev) {
  int cus = 256;
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  return cus > 0 ? cus : 256;
}

// ---- workspace regions -> pointers (the layout itself: cgps_plan.h) ----------------------------------------------
template <typename T>
struct LevelBuf {
  T *R, *O, *y;
};
// ping-pong buffer i of a level-wise workspace: R [cap][d][d], O [cap][d][d], then y
template <typename T>
LevelBuf<T> carve(char* ws, const LevelWs& w, int i, int d, bool with_mats, bool with_vec) {
  LevelBuf<T> b{nullptr, nullptr, nullptr};
  T* p = at<T>(ws, w.buf[i]);
  if (with_mats) { b.R = p; p += w.cap[i] * d * d; b.O = p; p += w.cap[i] * d * d; }
  if (with_vec) b.y = p;
  return b;
}

inline bool bad_common(int64_t N, int d) { return N < 1 || d < 1; }

// ---- alignment of the caller's pointers (include/cgps.h, Conventions; the table of who reads what: DESIGN 3.2) ------
// Arrays of blocks and of vectors are read and written 16 bytes at a time (Vec16 in cgps_math.h), workspaces are cut
// into 256-byte regions, everything else is accessed by element.  A null pointer is not this check's business.
constexpr size_t ALIGN_VEC = 16, ALIGN_WS = 256;
inline size_t elem_bytes(int dtype) { return dtype == CGPS_F32 ? 4 : 8; }
struct PtrArg {
  const char* name;
  const void* p;
  size_t align;
};
inline bool misaligned(const void* p, size_t align) { return p && (reinterpret_cast<uintptr_t>(p) % align) != 0; }
// CGPS_OK, or CGPS_ERR_ARG with a message that names the first argument off its boundary; before anything is launched
inline int check_alignment(const char* entry, std::initializer_list<PtrArg> args) {
  for (const PtrArg& a : args)
    if (misaligned(a.p, a.align))
      return fail(CGPS_ERR_ARG, "%s: %s = %p is not aligned to %zu bytes", entry, a.name, a.p, a.align);
  return CGPS_OK;
}
// cgps_halfsolve without the alignment check, for cgps_decompose_solve: the sub-system of the levels its first pass
// leaves starts at a level offset inside the packed factor (cgps_solve.hip)
int halfsolve_unchecked(const void* Dp, const void* Fp, const void* Gp, int64_t N, int d, int dtype, int nrhs, const void* y,
                        void* xcrr, void* ws, size_t ws_bytes, double* mahal_out, void* stream);

inline bool levelwise_solve_requested() {
  static const int v = [] {
    const char* e = getenv("CGPS_LEVELWISE_SOLVE");
    return (e && e[0] == '1') ? 1 : 0;
  }();
  return v == 1;
}

// ---- one launch per reduction level (the simple, always-correct form) -----------------------------
template <typename T, int D>
int run_levelwise(const T* Rs, const T* Os, const T* x, int64_t N, T* Dp, T* Fp, T* Gp, T* xcrr,
                  char* ws, size_t ws_bytes, double* out2, int* info, hipStream_t st) {
  const bool rhs = (x != nullptr), emit = (Dp != nullptr);
  LevelWs w = level_ws(N, D, sizeof(T), true, rhs);
  if (ws_bytes < w.total) return fail(CGPS_ERR_ARG, "workspace too small: %zu < %zu", ws_bytes, w.total);
  Layout L;
  make_layout(N, L);
  double* partial = at<double>(ws, w.partial);
  LevelBuf<T> bufs[2] = {carve<T>(ws, w, 0, D, true, rhs), carve<T>(ws, w, 1, D, true, rhs)};
  (void)hipMemsetAsync(info, 0, sizeof(int), st);
  const T *R = Rs, *O = Os, *y = x;
  int64_t pb = 0;
  for (int l = 0; l < L.nlevels; ++l) {
    const int64_t n = L.ms[l];
    const int64_t nb = level_blocks(n);
    LevelBuf<T>& nx = bufs[l & 1];
    T* Dk = emit ? Dp + L.offD[l] * D * D : nullptr;
    T* Fk = emit ? Fp + L.offF[l] * D * D : nullptr;
    T* Gk = emit ? Gp + L.offG[l] * D * D : nullptr;
    T* xk = (emit && rhs && xcrr) ? xcrr + L.offD[l] * D : nullptr;
    dim3 grid((unsigned)nb), block(cgps::LEVEL_THREADS);
    if (l == 0 && g_prof_start) (void)hipEventRecord(g_prof_start, st);
    if (emit && rhs)
      hipLaunchKernelGGL((cgps::level_kernel<T, D, true, true>), grid, block, 0, st, R, O, y, n, l, Dk, Fk, Gk, xk,
                         nx.R, nx.O, nx.y, partial + 2 * pb, info);
    else if (emit)
      hipLaunchKernelGGL((cgps::level_kernel<T, D, true, false>), grid, block, 0, st, R, O, y, n, l, Dk, Fk, Gk, xk,
                         nx.R, nx.O, nx.y, partial + 2 * pb, info);
    else if (rhs)
      hipLaunchKernelGGL((cgps::level_kernel<T, D, false, true>), grid, block, 0, st, R, O, y, n, l, Dk, Fk, Gk, xk,
                         nx.R, nx.O, nx.y, partial + 2 * pb, info);
    else
      hipLaunchKernelGGL((cgps::level_kernel<T, D, false, false>), grid, block, 0, st, R, O, y, n, l, Dk, Fk, Gk, xk,
                         nx.R, nx.O, nx.y, partial + 2 * pb, info);
    if (l == 0 && g_prof_stop) {
      (void)hipEventRecord(g_prof_stop, st);
      g_prof_start = g_prof_stop = nullptr;
    }
    pb += nb;
    R = nx.R; O = nx.O; y = nx.y;
  }
  if (out2) hipLaunchKernelGGL(cgps::sum_partials_kernel, dim3(1), dim3(256), 0, st, partial, pb, out2);
  return check_launch("levelwise reduction");
}

}  // namespace cgps_host
