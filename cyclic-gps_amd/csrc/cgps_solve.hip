// cgps_solve.hip -- halfsolve / backhalfsolve / solve on a stored factor
// One translation unit of libcgps (include/cgps.h); host code only decides sizes/offsets and
// enqueues kernels on the caller's stream: nothing here allocates, copies to the host or synchronises.
#include "cgps_host.h"
#include "cgps_tile.h"
#include "cgps_solve_tile.h"
#include "cgps_solve_tile_m.h"

using namespace cgps_host;

namespace {
// ---- fused (tiled) substitution sweeps: cgps_solve_tile.h ---------------------------------------
// (the passes of a sweep: SolvePasses / plan_sweep / plan_panel_sweep in cgps_plan.h)
// passes of at most one tile per CU take the "deep" kernels (CGPS_NO_DEEP_SOLVE=1: the level-by-level loads, for A/B timing)
inline int64_t deep_tiles_max() {
  static PerDevice<int64_t> cus;
  return cus.get([](int dev) { return (int64_t)device_cus(dev); });
}
inline bool fused_top_enabled() {           // CGPS_NO_FUSED_TOP=1: separate forward / backward top passes
  static const bool on = [] { const char* e = getenv("CGPS_NO_FUSED_TOP"); return !(e && e[0] == '1'); }();
  return on;
}
inline bool deep_solve_enabled() {
  static const bool on = [] { const char* e = getenv("CGPS_NO_DEEP_SOLVE"); return !(e && e[0] == '1'); }();
  return on;
}

// the pb partial sums of a forward sweep -> mahal_out (the slot behind them was reserved for the sum)
inline void sum_mahal(double* partial, int64_t pb, double* mahal_out, hipStream_t st) {
  if (!mahal_out) return;
  hipLaunchKernelGGL(cgps::sum_partials_kernel, dim3(1), dim3(256), 0, st, partial, pb, partial + 2 * pb);
  (void)hipMemcpyAsync(mahal_out, partial + 2 * pb, sizeof(double), hipMemcpyDeviceToDevice, st);
}

template <typename T, int D>
int64_t deep_tiles_for() {
  if constexpr (cgps::solve_deep_supported<T, D>()) return deep_solve_enabled() ? deep_tiles_max() : 0;
  else return 0;
}

template <typename T, int D>
void solve_tile_attributes() {
  static PerDevice<int> done;
  done.get([](int) {
  const int lds = (int)cgps::solve_lds_bytes<T, D>();
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cgps::halfsolve_tile_kernel<T, D>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cgps::backsolve_tile_kernel<T, D>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if constexpr (cgps::solve_deep_supported<T, D>()) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cgps::halfsolve_deep_kernel<T, D, cgps::SOLVE_LP>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cgps::backsolve_deep_kernel<T, D, cgps::SOLVE_LP>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cgps::halfsolve_deep_kernel<T, D, cgps::SOLVE_LP - 1>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cgps::backsolve_deep_kernel<T, D, cgps::SOLVE_LP - 1>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cgps::solve_top_kernel<T, D, cgps::SOLVE_LP>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cgps::solve_top_kernel<T, D, cgps::SOLVE_LP - 1>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  }
  return 1;
  });
}

template <typename T, int D>
int run_halfsolve_tile(const T* Dp, const T* Fp, const T* Gp, int64_t N, const T* y0, T* xcrr, char* ws,
                       size_t ws_bytes, double* mahal_out, hipStream_t st, T* fused_top_x = nullptr,
                       bool* fused_top = nullptr) {
  // fused_top_x != nullptr (solve(), the caller's x): the backward sweep follows on the same workspace
  const LevelWs w = halfsolve_ws(N, D, sizeof(T));
  const BacksolveWs back = backsolve_ws(N, D, sizeof(T));
  const size_t need = fused_top_x ? max_bytes(w.total, back.total) : w.total;
  if (ws_bytes < need) return fail(CGPS_ERR_ARG, "workspace too small: %zu < %zu", ws_bytes, need);
  Layout L;
  make_layout(N, L);
  SolvePasses P;
  plan_sweep(L, P, deep_tiles_for<T, D>());
  solve_tile_attributes<T, D>();
  double* partial = at<double>(ws, w.partial);
  T* bufs[2] = {at<T>(ws, w.buf[0]), at<T>(ws, w.buf[1])};
  const size_t lds = cgps::solve_lds_bytes<T, D>();
  const T* y = y0;
  const T* owed_in = nullptr;
  int64_t n_owed = 0, pb = 0;
  int spt_in = 1;
  for (int p = 0; p < P.np; ++p) {
    const int64_t n = P.rows[p], g = P.tiles[p];
    const bool more = (p + 1 < P.np);
    T* yout = more ? bufs[P.buf(p)] : nullptr;         // [nsurv][D] surviving rows, then [g][D] owed vectors
    T* owed_out = more ? yout + (P.nsurv[p] + 1) * D : nullptr;
    bool launched = false;
    if constexpr (cgps::solve_deep_supported<T, D>()) {
      // solve(): the single-tile top pass runs its forward and its backward sweep in ONE launch
      // (solve_top_kernel) and leaves the solution of its rows where the backward sweep reads it
      if (fused_top_x != nullptr && !more && g == 1 && P.deep[p] && fused_top_enabled()) {
        T* xtop = (p == 0) ? fused_top_x : at<T>(ws, back.x_of(p));
        if (P.ts[p] == cgps::SOLVE_TS)
          hipLaunchKernelGGL((cgps::solve_top_kernel<T, D, cgps::SOLVE_LP>), dim3(1), dim3(cgps::SOLVE_NT), lds, st, Dp, Fp, Gp,
                             P.lv[p], owed_in, n_owed, spt_in, y, n, xcrr, xtop, partial + 2 * pb);
        else
          hipLaunchKernelGGL((cgps::solve_top_kernel<T, D, cgps::SOLVE_LP - 1>), dim3(1), dim3(cgps::SOLVE_NT / 2), lds, st, Dp,
                             Fp, Gp, P.lv[p], owed_in, n_owed, spt_in, y, n, xcrr, xtop, partial + 2 * pb);
        launched = true;
        *fused_top = true;
      }
    }
    if constexpr (cgps::solve_deep_supported<T, D>()) {
      // few tiles (at most one per CU): the latency-bound form with every factor block requested up front
      if (launched) {
      } else if (P.deep[p] && P.ts[p] == cgps::SOLVE_TS) {
        hipLaunchKernelGGL((cgps::halfsolve_deep_kernel<T, D, cgps::SOLVE_LP>), dim3((unsigned)g), dim3(cgps::SOLVE_NT), lds, st,
                           Dp, Fp, Gp, P.lv[p], owed_in, n_owed, spt_in, y, n, xcrr, yout, owed_out, partial + 2 * pb);
        launched = true;
      } else if (P.deep[p]) {
        hipLaunchKernelGGL((cgps::halfsolve_deep_kernel<T, D, cgps::SOLVE_LP - 1>), dim3((unsigned)g),
                           dim3(cgps::SOLVE_NT / 2), lds, st, Dp, Fp, Gp, P.lv[p], owed_in, n_owed, spt_in, y, n, xcrr, yout,
                           owed_out, partial + 2 * pb);
        launched = true;
      }
    }
    if (!launched)
      hipLaunchKernelGGL((cgps::halfsolve_tile_kernel<T, D>), dim3((unsigned)g), dim3(cgps::SOLVE_NT), lds, st, Dp, Fp, Gp,
                         P.lv[p], owed_in, n_owed, spt_in, y, n, xcrr, yout, owed_out, partial + 2 * pb);
    pb += g;
    y = yout;
    owed_in = owed_out;
    n_owed = g;
    spt_in = P.ts[p] >> P.lv[p].nlev;
    if (spt_in < 1) spt_in = 1;
  }
  sum_mahal(partial, pb, mahal_out, st);
  return check_launch("halfsolve (tiled)");
}

template <typename T, int D>
int run_backsolve_tile(const T* Dp, const T* Fp, const T* Gp, int64_t N, const T* ycrr, T* x, char* ws,
                       size_t ws_bytes, hipStream_t st, bool top_done = false) {
  const BacksolveWs w = backsolve_ws(N, D, sizeof(T));
  if (ws_bytes < w.total) return fail(CGPS_ERR_ARG, "workspace too small: %zu < %zu", ws_bytes, w.total);
  Layout L;
  make_layout(N, L);
  SolvePasses P;
  plan_sweep(L, P, deep_tiles_for<T, D>());   // (same passes as the forward sweep)
  solve_tile_attributes<T, D>();
  const size_t lds = cgps::solve_lds_bytes<T, D>();
  const T* xc = nullptr;
  for (int p = P.np - 1; p >= 0; --p) {
    const int64_t n = P.rows[p], g = P.tiles[p];
    T* X = (p == 0) ? x : at<T>(ws, w.x_of(p));
    if (top_done && p == P.np - 1) {                     // solve_top_kernel has left this pass's solution in X
      xc = X;
      continue;
    }
    bool launched = false;
    if constexpr (cgps::solve_deep_supported<T, D>()) {
      if (P.deep[p] && P.ts[p] == cgps::SOLVE_TS) {
        hipLaunchKernelGGL((cgps::backsolve_deep_kernel<T, D, cgps::SOLVE_LP>), dim3((unsigned)g), dim3(cgps::SOLVE_NT), lds, st,
                           Dp, Fp, Gp, P.lv[p], ycrr, xc, n, X);
        launched = true;
      } else if (P.deep[p]) {
        hipLaunchKernelGGL((cgps::backsolve_deep_kernel<T, D, cgps::SOLVE_LP - 1>), dim3((unsigned)g),
                           dim3(cgps::SOLVE_NT / 2), lds, st, Dp, Fp, Gp, P.lv[p], ycrr, xc, n, X);
        launched = true;
      }
    }
    if (!launched)
      hipLaunchKernelGGL((cgps::backsolve_tile_kernel<T, D>), dim3((unsigned)g), dim3(cgps::SOLVE_NT), lds, st, Dp, Fp, Gp,
                         P.lv[p], ycrr, xc, n, X);
    xc = X;
  }
  return check_launch("backsolve (tiled)");
}

template <typename T, int D>
int run_halfsolve_levelwise(const T* Dp, const T* Fp, const T* Gp, int64_t N, const T* y0, T* xcrr, char* ws,
                            size_t ws_bytes, double* mahal_out, hipStream_t st) {
  const LevelWs w = halfsolve_ws(N, D, sizeof(T));
  if (ws_bytes < w.total) return fail(CGPS_ERR_ARG, "workspace too small: %zu < %zu", ws_bytes, w.total);
  Layout L;
  make_layout(N, L);
  double* partial = at<double>(ws, w.partial);
  T* bufs[2] = {at<T>(ws, w.buf[0]), at<T>(ws, w.buf[1])};
  const T* y = y0;
  int64_t pb = 0;
  for (int l = 0; l < L.nlevels; ++l) {
    const int64_t n = L.ms[l], nb = level_blocks(n);
    T* yn = bufs[l & 1];
    hipLaunchKernelGGL((cgps::halfsolve_level_kernel<T, D>), dim3((unsigned)nb), dim3(cgps::LEVEL_THREADS), 0, st,
                       Dp + L.offD[l] * D * D, Fp + L.offF[l] * D * D, Gp + L.offG[l] * D * D, y, n,
                       xcrr + L.offD[l] * D, yn, partial + 2 * pb);
    pb += nb;
    y = yn;
  }
  sum_mahal(partial, pb, mahal_out, st);
  return check_launch("halfsolve");
}

template <typename T, int D>
int run_backsolve_levelwise(const T* Dp, const T* Fp, const T* Gp, int64_t N, const T* ycrr, T* x, char* ws,
                            size_t ws_bytes, hipStream_t st) {
  const BacksolveWs w = backsolve_ws(N, D, sizeof(T));
  if (ws_bytes < w.total) return fail(CGPS_ERR_ARG, "workspace too small: %zu < %zu", ws_bytes, w.total);
  Layout L;
  make_layout(N, L);
  const T* xo = nullptr;
  for (int l = L.nlevels - 1; l >= 0; --l) {
    const int64_t n = L.ms[l], nb = level_blocks(n);
    T* X = (l == 0) ? x : at<T>(ws, w.x_of(l));
    hipLaunchKernelGGL((cgps::backsolve_level_kernel<T, D>), dim3((unsigned)nb), dim3(cgps::LEVEL_THREADS), 0, st,
                       Dp + L.offD[l] * D * D, Fp + L.offF[l] * D * D, Gp + L.offG[l] * D * D,
                       ycrr + L.offD[l] * D, xo, n, X);
    xo = X;
  }
  return check_launch("backsolve");
}

template <typename T, int D>
int run_halfsolve(const T* Dp, const T* Fp, const T* Gp, int64_t N, const T* y0, T* xcrr, char* ws, size_t ws_bytes,
                  double* mahal_out, hipStream_t st, T* fused_top_x = nullptr, bool* fused_top = nullptr) {
  if (levelwise_solve_requested()) return run_halfsolve_levelwise<T, D>(Dp, Fp, Gp, N, y0, xcrr, ws, ws_bytes, mahal_out, st);
  return run_halfsolve_tile<T, D>(Dp, Fp, Gp, N, y0, xcrr, ws, ws_bytes, mahal_out, st, fused_top_x, fused_top);
}
template <typename T, int D>
int run_backsolve(const T* Dp, const T* Fp, const T* Gp, int64_t N, const T* ycrr, T* x, char* ws, size_t ws_bytes,
                  hipStream_t st, bool top_done = false) {
  if (levelwise_solve_requested()) return run_backsolve_levelwise<T, D>(Dp, Fp, Gp, N, ycrr, x, ws, ws_bytes, st);
  return run_backsolve_tile<T, D>(Dp, Fp, Gp, N, ycrr, x, ws, ws_bytes, st, top_done);
}

// ---- several right-hand sides per sweep: cgps_solve_tile_m.h ----------------------------------------
template <typename T, int D, int MC>
void solve_m_attributes() {
  static PerDevice<int> done;
  done.get([](int) {
    const int lds = (int)cgps::solve_m_lds_bytes<T, D, MC>();
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cgps::halfsolve_tile_m_kernel<T, D, MC>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cgps::backsolve_tile_m_kernel<T, D, MC>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    if constexpr (cgps::solve_deep_supported<T, D>()) {
      const int ldsd = (int)cgps::solve_m_deep_lds_bytes<T, D, MC>();
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cgps::halfsolve_deep_m_kernel<T, D, MC>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, ldsd);
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cgps::backsolve_deep_m_kernel<T, D, MC>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, ldsd);
    }
    return 1;
  });
}

// forward sweep of w <= MC columns: y [N][D][ld_y] -> xcrr [N][D][ld_x]; partial sums appended at *pb
template <typename T, int D, int MC>
int run_halfsolve_panel(const SolvePasses& P, const T* Dp, const T* Fp, const T* Gp, const T* y0, int ld_y, int w, T* xcrr, int ld_x,
                        double* partial, int64_t* pb, T* buf0, T* buf1, hipStream_t st) {
  constexpr int TSL = cgps::solve_m_tile_log2<MC>(), TS = 1 << TSL, NT = TS / 2, PW = D * MC;
  constexpr int TSLD = cgps::solve_m_deep_tile_log2<MC>(), TSD = 1 << TSLD, CS = cgps::solve_m_col_splits<MC>();
  constexpr bool DEEP = cgps::solve_deep_supported<T, D>();
  solve_m_attributes<T, D, MC>();
  T* bufs[2] = {buf0, buf1};
  const size_t lds = cgps::solve_m_lds_bytes<T, D, MC>();
  const T* y = y0;
  int ld = ld_y;
  const T* owed_in = nullptr;
  int64_t n_owed = 0;
  int spt_in = 1;
  for (int p = 0; p < P.np; ++p) {
    const int ts = P.ts[p];
    const int64_t n = P.rows[p], g = P.tiles[p];
    const bool more = (p + 1 < P.np);
    T* yout = more ? bufs[P.buf(p)] : nullptr;         // [nsurv][D][MC] surviving rows, then [g][D][MC] owed panels
    T* owed_out = more ? yout + (P.nsurv[p] + 1) * PW : nullptr;
    bool launched = false;
    if constexpr (DEEP) {
      if (P.deep[p]) {
        const size_t ldsd = cgps::solve_m_deep_lds_bytes<T, D, MC>();
        hipLaunchKernelGGL((cgps::halfsolve_deep_m_kernel<T, D, MC>), dim3((unsigned)g), dim3(TSD / 2 * CS), ldsd, st, Dp, Fp, Gp,
                           P.lv[p], owed_in, n_owed, spt_in, y, ld, n, w, xcrr, ld_x, yout, owed_out, partial + 2 * *pb);
        launched = true;
      }
    }
    if (!launched)
      hipLaunchKernelGGL((cgps::halfsolve_tile_m_kernel<T, D, MC>), dim3((unsigned)g), dim3(NT * CS), lds, st, Dp, Fp, Gp, P.lv[p],
                         owed_in, n_owed, spt_in, y, ld, n, w, xcrr, ld_x, yout, owed_out, partial + 2 * *pb);
    *pb += g;
    y = yout;
    ld = MC;
    owed_in = owed_out;
    n_owed = g;
    spt_in = ts >> P.lv[p].nlev;
    if (spt_in < 1) spt_in = 1;
  }
  return CGPS_OK;
}

template <typename T, int D, int MC>
int run_backsolve_panel(const SolvePasses& P, const T* Dp, const T* Fp, const T* Gp, const T* b, int ld_b, int w, T* x, int ld_o,
                        T* buf0, T* buf1, hipStream_t st) {
  constexpr int TSL = cgps::solve_m_tile_log2<MC>(), TS = 1 << TSL, NT = TS / 2;
  constexpr int TSLD = cgps::solve_m_deep_tile_log2<MC>(), TSD = 1 << TSLD, CS = cgps::solve_m_col_splits<MC>();
  constexpr bool DEEP = cgps::solve_deep_supported<T, D>();
  solve_m_attributes<T, D, MC>();
  T* bufs[2] = {buf0, buf1};
  const size_t lds = cgps::solve_m_lds_bytes<T, D, MC>();
  const T* xc = nullptr;
  for (int p = P.np - 1; p >= 0; --p) {
    const int64_t n = P.rows[p], g = P.tiles[p];
    T* X = (p == 0) ? x : bufs[P.buf(p)];
    bool launched = false;
    if constexpr (DEEP) {
      if (P.deep[p]) {
        const size_t ldsd = cgps::solve_m_deep_lds_bytes<T, D, MC>();
        hipLaunchKernelGGL((cgps::backsolve_deep_m_kernel<T, D, MC>), dim3((unsigned)g), dim3(TSD / 2 * CS), ldsd, st, Dp, Fp, Gp,
                           P.lv[p], b, ld_b, xc, n, w, X, (p == 0) ? ld_o : MC);
        launched = true;
      }
    }
    if (!launched)
      hipLaunchKernelGGL((cgps::backsolve_tile_m_kernel<T, D, MC>), dim3((unsigned)g), dim3(NT * CS), lds, st, Dp, Fp, Gp, P.lv[p],
                         b, ld_b, xc, n, w, X, (p == 0) ? ld_o : MC);
    xc = X;
  }
  return CGPS_OK;
}

enum class PanelOp { Half, Back, Solve };
// nrhs >= 2 columns, panels of up to eight: halfsolve (y -> xcrr, mahal), backsolve (y = CRR -> x), solve (y -> x)
template <typename T, int D, int MC>
int run_panels(PanelOp op, const T* Dp, const T* Fp, const T* Gp, int64_t N, int nrhs, const T* y, T* out, char* ws,
               size_t ws_bytes, double* mahal_out, hipStream_t st) {
  const PanelWs w = panel_ws(N, D, sizeof(T), nrhs, op == PanelOp::Solve);
  if (ws_bytes < w.total) return fail(CGPS_ERR_ARG, "workspace too small: %zu < %zu", ws_bytes, w.total);
  double* partial = at<double>(ws, w.partial);
  T* buf0 = at<T>(ws, w.buf[0]);
  T* buf1 = at<T>(ws, w.buf[1]);
  T* xcrr_ws = at<T>(ws, w.crr);
  Layout L;
  make_layout(N, L);
  SolvePasses P;                    // the passes of every chunk's forward and backward sweep
  plan_panel_sweep(L, P, MC, cgps::solve_deep_supported<T, D>(), deep_solve_enabled());
  int64_t pb = 0;
  for (int c0 = 0; c0 < nrhs; c0 += MC) {
    const int wd = nrhs - c0 < MC ? nrhs - c0 : MC;
    if (op == PanelOp::Half)
      run_halfsolve_panel<T, D, MC>(P, Dp, Fp, Gp, y + c0, nrhs, wd, out + c0, nrhs, partial, &pb, buf0, buf1, st);
    else if (op == PanelOp::Back)
      run_backsolve_panel<T, D, MC>(P, Dp, Fp, Gp, y + c0, nrhs, wd, out + c0, nrhs, buf0, buf1, st);
    else {
      run_halfsolve_panel<T, D, MC>(P, Dp, Fp, Gp, y + c0, nrhs, wd, xcrr_ws, MC, partial, &pb, buf0, buf1, st);
      run_backsolve_panel<T, D, MC>(P, Dp, Fp, Gp, xcrr_ws, MC, wd, out + c0, nrhs, buf0, buf1, st);
    }
  }
  sum_mahal(partial, pb, mahal_out, st);
  return check_launch("panel substitution sweeps");
}

template <typename T, int D>
int run_panels_any(PanelOp op, const T* Dp, const T* Fp, const T* Gp, int64_t N, int nrhs, const T* y, T* out, char* ws,
                   size_t ws_bytes, double* mahal_out, hipStream_t st) {
  switch (cgps::panel_width(nrhs)) {
    case 2: return run_panels<T, D, 2>(op, Dp, Fp, Gp, N, nrhs, y, out, ws, ws_bytes, mahal_out, st);
    case 4: return run_panels<T, D, 4>(op, Dp, Fp, Gp, N, nrhs, y, out, ws, ws_bytes, mahal_out, st);
    default: return run_panels<T, D, 8>(op, Dp, Fp, Gp, N, nrhs, y, out, ws, ws_bytes, mahal_out, st);
  }
}

// cgps_halfsolve (aligned = true: the caller's pointers are checked) and the call cgps_decompose_solve makes on the
// sub-system of the levels its first pass leaves, whose factor starts at a level offset (halfsolve_unchecked)
int halfsolve_any(const void* Dp, const void* Fp, const void* Gp, int64_t N, int d, int dtype, int nrhs, const void* y,
                  void* xcrr, void* ws, size_t ws_bytes, double* mahal_out, void* stream, bool aligned) {
  if (bad_common(N, d) || nrhs < 1 || !Dp || !Fp || !Gp || !y || !xcrr || !ws)
    return fail(CGPS_ERR_ARG, "cgps_halfsolve: null pointer, N < 1 or nrhs < 1");
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (aligned)
      if (int rc = check_alignment("cgps_halfsolve", {{"Dp", Dp, ALIGN_VEC}, {"Fp", Fp, ALIGN_VEC}, {"Gp", Gp, ALIGN_VEC},
                                                      {"y", y, ALIGN_VEC}, {"xcrr", xcrr, ALIGN_VEC}, {"ws", ws, ALIGN_WS},
                                                      {"mahal_out", mahal_out, 8}}))
        return rc;
    if (nrhs > 1)
      return run_panels_any<T, D>(PanelOp::Half, (const T*)Dp, (const T*)Fp, (const T*)Gp, N, nrhs, (const T*)y, (T*)xcrr,
                                  (char*)ws, ws_bytes, mahal_out, (hipStream_t)stream);
    return run_halfsolve<T, D>((const T*)Dp, (const T*)Fp, (const T*)Gp, N, (const T*)y, (T*)xcrr, (char*)ws, ws_bytes,
                               mahal_out, (hipStream_t)stream);
  });
}
}  // namespace

extern "C" {

int cgps_solve_workspace_bytes(int64_t N, int d, int dtype, int op, int nrhs, size_t* bytes) {
  if (bad_common(N, d) || !bytes || nrhs < 1) return fail(CGPS_ERR_ARG, "cgps_solve_workspace_bytes: bad argument");
  if (nrhs == 1) return cgps_workspace_bytes(N, d, dtype, op, bytes);
  if (d > 8) return fail(CGPS_ERR_UNSUPPORTED, "block size d=%d outside 1..8", d);
  if (dtype != CGPS_F32 && dtype != CGPS_F64) return fail(CGPS_ERR_UNSUPPORTED, "dtype %d not supported", dtype);
  if (op != CGPS_OP_HALFSOLVE && op != CGPS_OP_BACKSOLVE && op != CGPS_OP_SOLVE)
    return fail(CGPS_ERR_ARG, "cgps_solve_workspace_bytes: op %d takes no right-hand sides", op);
  const size_t s = dtype == CGPS_F32 ? 4 : 8;
  *bytes = panel_ws(N, d, s, nrhs, op == CGPS_OP_SOLVE).total;
  return CGPS_OK;
}

int cgps_halfsolve(const void* Dp, const void* Fp, const void* Gp, int64_t N, int d, int dtype, int nrhs, const void* y,
                   void* xcrr, void* ws, size_t ws_bytes, double* mahal_out, void* stream) {
  return halfsolve_any(Dp, Fp, Gp, N, d, dtype, nrhs, y, xcrr, ws, ws_bytes, mahal_out, stream, true);
}

}  // extern "C"

int cgps_host::halfsolve_unchecked(const void* Dp, const void* Fp, const void* Gp, int64_t N, int d, int dtype, int nrhs,
                                   const void* y, void* xcrr, void* ws, size_t ws_bytes, double* mahal_out, void* stream) {
  return halfsolve_any(Dp, Fp, Gp, N, d, dtype, nrhs, y, xcrr, ws, ws_bytes, mahal_out, stream, false);
}

extern "C" {

int cgps_backsolve(const void* Dp, const void* Fp, const void* Gp, int64_t N, int d, int dtype, int nrhs,
                   const void* ycrr, void* x, void* ws, size_t ws_bytes, void* stream) {
  if (bad_common(N, d) || nrhs < 1 || !Dp || !Fp || !Gp || !ycrr || !x || !ws)
    return fail(CGPS_ERR_ARG, "cgps_backsolve: null pointer, N < 1 or nrhs < 1");
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_backsolve", {{"Dp", Dp, ALIGN_VEC}, {"Fp", Fp, ALIGN_VEC}, {"Gp", Gp, ALIGN_VEC},
                                                    {"ycrr", ycrr, ALIGN_VEC}, {"x", x, ALIGN_VEC}, {"ws", ws, ALIGN_WS}}))
      return rc;
    if (nrhs > 1)
      return run_panels_any<T, D>(PanelOp::Back, (const T*)Dp, (const T*)Fp, (const T*)Gp, N, nrhs, (const T*)ycrr, (T*)x,
                                  (char*)ws, ws_bytes, nullptr, (hipStream_t)stream);
    return run_backsolve<T, D>((const T*)Dp, (const T*)Fp, (const T*)Gp, N, (const T*)ycrr, (T*)x, (char*)ws, ws_bytes,
                               (hipStream_t)stream);
  });
}

int cgps_solve(const void* Dp, const void* Fp, const void* Gp, int64_t N, int d, int dtype, int nrhs, const void* y,
               void* x, void* ws, size_t ws_bytes, void* stream) {
  if (bad_common(N, d) || nrhs < 1 || !Dp || !Fp || !Gp || !y || !x || !ws)
    return fail(CGPS_ERR_ARG, "cgps_solve: null pointer, N < 1 or nrhs < 1");
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_solve", {{"Dp", Dp, ALIGN_VEC}, {"Fp", Fp, ALIGN_VEC}, {"Gp", Gp, ALIGN_VEC},
                                                {"y", y, ALIGN_VEC}, {"x", x, ALIGN_VEC}, {"ws", ws, ALIGN_WS}}))
      return rc;
    if (nrhs > 1)
      return run_panels_any<T, D>(PanelOp::Solve, (const T*)Dp, (const T*)Fp, (const T*)Gp, N, nrhs, (const T*)y, (T*)x,
                                  (char*)ws, ws_bytes, nullptr, (hipStream_t)stream);
    // [CRR vector] [what the two sweeps use one after the other]: the fused top pass of the forward sweep leaves its
    // solution where the backward sweep's plan reads it
    const SolveWs w = solve_ws(N, D, sizeof(T));
    if (ws_bytes < w.total) return fail(CGPS_ERR_ARG, "workspace too small: %zu < %zu", ws_bytes, w.total);
    T* xcrr = at<T>((char*)ws, w.crr);
    char* sweep = at<char>((char*)ws, w.sweep);
    bool top_done = false;
    int rc = run_halfsolve<T, D>((const T*)Dp, (const T*)Fp, (const T*)Gp, N, (const T*)y, xcrr, sweep, w.sweep.bytes,
                                 nullptr, (hipStream_t)stream, (T*)x, &top_done);
    if (rc != CGPS_OK) return rc;
    return run_backsolve<T, D>((const T*)Dp, (const T*)Fp, (const T*)Gp, N, xcrr, (T*)x, sweep, w.sweep.bytes,
                               (hipStream_t)stream, top_done);
  });
}

}  // extern "C"
