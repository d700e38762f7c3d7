// cgps_decompose.hip -- factor-emitting decompose
// One translation unit of libcgps (include/cgps.h); host code only decides sizes/offsets and
// enqueues kernels on the caller's stream: nothing here allocates, copies to the host or synchronises.
#include "cgps_host.h"
#include "cgps_tile.h"
#include "cgps_decomp_tile.h"
#include "cgps_decomp_lds.h"

using namespace cgps_host;

namespace {
// ---- fused (tiled) factorisation: cgps_decomp_tile.h (bulk passes) + cgps_decomp_lds.h (tail) ----
// Bulk passes (cgps_decomp_tile.h) + in-LDS tail (cgps_decomp_lds.h) for the block sizes whose 256-row tile fits the LDS.
// Larger blocks (fp64 d = 6, 7, 8): in-LDS passes only (2^20 rows: 2^20 -> 2^14 -> 2^8 -> 4 -> done; level by level:
// 21 launches, every level's rows written and read back).  Measured (prof_case --op decompose, 2^20 rows, level by
// level -> this): d = 6 1 084 -> 836 us.  For d = 7, 8 the tile passes are bound by their two workgroups per CU (65 KB of
// LDS per 8 x 8 tile): 1 588 -> 1 931 us and 1 836 -> 2 278 us at 2^20 rows, but 263 -> 170 / 330 -> 164 us at 2^14 and
// 334 -> 269 / 403 -> 276 us at 2^16 (a tie at 2^18) -- so those sizes run their levels of more than 2^17 rows one
// launch per level (level_kernel, full occupancy) and hand over to the tile passes below that.
// Which passes, and where each puts its records: plan_decompose in cgps_plan.h.
template <typename T, int D>
int run_decompose_passes(const T* Rs, const T* Os, int64_t N, T* Dp, T* Fp, T* Gp, char* ws, size_t ws_bytes, int* info,
                         hipStream_t st, const T* y = nullptr, T* xcrr = nullptr, T* ynext = nullptr, T* owedy = nullptr,
                         int* rhs_levels = nullptr) {
  // y != nullptr (cgps_decompose_solve): the first pass, when it is a bulk pass of DEC_LP levels, also carries the
  // forward substitution of y through its levels (decomp_tile_kernel<.., RHS = true>); *rhs_levels = levels done
  constexpr bool BULK = cgps::tile_fits_256<T, D>();
  constexpr int LP = cgps::decomp_lds_lp<T, D>();
  DecPlan P;
  plan_decompose(N, D, sizeof(T), y != nullptr, P);
  if (ws_bytes < P.ws.total) return fail(CGPS_ERR_ARG, "workspace too small: %zu < %zu", ws_bytes, P.ws.total);
  Layout L;
  make_layout(N, L);
  // bulk passes, persistent waves: as many workgroups (one wave each) as the chip holds at once
  const size_t lds = (size_t)64 * D * D * sizeof(T);      // staging of the coalesced factor stores
  const size_t lds_small = cgps::decomp_lds_tile_bytes<T, D, LP>();
  struct Caps { int64_t c[2]; };
  static PerDevice<Caps> caps;                          // per device, filled once (thread-safe)
  const Caps& grid_caps = caps.get([&](int dev) {
    int nb0 = 4, nb1 = 4;
    if constexpr (BULK) {
      (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb0, cgps::decomp_tile_kernel<T, D, false>, cgps::DEC_NT, lds);
      (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb1, cgps::decomp_tile_kernel<T, D, true>, cgps::DEC_NT, lds);
    }
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cgps::decomp_lds_kernel<T, D, false, LP>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_small);
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&cgps::decomp_lds_kernel<T, D, true, LP>),
                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_small);
    const int cus = device_cus(dev);
    return Caps{{(int64_t)cus * (nb0 > 0 ? nb0 : 1), (int64_t)cus * (nb1 > 0 ? nb1 : 1)}};
  });
  (void)hipMemsetAsync(info, 0, sizeof(int), st);
  // the two level buffers are also the record buffers of the tile passes
  T* recs[2] = {at<T>(ws, P.ws.buf[0]), at<T>(ws, P.ws.buf[1])};
  LevelBuf<T> bufs[2] = {carve<T>(ws, P.ws, 0, D, true, false), carve<T>(ws, P.ws, 1, D, true, false)};
  double* partial = at<double>(ws, P.ws.partial);
  const T *Rl = Rs, *Ol = Os;     // rows for the first tile pass: the caller's, or those of the last one-level launch
  int64_t pb = 0;
  for (int p = 0; p < P.np; ++p) {
    const DecPass& q = P.pass[p];
    const bool from_rows = q.records_in == 0;             // else from the records of the pass before
    const T* rin = from_rows ? nullptr : recs[q.in];
    T* rout = q.out >= 0 ? recs[q.out] : nullptr;
    if (q.kind == DecKind::Level) {
      const int l = q.first;
      LevelBuf<T>& nx = bufs[q.out];
      hipLaunchKernelGGL((cgps::level_kernel<T, D, true, false>), dim3((unsigned)q.tiles), dim3(cgps::LEVEL_THREADS), 0, st, Rl, Ol,
                         (const T*)nullptr, q.rows, l, Dp + L.offD[l] * D * D, Fp + L.offF[l] * D * D, Gp + L.offG[l] * D * D,
                         (T*)nullptr, nx.R, nx.O, nx.y, partial + 2 * pb, info);
      pb += q.tiles;
      Rl = nx.R;
      Ol = nx.O;
    } else if (q.kind == DecKind::Lds) {
      cgps::DecompLevelsL dl;
      dl.nlev = q.nlev;
      fill_window(L, q.first, dl);
      if (from_rows)
        hipLaunchKernelGGL((cgps::decomp_lds_kernel<T, D, false, LP>), dim3((unsigned)q.tiles), dim3(cgps::DECL_NT), lds_small, st,
                           Rl, Ol, q.rows, (int64_t)0, 1, dl, q.first, Dp, Fp, Gp, rout, info);
      else
        hipLaunchKernelGGL((cgps::decomp_lds_kernel<T, D, true, LP>), dim3((unsigned)q.tiles), dim3(cgps::DECL_NT), lds_small, st,
                           rin, (const T*)nullptr, q.rows, q.records_in, q.spt_in, dl, q.first, Dp, Fp, Gp, rout, info);
    } else if constexpr (BULK) {
      cgps::DecompLevels dl;
      dl.nlev = q.nlev;
      fill_window(L, q.first, dl);
      const int64_t cap = grid_caps.c[from_rows ? 0 : 1];
      const unsigned grid = (unsigned)(q.tiles < cap ? q.tiles : cap);
      if (q.kind == DecKind::BulkRhs) {
        hipLaunchKernelGGL((cgps::decomp_tile_kernel<T, D, false, true>), dim3(grid), dim3(cgps::DEC_NT),
                           lds + (size_t)(D * D + D) * sizeof(T), st, Rs, Os,
                           q.rows, (int64_t)0, 1, dl, q.first, Dp, Fp, Gp, rout, info, y, xcrr, ynext, owedy);
        const int64_t pairs = (q.tiles - 1) * D;
        if (pairs > 0)
          hipLaunchKernelGGL((cgps::decomp_rhs_fixup_kernel<T, D>), dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, ynext,
                             (const T*)owedy, q.tiles, (int)(cgps::DEC_TS >> q.nlev), L.ms[q.nlev]);
        if (rhs_levels) *rhs_levels = q.nlev;
      } else if (from_rows)
        hipLaunchKernelGGL((cgps::decomp_tile_kernel<T, D, false>), dim3(grid), dim3(cgps::DEC_NT), lds, st, Rs, Os,
                           q.rows, (int64_t)0, 1, dl, q.first, Dp, Fp, Gp, rout, info);
      else
        hipLaunchKernelGGL((cgps::decomp_tile_kernel<T, D, true>), dim3(grid), dim3(cgps::DEC_NT), lds, st, rin,
                           (const T*)nullptr, q.rows, q.records_in, q.spt_in, dl, q.first, Dp, Fp, Gp, rout, info);
    }
  }
  return check_launch("decompose (tiled)");
}
}  // namespace

extern "C" {

int cgps_decompose_solve(const void* Rs, const void* Os, const void* y, int64_t N, int d, int dtype, void* Dp, void* Fp,
                         void* Gp, void* xcrr, void* x, void* ws, size_t ws_bytes, int* info, void* stream) {
  if (bad_common(N, d) || !Rs || (N > 1 && !Os) || !y || !Dp || !Fp || !Gp || !xcrr || !x || !ws || !info)
    return fail(CGPS_ERR_ARG, "cgps_decompose_solve: null pointer or N < 1");
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_decompose_solve", {{"Rs", Rs, ALIGN_VEC}, {"Os", Os, ALIGN_VEC}, {"y", y, ALIGN_VEC},
                                                          {"Dp", Dp, ALIGN_VEC}, {"Fp", Fp, ALIGN_VEC}, {"Gp", Gp, ALIGN_VEC},
                                                          {"xcrr", xcrr, ALIGN_VEC}, {"x", x, ALIGN_VEC}, {"ws", ws, ALIGN_WS},
                                                          {"info", info, 4}}))
      return rc;
    const DecomposeSolveWs w = decompose_solve_ws(N, D, sizeof(T));
    if (ws_bytes < w.total) return fail(CGPS_ERR_ARG, "workspace too small: %zu < %zu", ws_bytes, w.total);
    const size_t main_bytes = w.main.bytes;      // what decompose and the sweeps use, one after the other
    T* ynext = at<T>((char*)ws, w.ynext);
    T* owedy = at<T>((char*)ws, w.owedy);
    int rhs_levels = 0, rc;
    if (!levelwise_solve_requested())
      rc = run_decompose_passes<T, D>((const T*)Rs, (const T*)Os, N, (T*)Dp, (T*)Fp, (T*)Gp, (char*)ws, main_bytes, info,
                                      (hipStream_t)stream, (const T*)y, (T*)xcrr, ynext, owedy, &rhs_levels);
    else
      rc = cgps_decompose(Rs, Os, N, d, dtype, Dp, Fp, Gp, ws, main_bytes, info, stream);
    if (rc != CGPS_OK) return rc;
    if (rhs_levels > 0) {
      // the forward sweep goes on at level rhs_levels: the packed factor of levels >= l IS the packed factor of the
      // (N >> l)-row system those levels reduce (level sizes halve with the same rounding), so the stored-factor
      // sweep runs on that sub-system with the surviving rows' right-hand side
      Layout L;
      make_layout(N, L);
      const int l = rhs_levels;
      rc = halfsolve_unchecked((const T*)Dp + L.offD[l] * D * D, (const T*)Fp + L.offF[l] * D * D, (const T*)Gp + L.offG[l] * D * D,
                          L.ms[l], d, dtype, 1, ynext, (T*)xcrr + L.offD[l] * D, ws, main_bytes, nullptr, stream);
    } else {
      rc = cgps_halfsolve(Dp, Fp, Gp, N, d, dtype, 1, y, xcrr, ws, main_bytes, nullptr, stream);
    }
    if (rc != CGPS_OK) return rc;
    return cgps_backsolve(Dp, Fp, Gp, N, d, dtype, 1, xcrr, x, ws, main_bytes, stream);
  });
}

int cgps_decompose(const void* Rs, const void* Os, int64_t N, int d, int dtype, void* Dp, void* Fp, void* Gp, void* ws,
                   size_t ws_bytes, int* info, void* stream) {
  if (bad_common(N, d) || !Rs || (N > 1 && !Os) || !Dp || !Fp || !Gp || !ws || !info)
    return fail(CGPS_ERR_ARG, "cgps_decompose: null pointer or N < 1");
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    if (int rc = check_alignment("cgps_decompose", {{"Rs", Rs, ALIGN_VEC}, {"Os", Os, ALIGN_VEC}, {"Dp", Dp, ALIGN_VEC},
                                                    {"Fp", Fp, ALIGN_VEC}, {"Gp", Gp, ALIGN_VEC}, {"ws", ws, ALIGN_WS},
                                                    {"info", info, 4}}))
      return rc;
    if (!levelwise_solve_requested())
      return run_decompose_passes<T, D>((const T*)Rs, (const T*)Os, N, (T*)Dp, (T*)Fp, (T*)Gp, (char*)ws, ws_bytes, info,
                                        (hipStream_t)stream);
    return run_levelwise<T, D>((const T*)Rs, (const T*)Os, nullptr, N, (T*)Dp, (T*)Fp, (T*)Gp, nullptr, (char*)ws,
                               ws_bytes, nullptr, info, (hipStream_t)stream);
  });
}

}  // extern "C"
