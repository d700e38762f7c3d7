// Host-pure planning: everything the host decides before it launches -- the level layout of the packed factor, the
// tile shapes the plans branch on, how each operation's caller-owned workspace is cut into named regions, and the
// list of passes an operation runs (which kernel family, which levels, which region it reads and writes, how many
// bytes it writes there).  cgps_workspace_bytes() / cgps_solve_workspace_bytes() return a plan's `total`; every run_*
// function takes its pointers from the same plan and checks ws_bytes against the same `total`.
// Nothing from HIP is included: this header compiles with a plain C++17 host compiler, so that the layout can be
// checked without a GPU (tests/test_plan.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/cgps.h"

namespace cgps {

// ---- tile shapes (one definition each; the kernel headers include this file for them) ---------------------------
constexpr int LEVEL_THREADS = 128;      // one launch per level: eliminations per workgroup

constexpr int SOLVE_LP = 10;            // substitution sweeps: levels per pass
constexpr int SOLVE_TS = 1 << SOLVE_LP; // rows per tile
constexpr int SOLVE_NT = 512;           // threads per workgroup (= eliminations of a tile's level 0)
constexpr int SOLVE_MAXLEV = SOLVE_LP + 1;
constexpr int SOLVE_LP_WIDE = 3;                  // levels per pass while the system is large ...
constexpr int64_t SOLVE_WIDE_ROWS = 1 << 20;      // ... i.e. has at least this many rows (2^18 .. 2^20 measured alike)
// blocks of at most 128 bytes take the latency-bound ("deep") kernels of the sweeps and of the inverse
constexpr bool deep_block(int d, size_t s) { return (size_t)d * d * s <= 128; }

// panel sweeps (cgps_solve_tile_m.h): the panel tile takes the LDS of the single-column tile
constexpr int solve_m_tile_log2(int mc) { return mc <= 2 ? 9 : (mc <= 4 ? 8 : 7); }
constexpr int solve_m_deep_tile_log2(int mc) { return mc >= 8 ? 8 : 9; }
template <int MC> constexpr int solve_m_tile_log2() { return solve_m_tile_log2(MC); }
template <int MC> constexpr int solve_m_deep_tile_log2() { return solve_m_deep_tile_log2(MC); }
constexpr int panel_width(int nrhs) { return nrhs <= 2 ? 2 : (nrhs <= 4 ? 4 : 8); }

constexpr int DEC_LP = 3;               // factorisation, bulk passes: levels per pass over many tiles
constexpr int DEC_TS = 128;             // rows per tile: two per lane
constexpr int DEC_TS_LOG2 = 7;          // levels per pass over few tiles (one survivor per tile)
constexpr int DEC_MAXLEV = 8;           // the last pass takes a system of <= DEC_TS rows to the end: log2(128) + 1
constexpr int64_t DEC_FEW_TILES = 512;  // below this a pass is latency-bound: run all levels of a tile
constexpr int DECL_LP = 8;              // factorisation, in-LDS passes
constexpr int DECL_TS = 1 << DECL_LP;   // 256 rows per tile
constexpr int DECL_MAXLEV = DECL_LP + 1;
// a 256-row tile (R, O, y per row and one spare block) fits the LDS
constexpr bool tile_fits_256(int d, size_t s) { return ((size_t)256 * (2 * d * d + d) + d * d) * s + 4096 <= 160 * 1024; }
// levels per in-LDS pass: blocks whose 256-row tile does not fit (fp64 d = 6, 7, 8) take 64-row tiles
constexpr int decomp_lds_lp(int d, size_t s) {
  return (((size_t)DECL_TS * 2 * d * d + d * d) * s + 4096 <= 160 * 1024) ? DECL_LP : 6;
}
// at or below this many rows a pass of the tiled factorisation is latency-bound and runs in LDS (8 x 8 blocks: the
// in-LDS passes, four lanes per elimination, beat the one-wave-per-tile register passes already at 2^18 rows --
// config 3: 1 490 -> 1 447 us; 4 x 4 fp64: no difference between 2^15 and 2^18)
constexpr int64_t dec_small_rows(int d) { return d == 8 ? 262144 : 32768; }
// in-LDS-only factorisation (fp64 d = 6, 7, 8): levels of more rows than this run one launch per level (d = 7, 8)
constexpr int64_t dec_lds_max_rows(int d) { return d >= 7 ? (int64_t)131072 : ((int64_t)1 << 62); }

constexpr int INV_LP = 3;               // inverse_blocks: levels per fused pass
constexpr int INV_TS = 128;
constexpr int64_t INV_FUSED_MIN_ROWS = 1024;   // a fused inverse pass must produce at least this many rows
constexpr int INVD_MAXLEV = 10;
// rows of the finest level the one-launch coarse end takes: 512 for blocks <= 128 bytes, 256 up to 256 bytes
constexpr int invd_tsl(int d, size_t s) { return deep_block(d, s) ? 9 : 8; }

constexpr int LOGDET_MAX_BLOCKS = 1024;  // cgps_logdet_factor: at most this many workgroups leave a partial sum

// ---- kernel-argument structs: the window of levels one launch covers (offsets in blocks into Dp / Fp / Gp) --------
struct PassLevels {
  int64_t offD[SOLVE_MAXLEV], offF[SOLVE_MAXLEV], offG[SOLVE_MAXLEV], m[SOLVE_MAXLEV];
  int nlev;       // levels this pass runs
  int64_t endD, endF, endG;   // one past the last block of this pass's levels in Dp / Fp / Gp
};
struct DecompLevels {
  int64_t offD[DEC_MAXLEV], offF[DEC_MAXLEV], offG[DEC_MAXLEV];
  int nlev;
};
struct DecompLevelsL {
  int64_t offD[DECL_MAXLEV], offF[DECL_MAXLEV], offG[DECL_MAXLEV];
  int nlev;
};
struct InverseLevels {
  int64_t offD[INV_LP], offF[INV_LP], offG[INV_LP];   // packed-array offsets of levels L, L+1, L+2
};
struct InverseDeepLevels {
  int64_t offD[INVD_MAXLEV], offF[INVD_MAXLEV], offG[INVD_MAXLEV];   // packed-array offsets of the kernel's levels, finest first
  int nlev;
};

// ---- the fused solve + log-det pipeline (cgps_tile.h): rows per stage-1 workgroup, records, partial results --------
// per-block partial results: {sum x^2, sum log pivots, 1 + first failing row or 0, unused}
constexpr int PARTIAL_STRIDE = 4;
// elements of a tile record (RecordLayout<T, D>::STRIDE): boundary row, coupling, owed update, their vectors;
// 16/32-byte aligned
constexpr int record_stride(int d) { return ((3 * d * d + 2 * d + 3) / 4) * 4; }

// TileCfg<T, d>::ROWS1 for a run-time d and scalar size s (cgps_tile.h asserts that the two agree)
constexpr int64_t tile_rows1(int d, size_t s) {
  if (d == 8) return s == 4 ? 128 * 256 / 4 : 64 * 256 / 4;
  if (s == 8 && d == 6) return 32 * 256 / 2;
  if (s == 8 && d == 7) return 16 * 128;
  return 16 * 256;
}
// Below ~2^19 rows the op is pure latency and stage 1's sequential chain of C - 1 eliminations
// per lane is most of it.  Small systems therefore take fewer rows per lane: the smallest C of
// {1, 4, 8, C_full} that keeps the grid within one workgroup per CU (more lanes, shorter chains,
// the same number of records for the final stage or fewer).
constexpr int64_t STAGE1_SMALL_TILES = 256;
inline int stage1_rows_per_lane(int64_t N, int c_full, int lanes) {
  // a few hundred rows: ONE workgroup (a second one costs an inter-workgroup hand-off, ~10 us, to save
  // three or seven eliminations of ~1 us per lane)
  if (c_full > 4 && N > lanes && N <= (int64_t)lanes * 4) return 4;
  if (c_full > 8 && N > lanes && N <= (int64_t)lanes * 8) return 8;
  if (c_full > 4 && N <= STAGE1_SMALL_TILES * lanes * 1) return 1;
  if (c_full > 4 && N <= STAGE1_SMALL_TILES * lanes * 4) return 4;
  if (c_full > 8 && N <= STAGE1_SMALL_TILES * lanes * 8) return 8;
  return c_full;
}
inline int64_t tile_cap(int64_t N, int d, size_t s) { return N / tile_rows1(d, s) + 2 + STAGE1_SMALL_TILES; }

}  // namespace cgps

namespace cgps_host {

// ---- level layout of the packed factor ----------------------------------------------------------
struct Layout {
  int nlevels;
  int64_t ms[CGPS_MAX_LEVELS], offD[CGPS_MAX_LEVELS + 1], offF[CGPS_MAX_LEVELS + 1], offG[CGPS_MAX_LEVELS + 1];
};

inline void make_layout(int64_t N, Layout& L) {
  int l = 0;
  int64_t m = N, oD = 0, oF = 0, oG = 0;
  for (;;) {
    L.ms[l] = m;
    L.offD[l] = oD; L.offF[l] = oF; L.offG[l] = oG;
    oD += (m + 1) / 2; oF += m / 2; oG += (m - 1) / 2;
    ++l;
    if (m == 1) break;
    m /= 2;
  }
  L.nlevels = l;
  L.offD[l] = oD; L.offF[l] = oF; L.offG[l] = oG;
}

// the window of levels a kernel sees, starting at level lvl: as many entries as the kernel-argument struct holds,
// levels past the coarsest one repeat it
template <typename W>
void fill_window(const Layout& L, int lvl, W& w) {
  constexpr int n = (int)(sizeof(w.offD) / sizeof(w.offD[0]));
  for (int j = 0; j < n; ++j) {
    const int l = lvl + j < L.nlevels ? lvl + j : L.nlevels - 1;
    w.offD[j] = L.offD[l]; w.offF[j] = L.offF[l]; w.offG[j] = L.offG[l];
  }
}

inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }
inline size_t max_bytes(size_t a, size_t b) { return a > b ? a : b; }
inline int64_t level_blocks(int64_t m) { return ((m + 1) / 2 + cgps::LEVEL_THREADS - 1) / cgps::LEVEL_THREADS; }

// ---- workspaces: named regions (offset and bytes from the start of the workspace) and their total ---------------------
struct Region {
  size_t off, bytes;
  size_t end() const { return off + bytes; }
};
template <typename T>
T* at(char* ws, const Region& r) { return reinterpret_cast<T*>(ws + r.off); }

// level-wise reduction, decompose (with_mats), forward sweep (with_vec): per-block partial sums and two ping-pong
// buffers of capA / capB rows, each row 2 d^2 (R, O) and / or d nrhs (y) scalars
struct LevelWs {
  Region partial;                     // [total blocks + 1][2] doubles
  Region buf[2];                      // ping-pong level buffers (the tiled paths: records / surviving rows of a pass)
  int64_t cap[2];                     // rows
  size_t total;
};
inline LevelWs level_ws(int64_t N, int d, size_t s, bool with_mats, bool with_vec, int nrhs = 1) {
  LevelWs w{};
  Layout L;
  make_layout(N, L);
  int64_t nb = 0;
  for (int l = 0; l < L.nlevels; ++l) nb += level_blocks(L.ms[l]);
  w.cap[0] = N / 2 + 1;
  w.cap[1] = N / 4 + 1;
  const size_t per_row = (with_mats ? 2 * (size_t)d * d : 0) + (with_vec ? (size_t)d * nrhs : 0);
  w.partial = {0, align_up((size_t)(nb + 1) * 16)};
  w.buf[0] = {w.partial.end(), align_up(per_row * s * w.cap[0])};
  w.buf[1] = {w.buf[0].end(), align_up(per_row * s * w.cap[1])};
  w.total = w.buf[1].end();
  return w;
}
inline LevelWs decompose_ws(int64_t N, int d, size_t s) { return level_ws(N, d, s, true, false); }
inline LevelWs halfsolve_ws(int64_t N, int d, size_t s) { return level_ws(N, d, s, false, true); }

// backward sweep: both ping-pong buffers hold a level-1 vector (the partial sums of the forward sweep stay in front,
// so that solve() runs both sweeps on one workspace); pass / level p > 0 leaves its solution in x_of(p)
struct BacksolveWs {
  Region partial, buf[2];
  size_t total;
  const Region& x_of(int p) const { return buf[p & 1]; }
};
inline BacksolveWs backsolve_ws(int64_t N, int d, size_t s) {
  BacksolveWs w{};
  w.partial = halfsolve_ws(N, d, s).partial;
  const size_t one = align_up((size_t)d * s * (N / 2 + 1));
  w.buf[0] = {w.partial.end(), one};
  w.buf[1] = {w.buf[0].end(), one};
  w.total = w.buf[1].end();
  return w;
}

// what serves either sweep (CGPS_OP_BACKSOLVE asks for this much)
inline size_t sweeps_ws_bytes(int64_t N, int d, size_t s) {
  return max_bytes(halfsolve_ws(N, d, s).total, backsolve_ws(N, d, s).total);
}

// solve(), one column: the intermediate (CRR) vector, then one region both sweeps use one after the other
struct SolveWs {
  Region crr, sweep;
  size_t total;
};
inline SolveWs solve_ws(int64_t N, int d, size_t s) {
  SolveWs w{};
  w.crr = {0, align_up((size_t)N * d * s)};
  w.sweep = {w.crr.end(), sweeps_ws_bytes(N, d, s)};
  w.total = w.sweep.end();
  return w;
}

// panel sweeps (nrhs >= 2, mc columns at a time): partial sums | two ping-pong buffers of [N/2 + 2][d][mc] | solve():
// the intermediate panel [N][d][mc]
struct PanelWs {
  Region partial, buf[2], crr;
  size_t total;
};
inline PanelWs panel_ws(int64_t N, int d, size_t s, int nrhs, bool solve) {
  PanelWs w{};
  const int mc = cgps::panel_width(nrhs), chunks = (nrhs + mc - 1) / mc;
  // grids of all passes of all chunks: < 1.2 N / 128 tiles per chunk (the smallest tile has 128 rows)
  const int64_t tiles = (N / 128 + 64) * 2;
  w.partial = {0, align_up((size_t)(tiles * chunks + 2) * 16)};
  const size_t one = align_up((size_t)(N / 2 + 2) * d * mc * s);
  w.buf[0] = {w.partial.end(), one};
  w.buf[1] = {w.buf[0].end(), one};
  w.crr = {w.buf[1].end(), solve ? align_up((size_t)N * d * mc * s) : 0};
  w.total = w.crr.end();
  return w;
}

// cgps_decompose_solve: what decompose and the two sweeps need, one after the other, then the right-hand side of the
// rows that survive the first pass (ynext) and what each of its tiles owes the previous one (owedy)
struct DecomposeSolveWs {
  Region main, ynext, owedy;
  size_t total;
};
inline DecomposeSolveWs decompose_solve_ws(int64_t N, int d, size_t s) {
  DecomposeSolveWs w{};
  w.main = {0, align_up(max_bytes(decompose_ws(N, d, s).total, sweeps_ws_bytes(N, d, s)))};
  w.ynext = {w.main.end(), align_up((size_t)(N / 8 + 16) * d * s)};
  w.owedy = {w.ynext.end(), align_up((size_t)(N / 128 + 2) * d * s)};
  w.total = w.owedy.end();
  return w;
}

// inverse_blocks: two ping-pong buffers, each Sigma's diagonal blocks [cap][d][d] then its off-diagonal blocks
struct InverseWs {
  Region buf[2];
  int64_t cap;                        // rows; the off-diagonal blocks of a buffer start cap d^2 scalars into it
  size_t total;
};
inline InverseWs inverse_ws(int64_t N, int d, size_t s) {
  InverseWs w{};
  w.cap = N / 2 + 1;
  const size_t one = align_up((size_t)2 * d * d * s * w.cap);
  w.buf[0] = {0, one};
  w.buf[1] = {one, one};
  w.total = 2 * one;
  return w;
}

// log-det of a stored factor: one partial sum per workgroup and the two sums behind them
struct LogdetFactorWs {
  Region partial;
  size_t total;
};
inline LogdetFactorWs logdet_factor_ws() {
  LogdetFactorWs w{};
  w.partial = {0, align_up((size_t)(cgps::LOGDET_MAX_BLOCKS + 2) * 16)};
  w.total = w.partial.end();
  return w;
}

// the fused pipeline: partial results of every stage, then two record buffers the stages ping-pong between
struct TileWs {
  Region partial, recA, recB;
  int64_t tiles_cap;                  // stage-1 workgroups the buffers are sized for
  size_t total;
};
inline TileWs tile_ws(int64_t N, int d, size_t s) {
  TileWs w{};
  w.tiles_cap = cgps::tile_cap(N, d, s);
  const size_t rec = (size_t)(w.tiles_cap + 2) * cgps::record_stride(d) * s;
  w.partial = {0, align_up((size_t)(2 * w.tiles_cap + 8) * cgps::PARTIAL_STRIDE * sizeof(double))};
  w.recA = {w.partial.end(), rec};
  w.recB = {w.recA.end(), rec};
  w.total = w.partial.end() + align_up(2 * rec);
  return w;
}
// its pair form (cgps_leg_mahal_logdet_pair): two pipelines, `stride` bytes apart
struct TilePairWs {
  TileWs one;
  size_t stride, total;
};
inline TilePairWs tile_pair_ws(int64_t N, int d, size_t s) {
  TilePairWs w{};
  w.one = tile_ws(N, d, s);
  w.stride = align_up(w.one.total);
  w.total = 2 * w.stride;
  return w;
}
// cgps_mahal_logdet takes the fused pipeline or, where that is not built, the level-wise reduction
inline size_t mahal_logdet_ws_bytes(int64_t N, int d, size_t s) {
  return max_bytes(level_ws(N, d, s, true, true).total, tile_ws(N, d, s).total);
}

// what include/cgps.h states for the pair forms: twice cgps_mahal_logdet's, each half rounded up to 256 bytes
inline size_t leg_pair_ws_bytes(int64_t N, int d, size_t s) { return 2 * align_up(mahal_logdet_ws_bytes(N, d, s)); }
// (The entry points hold the caller to these stated sizes, not to the sometimes smaller part that the path taken cuts up.)

// ---- cgps_leg_filter_scan (cgps_leg_filter_scan.h): the time-parallel filter's levels of elements and chunk states ----
// Level 0 holds one element per (model, chunk), level l + 1 one per group of `fanout` elements of level l, up to the
// first level of at most `fanout` elements (one group).  An element is filter_scan_elem_scalars(d) scalars (A, b, C,
// eta, J, the reset flag) and a level is stored value-major, [M][scalars][n[l]], so that the lanes of a wave, which
// own neighbouring elements, read neighbouring addresses.  Behind the levels: what the final-rows phase reads per chunk
// (t0 [chunks], m0 [M][chunks][d], P0 [M][chunks][d][d]) and leaves per chunk (loglik [M][chunks] doubles, m_end, P_end).
constexpr int FILTER_SCAN_MAX_LEVELS = 40;      // fanout >= 2 and at most 2^36 chunks: 37 levels
constexpr int filter_scan_elem_scalars(int d) { return 3 * d * d + 2 * d + 1; }
struct FilterScanWs {
  int levels;
  int64_t n[FILTER_SCAN_MAX_LEVELS];            // elements per model of every level
  Region elem[FILTER_SCAN_MAX_LEVELS];
  Region t0, m0, P0, loglik, m_end, P_end;
  size_t total;
};
inline FilterScanWs filter_scan_ws(int64_t chunks, int64_t M, int d, size_t s, int64_t fanout) {
  FilterScanWs w{};
  size_t off = 0;
  auto cut = [&](size_t bytes) {
    Region r{off, align_up(bytes)};
    off = r.end();
    return r;
  };
  int64_t n = chunks;
  for (;;) {
    w.n[w.levels] = n;
    w.elem[w.levels] = cut((size_t)M * filter_scan_elem_scalars(d) * (size_t)n * s);
    ++w.levels;
    if (n <= fanout || w.levels == FILTER_SCAN_MAX_LEVELS) break;
    n = (n + fanout - 1) / fanout;
  }
  w.t0 = cut((size_t)chunks * s);
  w.m0 = cut((size_t)M * chunks * d * s);
  w.P0 = cut((size_t)M * chunks * d * d * s);
  w.loglik = cut((size_t)M * chunks * sizeof(double));
  w.m_end = cut((size_t)M * chunks * d * s);
  w.P_end = cut((size_t)M * chunks * d * d * s);
  w.total = off;
  return w;
}

// ---- cgps_leg_filter_adjoint (cgps_leg_filter_adjoint.h): E of the gap before every row, then E_bar over it -----------
// One d x d block per (model, row): [M][R][d][d].
inline size_t filter_adjoint_ws_bytes(int64_t R, int64_t B, int64_t M, int d, int obs, size_t s) {
  (void)B;
  (void)obs;
  return align_up((size_t)M * (size_t)R * d * d * s);
}

// ---- passes of the substitution sweeps -------------------------------------------------------------------------
// Forward pass p reads the surviving rows of pass p - 1 (the caller's y for p = 0) and, when a pass follows, writes
// [nsurv][D] surviving rows, one spare row, then [tiles][D] owed vectors into buf[p & 1] of its workspace.  Backward
// pass p reads the solution of pass p + 1 from buf[(p + 1) & 1] and writes its own [rows][D] into buf[p & 1] (p = 0:
// into the caller's x).
constexpr int SOLVE_MAX_PASSES = 8;
struct SolvePasses {
  int np;
  int ts[SOLVE_MAX_PASSES];                 // rows per tile of the pass
  bool deep[SOLVE_MAX_PASSES];              // latency-bound form (every factor block requested up front)
  cgps::PassLevels lv[SOLVE_MAX_PASSES];
  int64_t rows[SOLVE_MAX_PASSES], tiles[SOLVE_MAX_PASSES], nsurv[SOLVE_MAX_PASSES];
  static int buf(int p) { return p & 1; }
  // bytes from the start of buf[p & 1] the pass writes; row_bytes = d * columns * sizeof(T)
  size_t forward_write_bytes(int p, size_t row_bytes) const {
    return p + 1 < np ? (size_t)(nsurv[p] + 1 + tiles[p]) * row_bytes : 0;
  }
  size_t backward_write_bytes(int p, size_t row_bytes) const { return p > 0 ? (size_t)rows[p] * row_bytes : 0; }
};

// deep_tiles: passes of at most this many tiles take the latency-bound kernels (0: never): one
// 1024-row tile when the rows fit it, 512-row tiles (twice the CUs pulling the factor) otherwise
// ts_deep / lp_deep (panel sweeps): passes of at most `deep_tiles_m` such tiles take them, in the latency-bound form
inline void make_passes(const Layout& L, SolvePasses& P, int wide_lp, int ts_in = cgps::SOLVE_TS, int lp_in = cgps::SOLVE_LP,
                        int64_t deep_tiles = 0, int ts_deep = 0, int lp_deep = 0, int64_t deep_tiles_m = 0) {
  P.np = 0;
  int lvl = 0;
  while (lvl < L.nlevels) {
    const int64_t rows = L.ms[lvl];
    const int remaining = L.nlevels - lvl;
    int ts = ts_in, lp = lp_in;
    bool deep = false;
    if (deep_tiles > 0) {
      if (rows <= ts_in) deep = true;
      else if ((rows + ts_in / 2 - 1) / (ts_in / 2) <= deep_tiles) { deep = true; ts = ts_in / 2; lp = lp_in - 1; }
    }
    if (ts_deep > 0 && rows < cgps::SOLVE_WIDE_ROWS && (rows + ts_deep - 1) / ts_deep <= deep_tiles_m) {
      deep = true; ts = ts_deep; lp = lp_deep;
    }
    P.ts[P.np] = ts;
    P.deep[P.np] = deep;
    // many tiles: a few levels per pass (every lane busy, few barrier-separated latency
    // exposures, the factor still read once); few tiles: all ten levels of a tile
    const int nl = (rows <= ts) ? remaining : (rows >= cgps::SOLVE_WIDE_ROWS ? wide_lp : lp);   // <= lp + 1
    cgps::PassLevels& pl = P.lv[P.np];
    pl.nlev = nl;
    pl.endD = L.offD[lvl + nl];
    pl.endF = L.offF[lvl + nl < L.nlevels ? lvl + nl : L.nlevels - 1];
    pl.endG = L.offG[lvl + nl < L.nlevels ? lvl + nl : L.nlevels - 1];
    fill_window(L, lvl, pl);
    for (int j = 0; j < cgps::SOLVE_MAXLEV; ++j) pl.m[j] = lvl + j < L.nlevels ? L.ms[lvl + j] : 0;
    P.rows[P.np] = rows;
    P.tiles[P.np] = (rows + ts - 1) / ts;
    P.nsurv[P.np] = rows >> nl;           // rows of the next pass
    ++P.np;
    lvl += nl;
  }
}
// one column; deep_tiles: the device's CU count where the block size has the deep kernels and they are enabled, else 0
inline void plan_sweep(const Layout& L, SolvePasses& P, int64_t deep_tiles) {
  make_passes(L, P, cgps::SOLVE_LP_WIDE, cgps::SOLVE_TS, cgps::SOLVE_LP, deep_tiles);
}
// passes of a panel sweep over at most this many 2^TSLD-row tiles (two per CU) take the latency-bound kernels
// (cgps_solve_tile_m.h: every factor block requested up front)
// Measured at 2^20 rows, d = 4 fp64 (tools/prof_case.py --op solve --nrhs m): two columns 285 -> 257 us; four columns
// 402 -> 451 us, eight 631 -> 740-775 us (two 64 KB tiles per CU, each a chain of eight dependent levels on wide panels,
// against the four or five smaller tiles per CU the regular kernels keep in flight; LDS bank conflicts are not it:
// padding the panel rows changed nothing, 626 against 635 us): two-column panels only.
inline int64_t panel_deep_tiles(int mc, bool deep_enabled) { return (mc <= 2 && deep_enabled) ? 512 : 0; }
// mc columns; deep_block: the block size has the deep kernels, deep_enabled: they are not switched off
inline void plan_panel_sweep(const Layout& L, SolvePasses& P, int mc, bool deep_block, bool deep_enabled) {
  const int tsl = cgps::solve_m_tile_log2(mc), tsld = cgps::solve_m_deep_tile_log2(mc);
  make_passes(L, P, cgps::SOLVE_LP_WIDE, 1 << tsl, tsl, 0, deep_block ? 1 << tsld : 0, tsld, panel_deep_tiles(mc, deep_enabled));
}

// ---- cgps_sample (cgps_sample_tile.h): the backward panel sweep with ALL column chunks of a pass in one launch ------
// Chunk c (columns [c mc, c mc + mc)) has its own slice of the two coarse-solution buffers: backward pass p > 0 writes
// its [rows[p]][d][mc] solution into slice c of buf[p & 1] and pass p - 1 reads it there, so buf[b] is sized for the
// largest pass of its parity (exactly, from the plan) times the chunks of a launch.  At most SAMPLE_CHUNK_GROUP chunks
// (1024 columns) go into one launch, and the workspace never holds more than that many slices: more samples than that
// run group after group on the same slices (launches = passes x groups).  With the three-level first pass of a system
// of >= 2^20 rows a slice pair is (1/8 + 1/64) of the chunk's output, so the workspace stays below a fifth of x.
constexpr int64_t SAMPLE_CHUNK_GROUP = 128;
struct SampleWs {
  Region buf[2];
  size_t slice[2];                    // bytes from one chunk's slice of buf[b] to the next
  int mc;                             // panel width
  int64_t chunks, group;              // column chunks of the call; chunks per launch
  size_t total;
};
inline SampleWs sample_ws(int64_t N, int d, size_t s, int64_t nrhs) {
  SampleWs w{};
  w.mc = cgps::panel_width(nrhs > 8 ? 8 : (int)nrhs);
  w.chunks = (nrhs + w.mc - 1) / w.mc;
  w.group = w.chunks < SAMPLE_CHUNK_GROUP ? w.chunks : SAMPLE_CHUNK_GROUP;
  Layout L;
  make_layout(N, L);
  SolvePasses P;
  plan_panel_sweep(L, P, w.mc, false, false);
  int64_t cap[2] = {0, 0};
  for (int p = 1; p < P.np; ++p)
    if (P.rows[p] > cap[p & 1]) cap[p & 1] = P.rows[p];
  for (int b = 0; b < 2; ++b) w.slice[b] = align_up((size_t)cap[b] * d * w.mc * s);
  w.buf[0] = {0, w.slice[0] * (size_t)w.group};
  w.buf[1] = {w.buf[0].end(), w.slice[1] * (size_t)w.group};
  w.total = max_bytes(w.buf[1].end(), 256);
  return w;
}

// ---- passes of the factorisation ---------------------------------------------------------------------------------
// A pass reads the caller's Rs / Os (in < 0) or what the previous pass left in buf[in] of decompose_ws(), and writes
// into buf[out] (out < 0: nothing, the pass runs to the end): one launch per level writes the next level's rows
// (R [cap][d][d], then O), the tile passes write `records` tile records of record_stride(d) scalars.
enum class DecKind { Level, Bulk, BulkRhs, Lds };   // level_kernel, decomp_tile_kernel (RHS: with the forward sweep of y), decomp_lds_kernel
struct DecPass {
  DecKind kind;
  int first, nlev;                    // levels [first, first + nlev)
  int64_t rows, tiles;                // rows of level `first`; tiles (Level: workgroups) of the pass
  int in, out;                        // buffers read / written, -1: none
  int64_t records_in, records;        // tile records read / written
  int spt_in;                         // records each tile of the previous pass left
  size_t write_bytes;                 // bytes from the start of buf[out] the pass writes
};
struct DecPlan {
  LevelWs ws;
  int np;
  DecPass pass[CGPS_MAX_LEVELS];
};

// Block sizes whose 256-row tile fits the LDS (tile_fits_256): bulk passes (cgps_decomp_tile.h) while the rows are many,
// in-LDS passes (cgps_decomp_lds.h) for the latency-bound tail.  with_rhs (cgps_decompose_solve): the first pass, when
// it is a bulk pass of DEC_LP levels, also carries the forward substitution of y through its levels.
// Larger blocks (fp64 d = 6, 7, 8): in-LDS passes of 2^lp-row tiles only; levels of more than dec_lds_max_rows(d) rows
// run one launch per level first, alternating between the two level buffers, which are also the record buffers.
inline void plan_decompose(int64_t N, int d, size_t s, bool with_rhs, DecPlan& P) {
  P.ws = decompose_ws(N, d, s);
  P.np = 0;
  Layout L;
  make_layout(N, L);
  const bool fits = cgps::tile_fits_256(d, s);
  const int lp = cgps::decomp_lds_lp(d, s);
  int64_t n_rec = 0;
  int lvl = 0, spt_in = 1, in = -1;
  while (lvl < L.nlevels) {
    const int p = P.np++;
    DecPass& q = P.pass[p];
    const int64_t rows = L.ms[lvl];
    const int remaining = L.nlevels - lvl;
    q = DecPass{DecKind::Lds, lvl, 1, rows, 0, in, p & 1, n_rec, 0, spt_in, 0};
    if (!fits && lvl < L.nlevels - 1 && rows > cgps::dec_lds_max_rows(d)) {
      q.kind = DecKind::Level;
      q.tiles = level_blocks(rows);
      // the next level's n rows: R [n][d][d] at the start of the buffer, O [n - 1][d][d] behind its cap rows of R
      q.write_bytes = ((size_t)P.ws.cap[q.out] + (size_t)(L.ms[lvl + 1] - 1)) * d * d * s;
    } else if (!fits || rows <= cgps::dec_small_rows(d)) {
      // latency-bound tail (or a small system): tiles in LDS, lp levels per launch, four waves per elimination;
      // one record per tile, none when one tile takes it to the end (nobody reads it)
      q.tiles = (rows + (1 << lp) - 1) >> lp;
      q.nlev = (q.tiles == 1) ? remaining : lp;                      // <= lp + 1
      q.records = (q.tiles == 1) ? 0 : q.tiles;
      spt_in = 1;
    } else {
      const int64_t g = (rows + cgps::DEC_TS - 1) / cgps::DEC_TS;
      const bool top = g == 1;                                       // one tile takes it to the end
      // many tiles: a few levels per pass keep the lanes busy; few tiles: all levels of a tile
      const int nl = top ? remaining : (g >= cgps::DEC_FEW_TILES ? cgps::DEC_LP : cgps::DEC_TS_LOG2);   // <= DEC_MAXLEV
      q.kind = (p == 0 && with_rhs && !top && nl == cgps::DEC_LP) ? DecKind::BulkRhs : DecKind::Bulk;
      q.tiles = g;
      q.nlev = nl;
      // every tile leaves DEC_TS >> nl records, the last one what survives of it, at least one
      const int64_t spt = cgps::DEC_TS >> nl;
      const int64_t last = (rows - (g - 1) * cgps::DEC_TS) >> nl;
      q.records = top ? 0 : (g - 1) * spt + (last > 0 ? last : 1);
      spt_in = (int)(spt > 0 ? spt : 1);
    }
    if (q.kind != DecKind::Level) {
      // rule of the kernels' store addresses: decomp_tile_kernel writes record tile * spt + m (m < survivors of the tile)
      // and the owed update in record tile * spt of every tile; decomp_lds_kernel record blockIdx.x
      q.write_bytes = (size_t)q.records * cgps::record_stride(d) * s;
      if (q.records == 0) q.out = -1;
    }
    in = q.out;
    n_rec = q.records;
    lvl += q.nlev;
  }
}

// ---- passes of inverse_blocks (coarse to fine) ------------------------------------------------------------------------
// A pass reads Sigma of level first + nlev from buf[in] of inverse_ws() (in < 0: it starts at the coarsest level) and
// writes Sigma of level `first` into buf[out] (out < 0: level 0, into the caller's arrays): `rows` diagonal blocks at
// the start of the buffer, rows - 1 off-diagonal blocks behind its cap diagonal blocks.
enum class InvKind { Deep, Tile, Level };   // inverse_deep_kernel, the INV_LP-levels-per-launch kernels, inverse_level_kernel
struct InvPass {
  InvKind kind;
  int first, nlev;
  int64_t rows;                       // rows of level `first`
  int in, out;
  size_t write_bytes;
};
struct InvPlan {
  InverseWs ws;
  int np;
  InvPass pass[CGPS_MAX_LEVELS];
};
// fused: the block size has (and may use) the INV_LP-levels-per-launch kernels; fused_ok: they are not switched off for
// this form; deep: the block size has the one-launch coarse end and it is enabled
inline void plan_inverse(int64_t N, int d, size_t s, bool fused, bool fused_ok, bool deep, InvPlan& P) {
  P.ws = inverse_ws(N, d, s);
  P.np = 0;
  Layout L;
  make_layout(N, L);
  const size_t dd = (size_t)d * d;
  int p = 0, in = -1;
  auto add = [&](InvKind kind, int first, int nlev) {
    InvPass& q = P.pass[P.np++];
    q = InvPass{kind, first, nlev, L.ms[first], in, first == 0 ? -1 : p, 0};
    if (q.out >= 0) q.write_bytes = ((size_t)P.ws.cap + (size_t)(q.rows - 1)) * dd * s;
    in = q.out >= 0 ? q.out : in;
    p ^= 1;
  };
  int l_start = L.nlevels - 1;
  if (deep) {
    // the coarse end in ONE launch (inverse_deep_kernel): from the single row of the coarsest level down
    // to the finest level of at most INVD_TS rows at which the three-levels-per-launch passes can take
    // over (a multiple of INV_LP), or to level 0 of a small system
    const int64_t invd_ts = (int64_t)1 << cgps::invd_tsl(d, s);
    int lf = -1;
    for (int l = 0; l < L.nlevels; ++l)
      if (L.ms[l] <= invd_ts && (l % cgps::INV_LP == 0 || !fused)) { lf = l; break; }
    if (lf < 0)
      for (int l = 0; l < L.nlevels; ++l)
        if (L.ms[l] <= invd_ts) { lf = l; break; }
    if (lf >= 0 && L.nlevels - lf <= cgps::INVD_MAXLEV) {
      add(InvKind::Deep, lf, L.nlevels - lf);
      l_start = lf - 1;
    }
  }
  // The coarse levels one launch each (latency-bound, little data); once a level that is a
  // multiple of INV_LP above level 0 is reached and the rows get many, INV_LP levels per launch
  // (cgps_inverse_tile.h): those passes read 1/8 of what they write instead of ping-ponging every
  // level's Sigma through HBM.
  for (int l = l_start; l >= 0;) {
    const int have = l + 1;                               // the previous pass left Sigma of this level
    if (fused && fused_ok && P.np > 0 && have % cgps::INV_LP == 0 && L.ms[have] >= 1 &&
        L.ms[have - cgps::INV_LP] >= cgps::INV_FUSED_MIN_ROWS) {
      add(InvKind::Tile, have - cgps::INV_LP, cgps::INV_LP);
      l = have - cgps::INV_LP - 1;
      continue;
    }
    add(InvKind::Level, l, 1);
    --l;
  }
}

}  // namespace cgps_host
