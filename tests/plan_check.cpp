// Host-only check of cgps_plan.h (compiled and run by tests/test_plan.py with a plain C++17 compiler; that it
// compiles at all is the proof that the header needs nothing from HIP).  For every plan, over N, d, scalar size, panel
// width and CU count: regions are disjoint and inside `total`, every pass's write extent is inside its region, a pass
// never reads the region it writes, and the region solve() hands to its fused top pass is the one the backward
// sweep's plan reads for that pass.  Prints every failing case; exit status 1 if there is one.
#include <cstdio>
#include <vector>

#include "cgps_plan.h"

using namespace cgps_host;

static long g_checks = 0, g_failed = 0;
static int64_t g_N;
static int g_d;
static size_t g_s;
#define CHECK(cond, ...)                                                              \
  do {                                                                                \
    ++g_checks;                                                                       \
    if (!(cond)) {                                                                    \
      if (++g_failed <= 50) {                                                         \
        printf("FAIL N=%lld d=%d s=%zu: %s: ", (long long)g_N, g_d, g_s, #cond);      \
        printf(__VA_ARGS__);                                                          \
        printf("\n");                                                                 \
      }                                                                               \
    }                                                                                 \
  } while (0)

static bool overlap(const Region& a, const Region& b) { return a.bytes && b.bytes && a.off < b.end() && b.off < a.end(); }

// regions in order, disjoint, inside total
static void check_regions(const char* what, const std::vector<Region>& r, size_t total) {
  for (size_t i = 0; i < r.size(); ++i) {
    CHECK(r[i].end() <= total, "%s region %zu ends at %zu > total %zu", what, i, r[i].end(), total);
    for (size_t j = i + 1; j < r.size(); ++j) CHECK(!overlap(r[i], r[j]), "%s regions %zu and %zu overlap", what, i, j);
  }
}

static void check_levelwise(int64_t N, int d, size_t s) {
  Layout L;
  make_layout(N, L);
  const size_t dd = (size_t)d * d;
  // mahal_logdet level by level: R, O and y of the next level
  for (int vec = 0; vec < 2; ++vec) {
    const LevelWs w = level_ws(N, d, s, true, vec);
    check_regions("level_ws", {w.partial, w.buf[0], w.buf[1]}, w.total);
    int64_t nb = 0;
    for (int l = 0; l < L.nlevels; ++l) {
      nb += level_blocks(L.ms[l]);
      const int64_t nn = l + 1 < L.nlevels ? L.ms[l + 1] : 0, cap = w.cap[l & 1];
      CHECK(nn <= cap, "level %d: %lld rows > cap %lld", l, (long long)nn, (long long)cap);
      const size_t extent = nn == 0 ? 0 : (vec ? (2 * cap * dd + nn * d) : (cap * dd + (nn - 1) * dd)) * s;
      CHECK(extent <= w.buf[l & 1].bytes, "level %d writes %zu > %zu", l, extent, w.buf[l & 1].bytes);
    }
    CHECK((size_t)(nb + 1) * 16 <= w.partial.bytes, "partial sums %lld blocks", (long long)nb);
  }
  // the sweeps level by level
  const LevelWs h = halfsolve_ws(N, d, s);
  const BacksolveWs b = backsolve_ws(N, d, s);
  check_regions("halfsolve_ws", {h.partial, h.buf[0], h.buf[1]}, h.total);
  check_regions("backsolve_ws", {b.partial, b.buf[0], b.buf[1]}, b.total);
  CHECK(b.partial.off == h.partial.off && b.partial.bytes == h.partial.bytes, "the sweeps' partial sums differ");
  for (int l = 0; l < L.nlevels; ++l) {
    const int64_t nn = l + 1 < L.nlevels ? L.ms[l + 1] : 0;
    CHECK((size_t)nn * d * s <= h.buf[l & 1].bytes, "forward level %d", l);
    if (l > 0) CHECK((size_t)L.ms[l] * d * s <= b.x_of(l).bytes, "backward level %d", l);
    if (l > 0) CHECK(&b.x_of(l) != &b.x_of(l + 1), "backward level %d reads what it writes", l);
  }
}

static void check_sweep(const char* what, const SolvePasses& P, const Region (&fwd)[2], const Region (&bwd)[2], const Region& partial,
                        size_t row_bytes, int chunks) {
  CHECK(P.np >= 1 && P.np <= SOLVE_MAX_PASSES, "%s: %d passes", what, P.np);
  int64_t tiles = 0;
  for (int p = 0; p < P.np; ++p) {
    tiles += P.tiles[p];
    CHECK(P.lv[p].nlev <= cgps::SOLVE_MAXLEV, "%s pass %d: %d levels", what, p, P.lv[p].nlev);
    CHECK(P.forward_write_bytes(p, row_bytes) <= fwd[P.buf(p)].bytes, "%s forward pass %d writes %zu > %zu", what, p,
          P.forward_write_bytes(p, row_bytes), fwd[P.buf(p)].bytes);
    CHECK(P.backward_write_bytes(p, row_bytes) <= bwd[P.buf(p)].bytes, "%s backward pass %d writes %zu > %zu", what, p,
          P.backward_write_bytes(p, row_bytes), bwd[P.buf(p)].bytes);
    // pass p reads buffer (p - 1) & 1 going forward, (p + 1) & 1 going backward: never p & 1
    CHECK(P.buf(p) != P.buf(p + 1), "%s pass %d reads the buffer it writes", what, p);
    if (p > 0) CHECK(P.rows[p] == P.nsurv[p - 1], "%s pass %d: %lld rows, %lld survived", what, p, (long long)P.rows[p], (long long)P.nsurv[p - 1]);
  }
  CHECK((size_t)(tiles * chunks + 1) * 16 <= partial.bytes, "%s: %lld partial sums x %d", what, (long long)tiles, chunks);
}

static void check_sweeps(int64_t N, int d, size_t s) {
  Layout L;
  make_layout(N, L);
  const LevelWs h = halfsolve_ws(N, d, s);
  const BacksolveWs b = backsolve_ws(N, d, s);
  const SolveWs sv = solve_ws(N, d, s);
  check_regions("solve_ws", {sv.crr, sv.sweep}, sv.total);
  CHECK((size_t)N * d * s <= sv.crr.bytes, "CRR vector");
  CHECK(h.total <= sv.sweep.bytes && b.total <= sv.sweep.bytes, "sweep region %zu < %zu / %zu", sv.sweep.bytes, h.total, b.total);
  const int cus[] = {0, 1, 64, 256, 304};      // 0: the deep kernels switched off / not built for the block size
  for (int c : cus) {
    if (c > 0 && !cgps::deep_block(d, s)) continue;
    SolvePasses P;
    plan_sweep(L, P, c);
    check_sweep("sweep", P, h.buf, b.buf, h.partial, (size_t)d * s, 1);
    // solve(): a single-tile deep last pass runs both sweeps (solve_top_kernel): it reads what forward pass p - 1 left
    // in the forward plan's buffer and writes its solution where the backward plan reads it for pass p - 1
    const int p = P.np - 1;
    if (c > 0 && P.tiles[p] == 1 && P.deep[p] && p > 0) {
      const Region& xtop = b.x_of(p);
      CHECK((size_t)P.rows[p] * d * s <= xtop.bytes, "fused top pass writes %lld rows", (long long)P.rows[p]);
      const Region in{h.buf[P.buf(p - 1)].off, P.forward_write_bytes(p - 1, (size_t)d * s)};
      CHECK(!overlap(in, xtop), "fused top pass %d writes over its input", p);
      CHECK(!overlap(h.partial, xtop), "fused top pass %d writes over the partial sums", p);
      CHECK(xtop.off == b.buf[(p - 1 + 1) & 1].off, "backward pass %d reads another region than the top pass wrote", p - 1);
    }
  }
  const int widths[] = {2, 3, 4, 5, 8, 9, 17};
  for (int nrhs : widths)
    for (int solve = 0; solve < 2; ++solve)
      for (int enabled = 0; enabled < 2; ++enabled) {
        const PanelWs w = panel_ws(N, d, s, nrhs, solve);
        const int mc = cgps::panel_width(nrhs), chunks = (nrhs + mc - 1) / mc;
        check_regions("panel_ws", {w.partial, w.buf[0], w.buf[1], w.crr}, w.total);
        if (solve) CHECK((size_t)N * d * mc * s <= w.crr.bytes, "CRR panel");
        SolvePasses P;
        plan_panel_sweep(L, P, mc, cgps::deep_block(d, s), enabled);
        check_sweep("panel sweep", P, w.buf, w.buf, w.partial, (size_t)d * mc * s, chunks);
      }
}

static void check_dec_plan(const char* what, const DecPlan& P, int d, size_t s) {
  check_regions(what, {P.ws.partial, P.ws.buf[0], P.ws.buf[1]}, P.ws.total);
  CHECK(P.np >= 1 && P.np <= CGPS_MAX_LEVELS, "%s: %d passes", what, P.np);
  int lvl = 0, prev_out = -1;
  int64_t prev_records = 0, level_blocks_sum = 0;
  for (int p = 0; p < P.np; ++p) {
    const DecPass& q = P.pass[p];
    CHECK(q.first == lvl, "%s pass %d starts at level %d, not %d", what, p, q.first, lvl);
    CHECK(q.in == prev_out, "%s pass %d reads buffer %d, pass before wrote %d", what, p, q.in, prev_out);
    CHECK(q.records_in == prev_records, "%s pass %d reads %lld records of %lld", what, p, (long long)q.records_in, (long long)prev_records);
    CHECK(q.out < 0 || q.out != q.in, "%s pass %d reads the buffer it writes", what, p);
    CHECK(q.nlev <= (q.kind == DecKind::Lds ? cgps::decomp_lds_lp(d, s) + 1 : (q.kind == DecKind::Level ? 1 : cgps::DEC_MAXLEV)), "%s pass %d: %d levels", what, p, q.nlev);
    if (q.kind != DecKind::Level) CHECK(q.write_bytes == (size_t)q.records * cgps::record_stride(d) * s, "%s pass %d extent", what, p);
    if (q.out >= 0)
      CHECK(q.write_bytes <= P.ws.buf[q.out].bytes, "%s pass %d (kind %d, %lld rows, %lld records) writes %zu > %zu", what, p,
            (int)q.kind, (long long)q.rows, (long long)q.records, q.write_bytes, P.ws.buf[q.out].bytes);
    else
      CHECK(q.write_bytes == 0 && p == P.np - 1, "%s pass %d writes nowhere but is not the last", what, p);
    if (q.kind == DecKind::Level) level_blocks_sum += q.tiles;
    lvl += q.nlev;
    prev_out = q.out;
    prev_records = q.records;
  }
  Layout L;
  make_layout(g_N, L);
  CHECK(lvl == L.nlevels, "%s covers %d of %d levels", what, lvl, L.nlevels);
  CHECK((size_t)(level_blocks_sum + 1) * 16 <= P.ws.partial.bytes, "%s partial sums", what);
}

static void check_decompose(int64_t N, int d, size_t s) {
  static DecPlan P;
  for (int rhs = 0; rhs < 2; ++rhs) {
    plan_decompose(N, d, s, rhs, P);
    check_dec_plan("decompose", P, d, s);
    const DecomposeSolveWs w = decompose_solve_ws(N, d, s);
    for (int p = 0; p < P.np; ++p) {
      const DecPass& q = P.pass[p];
      CHECK((q.kind == DecKind::BulkRhs) <= (rhs && p == 0), "right-hand side in pass %d", p);
      CHECK(cgps::tile_fits_256(d, s) ? q.kind != DecKind::Level : (q.kind == DecKind::Level || q.kind == DecKind::Lds),
            "pass %d: kind %d", p, (int)q.kind);
      if (q.kind != DecKind::BulkRhs) continue;
      // decomp_tile_kernel<.., RHS>: one row of ynext per record, one row of owedy per tile
      CHECK((size_t)q.records * d * s <= w.ynext.bytes, "ynext: %lld rows", (long long)q.records);
      CHECK((size_t)q.tiles * d * s <= w.owedy.bytes, "owedy: %lld rows", (long long)q.tiles);
    }
  }
  const DecomposeSolveWs w = decompose_solve_ws(N, d, s);
  check_regions("decompose_solve_ws", {w.main, w.ynext, w.owedy}, w.total);
  CHECK(decompose_ws(N, d, s).total <= w.main.bytes && sweeps_ws_bytes(N, d, s) <= w.main.bytes, "decompose_solve main region");
}

static void check_inverse(int64_t N, int d, size_t s) {
  static InvPlan P;
  for (int flags = 0; flags < 8; ++flags) {
    const bool fused = flags & 1, fused_ok = flags & 2, deep = flags & 4;
    if (deep && !cgps::deep_block(d, s)) continue;
    plan_inverse(N, d, s, fused, fused_ok, deep, P);
    check_regions("inverse_ws", {P.ws.buf[0], P.ws.buf[1]}, P.ws.total);
    Layout L;
    make_layout(N, L);
    int have = L.nlevels, prev_out = -1;
    for (int p = 0; p < P.np; ++p) {
      const InvPass& q = P.pass[p];
      CHECK(q.first + q.nlev == have, "inverse pass %d: levels [%d, %d), have %d", p, q.first, q.first + q.nlev, have);
      CHECK(q.in == prev_out, "inverse pass %d reads buffer %d, not %d", p, q.in, prev_out);
      CHECK(q.out < 0 || q.out != q.in, "inverse pass %d reads the buffer it writes", p);
      CHECK((q.out < 0) == (q.first == 0), "inverse pass %d output", p);
      if (q.out >= 0) {
        CHECK(q.rows <= P.ws.cap, "inverse pass %d: %lld rows > cap", p, (long long)q.rows);
        CHECK(q.write_bytes <= P.ws.buf[q.out].bytes, "inverse pass %d writes %zu > %zu", p, q.write_bytes, P.ws.buf[q.out].bytes);
      }
      if (q.kind == InvKind::Deep) CHECK(q.nlev <= cgps::INVD_MAXLEV && q.rows <= ((int64_t)1 << cgps::invd_tsl(d, s)), "deep pass");
      have = q.first;
      prev_out = q.out;
    }
    CHECK(have == 0, "inverse stops at level %d", have);
  }
  const LogdetFactorWs lw = logdet_factor_ws();
  int64_t nb = (N * d + 255) / 256;
  if (nb > cgps::LOGDET_MAX_BLOCKS) nb = cgps::LOGDET_MAX_BLOCKS;
  CHECK((size_t)(nb + 1) * 16 <= lw.partial.bytes && lw.partial.end() <= lw.total, "logdet_factor partial sums");
}

// the fused pipeline: stage 1 leaves one record and one partial result per workgroup in recA / partial, every record
// stage one per workgroup in the other record buffer and further partial results behind the ones before
static void check_tile(int64_t N, int d, size_t s) {
  const TileWs w = tile_ws(N, d, s);
  check_regions("tile_ws", {w.partial, w.recA, w.recB}, w.total);
  const TilePairWs pw = tile_pair_ws(N, d, s);
  CHECK(pw.one.total <= pw.stride && pw.total == 2 * pw.stride && pw.stride % 256 == 0, "pair form");
  // rows per stage-1 workgroup: 16 rows x 256 lanes shrink for small systems; every other shape is fixed (longer
  // chunks only make fewer workgroups)
  const int64_t rows1 = cgps::tile_rows1(d, s);
  const int64_t per_tile = rows1 == 16 * 256 ? (int64_t)cgps::stage1_rows_per_lane(N, 16, 256) * 256 : rows1;
  const int64_t tiles = (N + per_tile - 1) / per_tile;
  CHECK(tiles <= w.tiles_cap, "%lld stage-1 workgroups > %lld", (long long)tiles, (long long)w.tiles_cap);
  const size_t rec = (size_t)cgps::record_stride(d) * s;
  CHECK((size_t)tiles * rec <= w.recA.bytes && (size_t)tiles * rec <= w.recB.bytes, "records of stage 1");
  // record stages: at least 64 records per workgroup, so all of them together leave fewer partial results than stage 1
  CHECK((size_t)(2 * tiles + 8) * cgps::PARTIAL_STRIDE * sizeof(double) <= w.partial.bytes, "partial results");
  // the LEG form: one round of at most STAGE1_SMALL_TILES workgroups
  CHECK(cgps::STAGE1_SMALL_TILES <= w.tiles_cap, "LEG form");
}

int main() {
  std::vector<int64_t> ns;
  for (int64_t n = 1; n <= 3000; ++n) ns.push_back(n);
  const int64_t centres[] = {32768, 65408, 131072, 262144, 1 << 20};
  for (int64_t c : centres)
    for (int64_t n = c - 1; n <= c + 1; ++n) ns.push_back(n);
  ns.push_back((1 << 21) + 3);
  ns.push_back((1 << 24) + 5);
  const size_t sizes[] = {4, 8};
  for (int64_t N : ns)
    for (int d = 1; d <= 8; ++d)
      for (size_t s : sizes) {
        g_N = N; g_d = d; g_s = s;
        check_levelwise(N, d, s);
        check_sweeps(N, d, s);
        check_decompose(N, d, s);
        check_inverse(N, d, s);
        check_tile(N, d, s);
      }
  printf("%ld checks, %ld failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
