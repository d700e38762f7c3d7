// Includes csrc/cgps_plan.h alone (host-pure): for every size, block size, scalar size and sample count, what each
// backward pass of cgps_sample writes into a chunk's slice of the coarse-solution buffers fits the slice, the pass
// after it reads no more rows than were written, and the slices of all chunks of a launch lie inside the workspace.
#include <cstdio>
#include <vector>

#include "cgps_plan.h"

using namespace cgps_host;

int main() {
  long checks = 0, failed = 0;
  auto fail = [&](const char* what, int64_t N, int d, size_t s, int64_t m) {
    if (failed++ < 20) std::printf("FAIL %s: N=%lld d=%d s=%zu nrhs=%lld\n", what, (long long)N, d, s, (long long)m);
  };
  std::vector<int64_t> Ns;
  for (int64_t n = 1; n <= 3000; ++n) Ns.push_back(n);
  for (int64_t n : {4095, 4096, 4097, 65535, 65536, 65537, 70001, (1 << 20) - 1, 1 << 20, (1 << 20) + 1, (1 << 23) + 5, (1 << 24) + 5})
    Ns.push_back(n);
  for (int64_t N : Ns)
    for (int d = 1; d <= 8; ++d)
      for (size_t s : {(size_t)4, (size_t)8})
        for (int64_t m : {1, 2, 3, 4, 5, 8, 9, 40, 1000, 1024, 1025, 5000}) {
          if (N > 3000 && d != 1 && d != 4 && d != 8) continue;
          const SampleWs w = sample_ws(N, d, s, m);
          Layout L;
          make_layout(N, L);
          SolvePasses P;
          plan_panel_sweep(L, P, w.mc, false, false);
          ++checks;
          if (w.mc != cgps::panel_width(m > 8 ? 8 : (int)m) || w.chunks * w.mc < m || (w.chunks - 1) * w.mc >= m) fail("chunks", N, d, s, m);
          if (w.group < 1 || w.group > SAMPLE_CHUNK_GROUP || w.group > w.chunks) fail("group", N, d, s, m);
          if (w.buf[0].off != 0 || w.buf[1].off != w.buf[0].end() || w.buf[1].end() > w.total) fail("regions", N, d, s, m);
          for (int b = 0; b < 2; ++b)
            if (w.slice[b] % 256 != 0 || w.slice[b] * (size_t)w.group != w.buf[b].bytes) fail("slices", N, d, s, m);
          if (P.rows[0] != N || P.np < 1 || P.np > SOLVE_MAX_PASSES) fail("passes", N, d, s, m);
          for (int p = 0; p < P.np; ++p) {
            if (P.deep[p] || P.ts[p] != (1 << cgps::solve_m_tile_log2(w.mc))) fail("one kernel form", N, d, s, m);
            if (P.lv[p].nlev < 1 || P.lv[p].nlev > cgps::SOLVE_MAXLEV) fail("levels", N, d, s, m);
            if (P.tiles[p] != (P.rows[p] + P.ts[p] - 1) / P.ts[p]) fail("tiles", N, d, s, m);
            // pass p > 0 writes rows[p] rows of d * mc scalars into its slice; pass p - 1 reads rows[p - 1] >> nlev of them
            if (p > 0 && (size_t)P.rows[p] * d * w.mc * s > w.slice[p & 1]) fail("write outside slice", N, d, s, m);
            if (p + 1 < P.np && (P.rows[p] >> P.lv[p].nlev) != P.rows[p + 1]) fail("reads what was written", N, d, s, m);
            if (p + 1 == P.np && (P.rows[p] >> P.lv[p].nlev) != 0) fail("top pass ends the sweep", N, d, s, m);
          }
        }
  std::printf("%ld checks, %ld failed\n", checks, failed);
  return failed ? 1 : 0;
}
