// The workspace of cgps_leg_filter_scan (filter_scan_ws in csrc/cgps_plan.h), checked on the host: built by a plain
// C++17 compiler from the header alone (tests/test_leg_filter_scan.py).  Arguments: groups of five numbers, chunks M d
// scalar-size fanout.  One line per group: the five numbers, the plan's total, the sum of its regions, its levels, and 1
// when the regions follow each other without gap or overlap from offset 0, each 256-byte aligned and large enough for
// what its phase stores there, and the levels shrink by the fan-out down to one group.
#include <cstdio>
#include <cstdlib>

#include "cgps_plan.h"

int main(int argc, char** argv) {
  using namespace cgps_host;
  for (int i = 1; i + 4 < argc; i += 5) {
    const long long chunks = atoll(argv[i]), M = atoll(argv[i + 1]), F = atoll(argv[i + 4]);
    const int d = atoi(argv[i + 2]);
    const size_t s = (size_t)atoll(argv[i + 3]);
    const FilterScanWs w = filter_scan_ws(chunks, M, d, s, F);
    size_t sum = 0, end = 0;
    bool ok = w.levels >= 1 && w.n[0] == chunks;
    auto take = [&](const Region& r, size_t need) {
      ok = ok && r.off == end && r.bytes >= need && r.off % 256 == 0;
      end = r.end();
      sum += r.bytes;
    };
    for (int l = 0; l < w.levels; ++l) {
      take(w.elem[l], (size_t)M * filter_scan_elem_scalars(d) * (size_t)w.n[l] * s);
      if (l + 1 < w.levels) ok = ok && w.n[l] > F && w.n[l + 1] == (w.n[l] + F - 1) / F;
    }
    ok = ok && w.n[w.levels - 1] <= F;
    take(w.t0, (size_t)chunks * s);
    take(w.m0, (size_t)M * chunks * d * s);
    take(w.P0, (size_t)M * chunks * d * d * s);
    take(w.loglik, (size_t)M * chunks * sizeof(double));
    take(w.m_end, (size_t)M * chunks * d * s);
    take(w.P_end, (size_t)M * chunks * d * d * s);
    ok = ok && end == w.total;
    printf("%lld %lld %d %zu %lld %zu %zu %d %d\n", chunks, M, d, s, F, w.total, sum, w.levels, ok ? 1 : 0);
  }
  return 0;
}
