// Which pass kinds does a case take?  Host-only: includes cgps_plan.h alone and is built like plan_check.cpp (a plain
// C++17 host compiler, tests/test_memory_contract.py).  The memory-contract tests choose their shapes from what this
// prints, not from guesses: a kernel family that no case runs is a family whose writes nobody has looked at.
//
//   plan_cases [--cus C] N,d,s,nrhs ...     one line per case:  "case N d s nrhs | kind kind ..."
//   plan_cases [--cus C] --extents N,d,s,nrhs ...   per case and operation, where the plan says the passes write inside
//                                           the workspace:  "extent N d s OP offset bytes" (OP: halfsolve, backsolve,
//                                           decompose, inverse; one column).  Everything else in the workspace is
//                                           nobody's: the device test finds it still poisoned after the call.
//   plan_cases [--cus C] --reachable        one line per scalar size:  "reachable s | kind kind ..." -- every kind some
//                                           (N, d, nrhs) of that precision takes, over N = 1 .. 4100 and the thresholds
//                                           the plans branch on with their neighbours
//
// Kinds, as cgps_plan.h defines them and as the run_* functions of the library ask for them:
//   dec:Level / dec:Bulk / dec:BulkRhs / dec:Lds   DecKind of plan_decompose, without and with the right-hand side
//   inv:Deep / inv:Tile / inv:Level                InvKind of plan_inverse, flags as run_inverse sets them
//   sweep:regular / sweep:deep                     passes of plan_sweep (one column), deep_tiles = C where deep_block()
//   top:fused / top:plain                          solve(): the last pass is one deep tile (solve_top_kernel) or not
//   panel:2 / panel:4 / panel:8                    panel_width(nrhs), nrhs > 1
//   psweep:regular / psweep:deep                   passes of plan_panel_sweep
//   chunk:1 / chunk:4 / chunk:8 / chunk:16         stage1_rows_per_lane of the 16 x 256 stage-1 tile; chunk:fixed for the
//                                                  block sizes whose stage-1 tile has one shape (d = 8, fp64 d = 6, 7)
//   mahal:fused / mahal:levelwise                  the two entry points; every (N, d, s) has both
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "cgps_plan.h"

using namespace cgps_host;
typedef std::set<std::string> Kinds;

static void kinds_of(int64_t N, int d, size_t s, int nrhs, int cus, Kinds& k) {
  Layout L;
  make_layout(N, L);
  static DecPlan D;
  for (int rhs = 0; rhs < 2; ++rhs) {
    plan_decompose(N, d, s, rhs != 0, D);
    for (int p = 0; p < D.np; ++p) {
      const DecKind q = D.pass[p].kind;
      k.insert(q == DecKind::Level ? "dec:Level" : q == DecKind::Bulk ? "dec:Bulk" : q == DecKind::BulkRhs ? "dec:BulkRhs" : "dec:Lds");
    }
  }
  {
    const bool in_quad = d == 8, fused = (size_t)d * d * s <= 400 || in_quad;
    static InvPlan I;
    plan_inverse(N, d, s, fused, true, cgps::deep_block(d, s), I);
    for (int p = 0; p < I.np; ++p) {
      const InvKind q = I.pass[p].kind;
      k.insert(q == InvKind::Deep ? "inv:Deep" : q == InvKind::Tile ? "inv:Tile" : "inv:Level");
    }
  }
  if (nrhs == 1) {
    SolvePasses P;
    plan_sweep(L, P, cgps::deep_block(d, s) ? cus : 0);
    for (int p = 0; p < P.np; ++p) k.insert(P.deep[p] ? "sweep:deep" : "sweep:regular");
    const int p = P.np - 1;
    k.insert(P.tiles[p] == 1 && P.deep[p] ? "top:fused" : "top:plain");
  } else {
    const int mc = cgps::panel_width(nrhs);
    k.insert("panel:" + std::to_string(mc));
    SolvePasses P;
    plan_panel_sweep(L, P, mc, cgps::deep_block(d, s), true);
    for (int p = 0; p < P.np; ++p) k.insert(P.deep[p] ? "psweep:deep" : "psweep:regular");
  }
  // (TileCfg in cgps_tile.h: 8 x 8 blocks and the blocks whose 256-row tile does not fit the LDS take their full chunk)
  if (d != 8 && cgps::tile_fits_256(d, s)) k.insert("chunk:" + std::to_string(cgps::stage1_rows_per_lane(N, 16, 256)));
  else k.insert("chunk:fixed");
  k.insert("mahal:fused");
  k.insert("mahal:levelwise");
}

// The host's model of what the kernels store into the workspace (forward_write_bytes, backward_write_bytes, the
// write_bytes of DecPass / InvPass, one pair of doubles per workgroup that leaves a partial sum).
static void extents_of(int64_t N, int d, size_t s, int cus) {
  char head[64];
  snprintf(head, sizeof(head), "extent %lld %d %zu", (long long)N, d, s);
  Layout L;
  make_layout(N, L);
  SolvePasses P;
  plan_sweep(L, P, cgps::deep_block(d, s) ? cus : 0);
  const LevelWs h = halfsolve_ws(N, d, s);
  const BacksolveWs b = backsolve_ws(N, d, s);
  int64_t tiles = 0;
  for (int p = 0; p < P.np; ++p) {
    tiles += P.tiles[p];
    printf("%s halfsolve %zu %zu\n", head, h.buf[P.buf(p)].off, P.forward_write_bytes(p, (size_t)d * s));
    printf("%s backsolve %zu %zu\n", head, b.x_of(p).off, P.backward_write_bytes(p, (size_t)d * s));
  }
  printf("%s halfsolve %zu %zu\n", head, h.partial.off, (size_t)tiles * 16);
  static DecPlan D;
  plan_decompose(N, d, s, false, D);
  int64_t blocks = 0;
  for (int p = 0; p < D.np; ++p) {
    const DecPass& q = D.pass[p];
    if (q.kind == DecKind::Level) blocks += q.tiles;
    if (q.out >= 0) printf("%s decompose %zu %zu\n", head, D.ws.buf[q.out].off, q.write_bytes);
  }
  printf("%s decompose %zu %zu\n", head, D.ws.partial.off, (size_t)blocks * 16);
  const bool in_quad = d == 8, fused = (size_t)d * d * s <= 400 || in_quad;
  static InvPlan I;
  plan_inverse(N, d, s, fused, true, cgps::deep_block(d, s), I);
  for (int p = 0; p < I.np; ++p)
    if (I.pass[p].out >= 0) printf("%s inverse %zu %zu\n", head, I.ws.buf[I.pass[p].out].off, I.pass[p].write_bytes);
}

static void print(const char* head, const Kinds& k) {
  printf("%s |", head);
  for (const std::string& t : k) printf(" %s", t.c_str());
  printf("\n");
}

int main(int argc, char** argv) {
  int cus = 256;
  bool reachable = false, extents = false;
  std::vector<const char*> cases;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--cus") && i + 1 < argc) cus = atoi(argv[++i]);
    else if (!strcmp(argv[i], "--reachable")) reachable = true;
    else if (!strcmp(argv[i], "--extents")) extents = true;
    else cases.push_back(argv[i]);
  }
  for (const char* c : cases) {
    long long N;
    int d, s, nrhs;
    if (sscanf(c, "%lld,%d,%d,%d", &N, &d, &s, &nrhs) != 4 || N < 1 || d < 1 || d > 8 || (s != 4 && s != 8) || nrhs < 1) {
      fprintf(stderr, "bad case %s (want N,d,s,nrhs)\n", c);
      return 2;
    }
    if (extents) {
      extents_of(N, d, (size_t)s, cus);
      continue;
    }
    Kinds k;
    kinds_of(N, d, (size_t)s, nrhs, cus, k);
    char head[96];
    snprintf(head, sizeof(head), "case %lld %d %d %d", N, d, s, nrhs);
    print(head, k);
  }
  if (reachable) {
    std::vector<int64_t> ns;
    for (int64_t n = 1; n <= 4100; ++n) ns.push_back(n);
    const int64_t centres[] = {32768, 65408, 131072, 262144, 524288, 1 << 20};
    for (int64_t c : centres)
      for (int64_t n = c - 1; n <= c + 1; ++n) ns.push_back(n);
    const int widths[] = {1, 2, 3, 9};
    for (int s = 4; s <= 8; s += 4) {
      Kinds k;
      for (int64_t N : ns)
        for (int d = 1; d <= 8; ++d)
          for (int nrhs : widths) kinds_of(N, d, (size_t)s, nrhs, cus, k);
      char head[32];
      snprintf(head, sizeof(head), "reachable %d", s);
      print(head, k);
    }
  }
  return 0;
}
