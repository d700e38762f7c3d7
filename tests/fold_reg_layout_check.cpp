// Host-only check of the layout helpers of csrc/cgps_tile_rec.h (compiled and run by
// tests/test_fold_register_stages.py with a plain C++17 compiler: the helpers need nothing from HIP).
// For every n = 1..16 records the register-resident record stage is walked level by level next to the
// (e, o, act) rule of the LDS path (tile_cr in cgps_tile.h):
//   * each level eliminates exactly the rows the LDS path eliminates, between the same neighbours;
//   * the last real row is never eliminated, every other row exactly once;
//   * the route an update takes (row rotation and register-set step) ends at the neighbour's owner;
//   * every element has exactly one owner (register set, lane).
// Prints every failing case; exit status 1 if there is one.
#include <cstdio>
#include <set>
#include <vector>

#include "cgps_tile_rec.h"

using namespace fold_reg;

static long g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                        \
  do {                                          \
    ++g_checks;                                 \
    if (!(cond)) {                              \
      if (++g_failed <= 50) {                   \
        printf("FAIL %s: ", #cond);             \
        printf(__VA_ARGS__);                    \
        printf("\n");                           \
      }                                         \
    }                                           \
  } while (0)

// where the element in (register set u, lane) ends up when the level hands it to the right (dir = +1) or left
// (dir = -1) neighbour: the register set and the row rotation cgps_tile_rec.h uses (row_ror: lane i of a 16-lane
// row takes the value of lane (i - rot) mod 16)
static void route(int l, int dir, int u, int lane, int* u_out, int* lane_out) {
  const int row = lane & ~15, in_row = lane & 15;
  const int rot = dir > 0 ? right_rot(l, u) : left_rot(l, u);
  *lane_out = row + ((in_row + rot) & 15);
  *u_out = dir > 0 ? right_set(l, u) : left_set(l, u);
}

int main() {
  // ownership: (position, r, c) <-> (register set, lane) is one to one
  std::set<std::pair<int, int>> owners;
  for (int p = 0; p < MAX_RECORDS; ++p)
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) {
        const int u = reg_set(p), lane = owner_lane(p, r, c);
        CHECK(u >= 0 && u < 4 && lane >= 0 && lane < 64, "p=%d r=%d c=%d -> set %d lane %d", p, r, c, u, lane);
        CHECK(position(u, (lane >> 2) & 3) == p && (lane >> 4) == r && (lane & 3) == c, "p=%d r=%d c=%d does not map back", p, r, c);
        CHECK(owners.insert({u, lane}).second, "p=%d r=%d c=%d: (set %d, lane %d) owned twice", p, r, c, u, lane);
      }
  CHECK(owners.size() == 4 * 64, "%zu owners", owners.size());

  for (int n = 1; n <= MAX_RECORDS; ++n) {
    const int K = n - 1;
    std::vector<int> gone(n, 0);
    int lds_levels = 0;
    for (int s = 1, l = 0; (s - 1) < K; s <<= 1, ++l, ++lds_levels) {
      // the LDS path's rule (tile_cr)
      const int M = (K + 1) / s;
      std::set<int> lds_e;
      for (int k = 0; k < (M + 1) / 2; ++k) {
        const int e = (2 * k + 1) * s - 1;
        const bool act = (2 * k < M) && (e != K);
        if (!act) continue;
        const int o = (2 * k + 1 < M) ? e + s : K;
        const int left = (k == 0) ? -1 : e - s;
        lds_e.insert(e);
        CHECK(e < MAX_RECORDS - 1 && eliminated(e, l, n), "n=%d level %d: row %d is not eliminated in registers", n, l, e);
        CHECK((right_is_tail(e, l, n) ? K : right_source(e, l)) == o, "n=%d level %d row %d: right neighbour %d", n, l, e, o);
        CHECK((left_is_outside(e, l) ? -1 : left_source(e, l)) == left, "n=%d level %d row %d: left neighbour %d", n, l, e, left);
        if (!right_is_tail(e, l, n)) CHECK(survivor(o, l) && !eliminated(o, l, n), "n=%d level %d: neighbour %d does not take", n, l, o);
        if (left >= 0) CHECK(survivor(left, l) && !eliminated(left, l, n), "n=%d level %d: neighbour %d does not take", n, l, left);
        // the chains of the level cover the row's register set
        bool carried = false;
        for (int j = 0; j < chains(l); ++j) carried = carried || chain_set(l, j) == reg_set(e);
        CHECK(carried, "n=%d level %d: register set %d of row %d is not carried", n, l, reg_set(e), e);
        // the updates reach the neighbours' owners, element by element
        for (int r = 0; r < 4; ++r)
          for (int c = 0; c < 4; ++c) {
            int u2, lane2;
            if (!right_is_tail(e, l, n)) {
              route(l, +1, reg_set(e), owner_lane(e, r, c), &u2, &lane2);
              CHECK(u2 == reg_set(o) && lane2 == owner_lane(o, r, c), "n=%d level %d: row %d -> %d arrives at set %d lane %d", n, l, e, o, u2, lane2);
            }
            if (left >= 0) {
              route(l, -1, reg_set(e), owner_lane(e, r, c), &u2, &lane2);
              CHECK(u2 == reg_set(left) && lane2 == owner_lane(left, r, c), "n=%d level %d: row %d -> %d arrives at set %d lane %d", n, l, e, left, u2, lane2);
            }
          }
        ++gone[e];
      }
      // ... and nothing else
      int last = -1;
      for (int p = 0; p < MAX_RECORDS; ++p)
        if (eliminated(p, l, n)) {
          CHECK(lds_e.count(p) == 1, "n=%d level %d: position %d is eliminated in registers only", n, l, p);
          CHECK(p != K, "n=%d level %d: the last real row is eliminated", n, l);
          last = p;
        }
      CHECK(last == last_eliminated(l, n), "n=%d level %d: last eliminated %d, helper says %d", n, l, last, last_eliminated(l, n));
      int tails = 0;
      for (int p = 0; p < MAX_RECORDS; ++p) tails += eliminated(p, l, n) && right_is_tail(p, l, n);
      CHECK(tails <= 1 && (tails == 0 || right_is_tail(last, l, n)), "n=%d level %d: %d rows update the tail", n, l, tails);
    }
    CHECK(lds_levels == levels(n), "n=%d: %d levels, helper says %d", n, lds_levels, levels(n));
    for (int l = levels(n); l < 4; ++l)
      for (int p = 0; p < MAX_RECORDS; ++p) CHECK(!eliminated(p, l, n) || l < levels(n), "n=%d: level %d would still eliminate %d", n, l, p);
    for (int p = 0; p < K; ++p) CHECK(gone[p] == 1, "n=%d: row %d eliminated %d times", n, p, gone[p]);
    CHECK(K < 0 || gone[K] == 0, "n=%d: the last real row is eliminated", n);
  }
  printf("fold_reg_layout_check: %ld checks, %ld failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
