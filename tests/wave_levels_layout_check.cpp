// Host-only check of the lane map of csrc/cgps_tile_wave.h (compiled and run by tests/test_wave_levels.py with a
// plain C++17 compiler: the map needs nothing from HIP).
// For full tiles of 64, 128 and 256 rows and every L = 1..4 the in-register levels are walked next to the
// (e, o, act) rule and the parking rule of the LDS path (tile_cr in cgps_tile.h):
//   * at level l < L exactly the lanes o that the LDS path names as right neighbours pull, from the row e it
//     eliminates, which still exists and sits in the same 16-lane row;
//   * after L levels the rows left are the slots surviving_slot(m, L), the rows of level L of the LDS path;
//   * a survivor's coupling goes where level L - 1 of the LDS path writes it and level L reads it;
//   * what a survivor owes its left neighbour is parked where level L - 1 parks it and level L looks for it;
//     the first survivor owes the row left of the tile (no parking slot).
// Prints every failing case; exit status 1 if there is one.
#include <cstdio>
#include <set>
#include <vector>

#include "cgps_tile_wave.h"

using namespace wave_levels;

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

int main() {
  static_assert(CGPS_WAVE_LEVELS >= 0 && CGPS_WAVE_LEVELS <= MAX_LEVELS, "the compiled number of levels");
  for (int NT : {64, 128, 256})
    for (int L = 1; L <= MAX_LEVELS; ++L) {
      const int K = NT - 1;
      std::vector<int> alive(NT, 1);
      // for each right neighbour of the last walked level: the slot its elimination parked in, the row that is
      // owed, and the index of the coupling it wrote
      std::vector<int> parked_at(NT, -2), owed_row(NT, -2), coupling_at(NT, -2);
      for (int l = 0, s = 1; l < L; ++l, s <<= 1) {
        CHECK((s - 1) < K, "NT=%d: level %d does not run in the LDS path", NT, l);
        const int M = (K + 1) / s;
        std::set<int> lds_o;
        for (int k = 0; k < (M + 1) / 2; ++k) {
          const int e = (2 * k + 1) * s - 1;
          const bool act = (2 * k < M) && (e != K);
          if (!act) continue;
          const int o = (2 * k + 1 < M) ? e + s : K;
          const int left = (k == 0) ? -1 : e - s;
          lds_o.insert(o);
          CHECK(pulls(o, l), "NT=%d level %d: lane %d does not pull", NT, l, o);
          CHECK(pull_source(o, l) == e, "NT=%d level %d: lane %d pulls from %d, the LDS path eliminates %d", NT, l, o, pull_source(o, l), e);
          CHECK(!pulls(e, l), "NT=%d level %d: the eliminated lane %d pulls as well", NT, l, e);
          CHECK(alive[e] && alive[o], "NT=%d level %d: row %d or %d is gone already", NT, l, e, o);
          CHECK((e >> 4) == (o >> 4) && (o & 15) - (e & 15) == s, "NT=%d level %d: %d -> %d is no row shift by %d", NT, l, e, o, s);
          CHECK(left < 0 || (alive[left] && pulls(left, l)), "NT=%d level %d: the left neighbour %d of %d does not survive", NT, l, left, e);
          alive[e] = 0;
          parked_at[o] = e;                     // tile_cr parks what row `left` is owed in the dead slot e
          owed_row[o] = left;
          coupling_at[o] = e - s + 1;           // ... and writes J[o, left] there
        }
        for (int lane = 0; lane < NT; ++lane)
          if (pulls(lane, l)) CHECK(lds_o.count(lane) == 1, "NT=%d level %d: lane %d pulls, but is no right neighbour", NT, l, lane);
      }
      // the rows left
      const int S = 1 << L, h = S >> 1;
      int m = 0;
      for (int slot = 0; slot < NT; ++slot) {
        CHECK(survives(slot, L) == (alive[slot] != 0), "NT=%d L=%d: slot %d", NT, L, slot);
        if (!alive[slot]) continue;
        CHECK(surviving_slot(m, L) == slot, "NT=%d L=%d: survivor %d at %d, the map says %d", NT, L, m, slot, surviving_slot(m, L));
        ++m;
        // level L of the LDS path reads the coupling of this row to its left neighbour at Oc[slot - S + 1] ...
        CHECK(coupling_slot(slot, L) == slot - S + 1 && coupling_slot(slot, L) == coupling_at[slot], "NT=%d L=%d slot %d: coupling at %d, level %d wrote %d",
              NT, L, slot, coupling_slot(slot, L), L - 1, coupling_at[slot]);
        CHECK(coupling_slot(slot, L) >= 0 && coupling_slot(slot, L) <= NT, "NT=%d L=%d slot %d: coupling index", NT, L, slot);
        // ... and what is pending for row r at r + h (pend_e / the right neighbour's pending in tile_cr)
        const int left = owed_row[slot];
        if (left < 0) {
          CHECK(parking_slot(slot, L) == -1 && slot == surviving_slot(0, L), "NT=%d L=%d slot %d owes the row left of the tile", NT, L, slot);
        } else {
          CHECK(parking_slot(slot, L) == parked_at[slot] && parking_slot(slot, L) == left + h, "NT=%d L=%d slot %d: parks at %d, level %d parked at %d, level %d reads %d",
                NT, L, slot, parking_slot(slot, L), L - 1, parked_at[slot], L, left + h);
          CHECK(!alive[parking_slot(slot, L)] && left + h < K, "NT=%d L=%d slot %d: parking slot %d", NT, L, slot, parking_slot(slot, L));
          CHECK((parking_slot(slot, L) >> 6) == (slot >> 6), "NT=%d L=%d slot %d parks in another wave's slots", NT, L, slot);
        }
      }
      CHECK(m == NT / S && alive[K], "NT=%d L=%d: %d rows left", NT, L, m);
    }
  printf("wave_levels_layout_check: %ld checks, %ld failed\n", g_checks, g_failed);
  return g_failed ? 1 : 0;
}
