// The first levels of a FULL tile's cyclic reduction in the registers of the lanes that streamed its rows
// (4 x 4 fp64 blocks, rows straight from memory).  Included from cgps_tile.h (inside namespace cgps) right
// before chunk_reduce_kernel; the map at the top is host-pure (tests/wave_levels_layout_check.cpp includes this
// header alone).
//
// After the streaming loop lane t holds the kept row of its chunk (Rc, yc), that row's coupling Cc to the kept
// row of lane t - 1, and (dRa, dya): what the chunk's eliminations owe that row, as negative sums.  Level l of
// tile_cr (stride s = 2^l) eliminates the rows e with e mod 2s == s - 1 between e - s and o = e + s.  For lane
// o that is one more step of the streaming loop: the "current" row is row e with what lane o owes it added,
// its coupling to the left boundary is Cc_e, the boundary's accumulators are those of lane e, the coupling to
// the "next" row is Cc_o and the next row is lane o's own.  eliminate_forward does the rest, unchanged, and lane
// o ends up with the surviving row, its coupling to row e - s and everything owed to that row.  The operands
// of lane e reach lane o by DPP row shifts (s <= 8: inside a 16-lane row).  No LDS, no barrier.
//
// After L levels the survivors sit in the lanes (m + 1) 2^L - 1 and hand tile_cr the LDS state it expects at
// level L: row and right-hand side at the lane's own slot, the coupling to the left survivor where that level
// reads it, and what the lane owes its left survivor PARKED half a stride to the left, in the form the levels
// read (the sum of G G^T and G x, symmetric).  The first survivor owes the row left of the tile: its share goes
// to the exchange words, as thread 0's does on the staged path.
#pragma once

#ifndef CGPS_WAVE_LEVELS
// Each level is one lane's whole elimination, a dependent chain of ~350 fp64 instructions on one wave per SIMD:
// 1.2 - 1.9 us whatever the number of lanes that still work.  Levels 0 and 1 (128 and 64 eliminations) cost the
// same in the LDS form, and doing them here saves the staging of 256 rows and its barrier; from level 2 on the LDS
// form (quads, then the matrix cores) is faster per level.  Measured at 2^20 rows: 1 / 2 / 3 levels give
// about -0.8 / -1.2 / 0.0 us against none.
#define CGPS_WAVE_LEVELS 2        // levels done in registers (0 .. 4); 0 builds the staged path only
#endif

namespace wave_levels {
constexpr int MAX_LEVELS = 4;                                      // a DPP row shift reaches 8 lanes
// lane o eliminates at level l: it is the right neighbour of a row that level removes
constexpr bool pulls(int lane, int l) { return (lane & ((2 << l) - 1)) == (2 << l) - 1; }
// ... the row of this lane
constexpr int pull_source(int lane, int l) { return lane - (1 << l); }
// slot of the m-th row that is left after L levels (= the lane that holds it)
constexpr int surviving_slot(int m, int L) { return (m + 1) * (1 << L) - 1; }
constexpr bool survives(int lane, int L) { return (lane & ((1 << L) - 1)) == (1 << L) - 1; }
// where survivor o leaves what it owes the survivor on its left (L >= 1); -1: the row left of the tile
constexpr int parking_slot(int o, int L) { return o < (2 << (L - 1)) ? -1 : o - (1 << (L - 1)); }
// index into Oc of survivor o's coupling to the survivor on its left (Oc[0]: to the row left of the tile)
constexpr int coupling_slot(int o, int L) { return o - (1 << L) + 1; }
}  // namespace wave_levels

#ifdef __HIPCC__
// lane i of every 16-lane row takes the value of lane i - S of that row (lanes i < S: unspecified)
template <int S>
__device__ __forceinline__ double row_shr_f64(double v) {
  static_assert(S >= 1 && S <= 15, "row_shr:1..15");
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), 0x110 + S, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), 0x110 + S, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}

// One level.  Every lane of the wave takes part in the shifts (a DPP read of a lane that is masked off
// returns nothing); the lanes that pull eliminate.
template <int LV>
__device__ __forceinline__ void wave_level(int lane, double (&Rc)[4][4], double (&yc)[4], double (&Cc)[4][4],
                                           double (&dRa)[4][4], double (&dya)[4], PivotLog& pl, double& mah, bool& fail) {
  constexpr int D = 4, S = 1 << LV;
  static_assert(wave_levels::pull_source(15, LV) >= 0, "the source is in the same 16-lane row");
  double eR[D][D], ey[D], eC[D][D], edR[D][D], edy[D];
#pragma unroll
  for (int i = 0; i < D; ++i) {
#pragma unroll
    for (int j = 0; j < D; ++j) {
      eC[i][j] = row_shr_f64<S>(Cc[i][j]);
      if (j <= i) {
        eR[i][j] = row_shr_f64<S>(Rc[i][j]);
        edR[i][j] = row_shr_f64<S>(dRa[i][j]);
      } else {
        eR[i][j] = 0.0;
        edR[i][j] = 0.0;
      }
    }
    ey[i] = row_shr_f64<S>(yc[i]);
    edy[i] = row_shr_f64<S>(dya[i]);
  }
  if (wave_levels::pulls(lane, LV)) {
#pragma unroll
    for (int i = 0; i < D; ++i) {
      ey[i] += dya[i];                         // what this lane owes the row it eliminates
#pragma unroll
      for (int j = 0; j <= i; ++j) eR[i][j] += dRa[i][j];
    }
    // (the lane's own row is the "next" row: updated in place)
    eliminate_forward<double, D>(eR, ey, eC, edR, edy, Cc, Rc, yc, pl, mah, fail);
#pragma unroll
    for (int i = 0; i < D; ++i) {
      dya[i] = edy[i];
#pragma unroll
      for (int j = 0; j < D; ++j) {
        Cc[i][j] = eC[i][j];
        if (j <= i) dRa[i][j] = edR[i][j];
      }
    }
  }
}

// Levels 0 .. L-1 of a full tile of NT lanes, then the hand-over to tile_cr (see the head of the file).
// tid: threadIdx.x as an opaque value (see tile_cr).  Threads past the NT lanes hold nothing and do nothing.
// The slots of t.R a wave writes are the right-hand-side lines of its own lanes (chunk_reduce_kernel), which
// that wave has finished reading; the barrier that opens tile_cr makes the stores visible.
template <int L, int NT>
__device__ __forceinline__ void wave_levels_and_hand_over(LdsTile<double, 4>& t, int tid, double (&Rc)[4][4], double (&yc)[4],
                                                          double (&Cc)[4][4], double (&dRa)[4][4], double (&dya)[4],
                                                          double* xch, PivotLog& pl, double& mah, bool& fail) {
  static_assert(L >= 1 && L <= wave_levels::MAX_LEVELS && NT % 64 == 0, "row shifts of 1, 2, 4 and 8 lanes");
  constexpr int D = 4;
  using LT = LdsTile<double, D>;
  if (tid >= NT) return;                       // (wave-uniform)
  wave_level<0>(tid, Rc, yc, Cc, dRa, dya, pl, mah, fail);
  if constexpr (L >= 2) wave_level<1>(tid, Rc, yc, Cc, dRa, dya, pl, mah, fail);
  if constexpr (L >= 3) wave_level<2>(tid, Rc, yc, Cc, dRa, dya, pl, mah, fail);
  if constexpr (L >= 4) wave_level<3>(tid, Rc, yc, Cc, dRa, dya, pl, mah, fail);
  if (wave_levels::survives(tid, L)) {
    mirror_lower<double, D>(Rc);
    LT::store_blk(t.R, tid, Rc);
    store_vec<double, D>(t.y + tid * D, yc);
    LT::store_blk(t.Oc, wave_levels::coupling_slot(tid, L), Cc);
    if (tid == wave_levels::surviving_slot(0, L)) {
#pragma unroll
      for (int i = 0; i < D; ++i) {
#pragma unroll
        for (int j = 0; j <= i; ++j) xch[i * D + j] = dRa[i][j];
        xch[D * D + i] = dya[i];
      }
    } else {
      const int park = tid - (1 << (L - 1));   // wave_levels::parking_slot
      double P[D][D], p[D];
#pragma unroll
      for (int i = 0; i < D; ++i) {
        p[i] = -dya[i];
#pragma unroll
        for (int j = 0; j <= i; ++j) P[i][j] = -dRa[i][j];
      }
      mirror_lower<double, D>(P);
      LT::store_blk(t.R, park, P);
      store_vec<double, D>(t.y + park * D, p);
    }
  }
}
#endif  // __HIPCC__
