// A record stage of the fused solve + log-det in ONE wave's registers (4 x 4 fp64 blocks).
// Included from cgps_tile.h (inside namespace cgps) right before fold_record_stages; the layout
// helpers at the top are host-pure (tests/fold_reg_layout_check.cpp includes this header alone).
//
// A stage takes n <= 16 records in and leaves one record (or the two scalars).  The LDS form
// (record_reduce_body) copies the records into the swizzled tile and runs up to four
// tile_cr_level_mfma passes, a workgroup barrier each, with one block element per lane already.
// Sixteen 4 x 4 blocks are sixteen doubles per element lane, so one wave holds the whole stage:
//
//   * rows 0 .. n-2 sit at POSITIONS p = 4 b + (p mod 4): the register set is u = SET_OF[p mod 4] with
//     SET_OF = {0, 2, 1, 3}, and element [r][c] of position p sits in lane 16 r + 4 b + c of set u (the
//     standard layout of cgps_tile_mfma.h: four blocks per MFMA).  So sets 0, 1 hold the EVEN
//     positions (4b, 4b + 2), set 2 the positions 4b + 1 and set 3 the positions 4b + 3: every level
//     finds its eliminations packed in whole register sets -- level 0 in sets 0 and 1, level 1 in set
//     2, levels 2 and 3 in set 3 -- five chains of arithmetic in all.  (With p = 4u + b, the layout
//     first tried, a level's eliminations are spread over all four sets, eleven chains in all: one
//     wave issues one chain's ~200 instructions in ~0.4 us whether its lanes are busy or not, and the
//     stage was SLOWER than the LDS form, 7.3 against 5.6 us for 16 records.)
//   * the last row K = n - 1 is never eliminated (it is the boundary the next group couples to) and
//     is the right neighbour of whichever elimination comes last in a level, at no fixed distance:
//     it lives in a TAIL register of its own, replicated over the four b;
//   * level l (stride s = 2^l) eliminates the positions p < K with (p + 1) mod 2s == s -- the rows
//     the (e, o, act) rule of tile_cr eliminates -- and hands F F^T, F x, the new coupling to position
//     p + s and G G^T, G x, the transposed new coupling to p - s.  A neighbour is either the same
//     lanes of another register set or one b away (a DPP row rotation by 4 lanes): right_set /
//     right_rot / left_set / left_rot below.  p + s >= K: the right neighbour is the tail, which takes
//     the sum over all positions of what is owed to it (one term is non-zero) by two row rotations.
//     p < s: the left neighbour is the row left of the group; what it is owed accumulates and
//     becomes the output record's dRa / dya;
//   * a position holds its couplings to BOTH active neighbours (left one straight, right one
//     transposed), so an elimination reads nothing from another lane;
//   * positions without work carry the identity and zero couplings: MFMAs stay wave-uniform and
//     their products are exact zeros.
// No LDS, no barrier, no address arithmetic between levels.
#pragma once

namespace fold_reg {
constexpr int MAX_RECORDS = 16;                                   // records of one stage
constexpr int set_of_residue(int m) { return m == 1 ? 2 : (m == 2 ? 1 : m); }      // {0, 2, 1, 3}: its own inverse
constexpr int reg_set(int p) { return set_of_residue(p & 3); }    // position -> register set
constexpr int reg_blk(int p) { return p >> 2; }                   // position -> 16-lane block slot b
constexpr int position(int u, int b) { return 4 * b + set_of_residue(u); }
constexpr int owner_lane(int p, int r, int c) { return 16 * r + 4 * reg_blk(p) + c; }
constexpr int levels(int n) { int l = 0; while ((1 << l) < n) ++l; return l; }      // strides s <= n - 1
// position p is eliminated at level l of a stage of n records (row n - 1 is the tail, at no position)
constexpr bool eliminated(int p, int l, int n) { return p < n - 1 && ((p + 1) & ((2 << l) - 1)) == (1 << l); }
// position p is a right neighbour at level l (row p + 1 is a multiple of 2s)
constexpr bool survivor(int p, int l) { return ((p + 1) & ((2 << l) - 1)) == 0; }
constexpr bool right_is_tail(int p, int l, int n) { return p + (1 << l) >= n - 1; }
constexpr bool left_is_outside(int p, int l) { return p < (1 << l); }
constexpr int left_source(int p, int l) { return p - (1 << l); }
constexpr int right_source(int p, int l) { return p + (1 << l); }
// register sets that hold the eliminated positions of level l: the chains carried through the arithmetic
constexpr int chains(int l) { return l == 0 ? 2 : 1; }
constexpr int chain_set(int l, int j) { return l == 0 ? j : (l == 1 ? 2 : 3); }
// where what an elimination in register set u owes its right / left neighbour goes at level l: the register set,
// and by how many lanes of the 16-lane row the value moves towards higher lanes (row_ror: 12 = one b down)
constexpr int right_set(int l, int u) { return l == 0 ? u + 2 : 3; }
constexpr int right_rot(int l, int u) { return l == 2 ? 4 : (l == 3 ? 8 : 0); }
constexpr int left_set(int l, int u) { return l == 0 ? 3 - u : 3; }
constexpr int left_rot(int l, int u) { return (l == 0 && u == 1) ? 0 : (l == 3 ? 8 : 12); }
// the last eliminated position of level l (n >= 2^l + 1); it is the only one whose right neighbour can be the tail
constexpr int last_eliminated(int l, int n) { return ((n - 1 - (1 << l)) / (2 << l)) * (2 << l) + (1 << l) - 1; }
}  // namespace fold_reg

#ifdef __HIPCC__
// lane i of every 16-lane row takes the value of lane (i - ROT) mod 16 of that row
template <int ROT>
__device__ __forceinline__ double row_rot_f64(double v) {
  static_assert(ROT >= 1 && ROT <= 15, "row_ror:1..15");
  const int lo = __builtin_amdgcn_mov_dpp(__double2loint(v), 0x120 + ROT, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_mov_dpp(__double2hiint(v), 0x120 + ROT, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
// sum over the four b of a row, in every lane (each 16-lane row: b = 0..3 of one r)
__device__ __forceinline__ double sum_over_b(double v) {
  v += row_rot_f64<4>(v);
  return v + row_rot_f64<8>(v);
}

// The arithmetic of tile_cr_level_mfma on register operands, U eliminations side by side: Li = L^-1 of
// A = L L^T right-looking over the 16 lanes, G^T = Li Ol, F^T = Li Or^T, x = Li y, then the products.
// Y and the x-products carry their vector in column 0.  FGt = F G^T and GFt = its transpose.
template <int U>
struct RecElim {
  double GGt[U], Gx[U], FFt[U], Fx[U], FGt[U], GFt[U], X[U], piv[U];
  bool f[U];
};
template <int U, bool PRODUCTS = true>
__device__ __forceinline__ void rec_eliminate(int r, double ident, double (&A)[U], const double (&Ol)[U],
                                              const double (&OrT)[U], const double (&Y)[U], RecElim<U>& o) {
  double B[U];
#pragma unroll
  for (int u = 0; u < U; ++u) { B[u] = ident; o.piv[u] = 1.0; o.f[u] = false; }
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const double sel = (r == kk) ? 1.0 : 0.0;
    double rowA[U], rowB[U], p[U], col[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      rowA[u] = mfma444(sel, A[u], 0.0);                         // A[kk][c] in every row
      rowB[u] = mfma444(sel, B[u], 0.0);                         // B[kk][c]
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (kk == 0) { p[u] = quad_bcast_f64<0>(rowA[u]); col[u] = quad_bcast_f64<0>(A[u]); }
      else if (kk == 1) { p[u] = quad_bcast_f64<1>(rowA[u]); col[u] = quad_bcast_f64<1>(A[u]); }
      else if (kk == 2) { p[u] = quad_bcast_f64<2>(rowA[u]); col[u] = quad_bcast_f64<2>(A[u]); }
      else { p[u] = quad_bcast_f64<3>(rowA[u]); col[u] = quad_bcast_f64<3>(A[u]); }
      o.f[u] = o.f[u] || !(p[u] > 0.0);
      o.piv[u] *= p[u];
    }
    double rs[U];
#pragma unroll
    for (int u = 0; u < U; ++u) rs[u] = rsqrt_fast(p[u]);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const double lik = col[u] * rs[u];                         // L[r][kk]
      const double ra = rowA[u] * rs[u], rb = rowB[u] * rs[u];   // L[c][kk];  row kk of B / L[kk][kk]
      if (r > kk) {
        A[u] = __builtin_fma(-lik, ra, A[u]);
        B[u] = __builtin_fma(-lik, rb, B[u]);
      } else if (r == kk) {
        B[u] = rb;
      }
    }
  }
  double Um[U], Gt[U], Ft[U];
#pragma unroll
  for (int u = 0; u < U; ++u) Um[u] = mfma444(B[u], ident, 0.0);          // Li^T
#pragma unroll
  for (int u = 0; u < U; ++u) {
    o.X[u] = mfma444(Um[u], Y[u], 0.0);                          // column 0: x = Li y
    if constexpr (PRODUCTS) {
      Gt[u] = mfma444(Um[u], Ol[u], 0.0);                        // Li Ol   = G^T
      Ft[u] = mfma444(Um[u], OrT[u], 0.0);                       // Li Or^T = F^T
    }
  }
  if constexpr (PRODUCTS) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      o.GGt[u] = mfma444(Gt[u], Gt[u], 0.0);
      o.Gx[u] = mfma444(Gt[u], o.X[u], 0.0);
      o.FFt[u] = mfma444(Ft[u], Ft[u], 0.0);
      o.Fx[u] = mfma444(Ft[u], o.X[u], 0.0);
      o.FGt[u] = mfma444(Ft[u], Gt[u], 0.0);
      o.GFt[u] = mfma444(Gt[u], Ft[u], 0.0);
    }
  }
}

// the stage's rows in registers; see the head of the file
struct RecStage {
  double R[4], Y[4], CL[4], CRt[4];          // positions: row, right-hand side (column 0), J[p, left], J[right, p]^T
  double RK, YK, CLK;                        // the tail row, replicated over b
  double dra, dya;                           // owed to the row left of the group (this lane's b only: sum_over_b at the end)
  double mah;
  PivotLog pl;
  int fcode;                                 // smallest fail code seen by this lane, 0x7fffffff: none
};

// One level.  K = n - 1; rec0 / rows_per_record / N: the rows behind a position, for the fail code.
template <int L>
__device__ __forceinline__ void rec_stage_level(RecStage& t, int K, int b, int r, int c, double ident, int64_t rec0,
                                                int64_t rows_per_record, int64_t N) {
  namespace fr = fold_reg;
  constexpr int S = 1 << L, NU = fr::chains(L), MASK = 2 * S - 1;
  double A[NU], Ol[NU], OrT[NU], Yv[NU];
  bool act[NU], spec[NU];
#pragma unroll
  for (int j = 0; j < NU; ++j) {
    const int u = fr::chain_set(L, j), p = fr::position(u, b);
    act[j] = ((p + 1) & MASK) == S && p < K;
    spec[j] = act[j] && p + S >= K;
    A[j] = act[j] ? t.R[u] : ident;
    Ol[j] = act[j] ? t.CL[u] : 0.0;
    OrT[j] = act[j] ? t.CRt[u] : 0.0;
    Yv[j] = act[j] ? t.Y[u] : 0.0;
  }
  RecElim<NU> e;
  rec_eliminate<NU>(r, ident, A, Ol, OrT, Yv, e);
#pragma unroll
  for (int j = 0; j < NU; ++j) {
    t.mah += e.X[j] * e.X[j];                                    // (zero off column 0 and at idle positions)
    if (act[j] && r == 0 && c == 0) t.pl.mul(e.piv[j]);
    if (act[j] && e.f[j]) {
      int64_t frow = (rec0 + fr::position(fr::chain_set(L, j), b) + 1) * rows_per_record;
      frow = (frow < N ? frow : N) - 1;
      const int code = fail_code(false, true, frow);
      t.fcode = code < t.fcode ? code : t.fcode;
    }
  }
  // ---- the tail: what the level's last elimination owes it, if its right neighbour is the tail ----
  if (fr::last_eliminated(L, K + 1) + S >= K) {                  // (wave-uniform)
    double tR = 0.0, tY = 0.0, tC = 0.0;
#pragma unroll
    for (int j = 0; j < NU; ++j) {
      tR += spec[j] ? e.FFt[j] : 0.0;
      tY += spec[j] ? e.Fx[j] : 0.0;
      tC += spec[j] ? e.FGt[j] : 0.0;
    }
    t.RK -= sum_over_b(tR);
    t.YK -= sum_over_b(tY);
    t.CLK = -sum_over_b(tC);
  }
  // ---- the row left of the group: owed by the level's first elimination (p = s - 1: chain 0) ----
  if (b == fr::reg_blk(S - 1)) {
    t.dra += e.GGt[0];
    t.dya += e.Gx[0];
  }
  // ---- the positions: right neighbours p (p + 1 a multiple of 2 s) take from p - s and p + s ----
  // (every rotation with all lanes on: a DPP read of a lane that is masked off returns nothing; the lanes
  // of b = 3 have no right source inside the stage: the rotation wraps around to b = 0 there)
  if constexpr (L == 0) {
    // chains 0, 1 = sets 0, 1 (positions 4b, 4b + 2); set 2 (4b + 1) takes from both in its own lanes,
    // set 3 (4b + 3) from set 1 in its own lanes and from set 0 one b up
    static_assert(fr::right_set(0, 0) == 2 && fr::right_set(0, 1) == 3 && fr::left_set(0, 1) == 2 && fr::left_set(0, 0) == 3, "");
    static_assert(fr::right_rot(0, 0) == 0 && fr::right_rot(0, 1) == 0 && fr::left_rot(0, 1) == 0, "");
    constexpr int ROT = fr::left_rot(0, 0);
    const double gR = row_rot_f64<ROT>(e.GGt[0]), gY = row_rot_f64<ROT>(e.Gx[0]), gC = row_rot_f64<ROT>(e.GFt[0]);
    t.R[2] -= e.FFt[0];
    t.Y[2] -= e.Fx[0];
    t.CL[2] = -e.FGt[0];
    t.R[2] -= e.GGt[1];
    t.Y[2] -= e.Gx[1];
    if (fr::position(2, b) + S < K) t.CRt[2] = -e.GFt[1];
    t.R[3] -= e.FFt[1];
    t.Y[3] -= e.Fx[1];
    t.CL[3] = -e.FGt[1];
    if (b < 3) {
      t.R[3] -= gR;
      t.Y[3] -= gY;
      if (fr::position(3, b) + S < K) t.CRt[3] = -gC;
    }
  } else if constexpr (L == 1) {
    // chain 0 = set 2 (positions 4b + 1); set 3 (4b + 3) takes from its own lanes and from one b up
    static_assert(fr::right_set(1, 2) == 3 && fr::left_set(1, 2) == 3 && fr::right_rot(1, 2) == 0, "");
    constexpr int ROT = fr::left_rot(1, 2);
    const double gR = row_rot_f64<ROT>(e.GGt[0]), gY = row_rot_f64<ROT>(e.Gx[0]), gC = row_rot_f64<ROT>(e.GFt[0]);
    t.R[3] -= e.FFt[0];
    t.Y[3] -= e.Fx[0];
    t.CL[3] = -e.FGt[0];
    if (b < 3) {
      t.R[3] -= gR;
      t.Y[3] -= gY;
      if (fr::position(3, b) + S < K) t.CRt[3] = -gC;
    }
  } else if constexpr (L == 2) {
    // chain 0 = set 3: positions 3 and 11 (b = 0, 2) are eliminated, 7 (b = 1) takes from both
    static_assert(fr::right_set(2, 3) == 3 && fr::left_set(2, 3) == 3, "");
    constexpr int ROTL = fr::right_rot(2, 3), ROTR = fr::left_rot(2, 3);
    const double fR = row_rot_f64<ROTL>(e.FFt[0]), fY = row_rot_f64<ROTL>(e.Fx[0]), fC = row_rot_f64<ROTL>(e.FGt[0]);
    const double gR = row_rot_f64<ROTR>(e.GGt[0]), gY = row_rot_f64<ROTR>(e.Gx[0]), gC = row_rot_f64<ROTR>(e.GFt[0]);
    if (b == 1) {
      t.R[3] -= fR;
      t.Y[3] -= fY;
      t.CL[3] = -fC;
      t.R[3] -= gR;
      t.Y[3] -= gY;
      if (fr::position(3, b) + S < K) t.CRt[3] = -gC;
    }
  }
  // (level 3 eliminates position 7 alone, between the row left of the group and the tail)
}

// One lane's wave reductions, fixed order: {sum, sum, min}; valid in lane 0
__device__ __forceinline__ void rec_wave_reduce(double& a, double& b2, int& m) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    a += __shfl_down(a, off, 64);
    b2 += __shfl_down(b2, off, 64);
    const int o = __shfl_down(m, off, 64);
    m = o < m ? o : m;
  }
}

// The stage, run by ONE whole wave (all 64 lanes, uniformly).  rin: the stage's n records (1 <= n <= 16),
// RecordLayout<double, 4> apart.  FINAL (wave-uniform; a run-time flag so that a kernel carries this code
// once per call site, not once per form): eliminates the last row too, adds the n_partial partial
// results and writes out2 / info.  Otherwise: writes the stage's record to rout and its partial result
// {sum of squares, sum of log pivots, fail code, 0} to partial_out (with the n_partial partial results of
// partial_in folded in when that is non-null: a shard's single record), all write-through.
// COH: the records and partial results are read with coherent loads only (load_coh).
// rec0: index of the stage's first record among its level's records; rows_per_record, N: for the fail code.
constexpr int REC_STAGE_MAX_PARTIALS = 320;                      // five per lane
template <bool COH>
__device__ __forceinline__ void record_stage_reg(int lane, bool FINAL, const double* rin, int n, double* rout,
                                                 double* partial_out, const double* partial_in,
                                                 int n_partial, double* out2, int* info,
                                                 int64_t rec0, int64_t rows_per_record, int64_t N) {
  using RL = RecordLayout<double, 4>;
  namespace fr = fold_reg;
  const int b = (lane >> 2) & 3, r = lane >> 4, c = lane & 3;
  const int el = 4 * r + c, elT = 4 * c + r;
  const double ident = (r == c) ? 1.0 : 0.0;
  const bool c0 = (c == 0);
  const int K = n - 1;
  CGPS_FSTAMP(0);
  // ---- every load is requested before the first one is waited for ----------------------------------
  double lR[4], lU[4], lC[4], lCr[4], lY[4], lYu[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int p = fr::position(u, b);
    const bool ok = p < K;                                       // lanes without a row read record 0 and discard
    const double* q = rin + (size_t)(ok ? p : 0) * RL::STRIDE;
    const double* q1 = rin + (size_t)(ok ? p + 1 : 0) * RL::STRIDE;
    lR[u] = load_coh<COH>(q + RL::RS + el);
    lU[u] = load_coh<COH>(q1 + RL::DRA + el);
    lC[u] = load_coh<COH>(q + RL::CS + el);
    lCr[u] = load_coh<COH>(q1 + RL::CS + elT);
    lY[u] = load_coh<COH>(q + RL::YS + r);
    lYu[u] = load_coh<COH>(q1 + RL::DYA + r);
  }
  const double* qk = rin + (size_t)K * RL::STRIDE;
  const double kR = load_coh<COH>(qk + RL::RS + el), kC = load_coh<COH>(qk + RL::CS + el), kY = load_coh<COH>(qk + RL::YS + r);
  const double oR = load_coh<COH>(rin + RL::DRA + el), oY = load_coh<COH>(rin + RL::DYA + r);   // the group's own share for the row left of it
  constexpr int PIT = REC_STAGE_MAX_PARTIALS / 64;
  double pm[PIT], pg[PIT], pf[PIT];
#pragma unroll
  for (int it = 0; it < PIT; ++it) {
    const int i = lane + 64 * it;
    const bool ok = partial_in != nullptr && i < n_partial;
    const double* p = (partial_in != nullptr ? partial_in : partial_out) + (size_t)PARTIAL_STRIDE * (ok ? i : 0);
    pm[it] = ok ? load_coh<COH>(p) : 0.0;
    pg[it] = ok ? load_coh<COH>(p + 1) : 0.0;
    pf[it] = ok ? load_coh<COH>(p + 2) : 0.0;
  }
  CGPS_FSTAMP(1);
  RecStage t;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const bool ok = fr::position(u, b) < K;
    t.R[u] = ok ? lR[u] + lU[u] : ident;
    t.Y[u] = (ok && c0) ? lY[u] + lYu[u] : 0.0;
    t.CL[u] = ok ? lC[u] : 0.0;
    t.CRt[u] = ok ? lCr[u] : 0.0;
  }
  t.RK = kR;
  t.YK = c0 ? kY : 0.0;
  t.CLK = kC;
  t.dra = 0.0;
  t.dya = 0.0;
  t.mah = 0.0;
  t.fcode = 0x7fffffff;
  CGPS_FSTAMP(2);
  if (K >= 1) rec_stage_level<0>(t, K, b, r, c, ident, rec0, rows_per_record, N);
  if (K >= 2) rec_stage_level<1>(t, K, b, r, c, ident, rec0, rows_per_record, N);
  if (K >= 4) rec_stage_level<2>(t, K, b, r, c, ident, rec0, rows_per_record, N);
  if (K >= 8) rec_stage_level<3>(t, K, b, r, c, ident, rec0, rows_per_record, N);
  CGPS_FSTAMP(3);
  if (FINAL) {
    // the very last row of the whole system, in the same form (every b carries a copy: b = 0 counts)
    double A[1] = {t.RK}, Z[1] = {0.0}, Yv[1] = {t.YK};
    RecElim<1> e;
    rec_eliminate<1, false>(r, ident, A, Z, Z, Yv, e);
    if (b == 0) t.mah += e.X[0] * e.X[0];
    if (lane == 0) t.pl.mul(e.piv[0]);
    if (e.f[0]) {
      const int code = fail_code(false, true, N - 1);
      t.fcode = code < t.fcode ? code : t.fcode;
    }
    CGPS_FSTAMP(4);
  } else {
    // the stage's record, one element per lane (b = 0)
    const double dra = oR - sum_over_b(t.dra), dya = oY - sum_over_b(t.dya);
    if (b == 0) {
      store_wt(rout + RL::RS + el, t.RK);
      store_wt(rout + RL::CS + el, t.CLK);
      store_wt(rout + RL::DRA + el, dra);
      if (c0) {
        store_wt(rout + RL::YS + r, t.YK);
        store_wt(rout + RL::DYA + r, dya);
      }
    }
  }
  // ---- sums, fixed order: the lane's partial results in index order, then the lanes ----
  double mah = t.mah, logp = t.pl.value();
  int fcode = t.fcode;
#pragma unroll
  for (int it = 0; it < PIT; ++it) {
    mah += pm[it];
    logp += pg[it];
    if (pf[it] != 0.0 && (int)pf[it] < fcode) fcode = (int)pf[it];
  }
  rec_wave_reduce(mah, logp, fcode);
  if (lane == 0) {
    const bool ok = (fcode == 0x7fffffff);
    if (FINAL) {
      // a caller that does not read `info` must not get a plausible number out of a system that is
      // not positive definite
      const double poison = __builtin_nan("");
      out2[0] = ok ? mah : poison;
      out2[1] = ok ? logp : poison;
      *info = ok ? 0 : (fcode & ~FAIL_LATE);
    } else {
      store_wt(partial_out + 0, mah);
      store_wt(partial_out + 1, logp);
      store_wt(partial_out + 2, ok ? 0.0 : (double)fcode);
      store_wt(partial_out + 3, 0.0);
    }
  }
  CGPS_FSTAMP(5);
}
#endif  // __HIPCC__
