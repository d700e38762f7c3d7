// Batched LEG log-likelihood reductions: many independent series in ONE launch (cgps_leg_loglik_batch,
// cgps_leg_loglik_batch_obs for rows that differ in what they observe, and cgps_leg_loglik_batch_w for rows with noise
// variances of their own).
// Included from cgps_mahal.hip and from cgps_leg_obs.hip, after cgps_host.h and cgps_tile.h (the chunk walk, the in-LDS
// reduction and the in-register assembly of cgps_tile_leg.h are reused as they are).
//
// Series b is rows [offsets[b], offsets[b+1]) of the concatenated ts / v / q.  Its two systems
//     K_b = PEG precision(ts_b, G) + blockdiag(A)        (posterior precision, right-hand side v_b)
//     S_b = PEG precision(ts_b, G)                        (prior precision, no right-hand side)
// do not couple to any other series, so each is reduced by ONE workgroup on its own: no records leave the
// workgroup, no arrival counters, no inter-workgroup hand-off.  Grid (B, 2): blockIdx.x = series,
// blockIdx.y = 0 for K_b, 1 for S_b (the gridDim.y = 2 layout of cgps_leg_mahal_logdet_pair).
//   streaming: NT lanes, C = ceil(n_b / NT) rows each; a lane assembles its rows in registers from ts and G
//              (leg_row / leg_gap) and eliminates them left to right (eliminate_forward), exactly as
//              chunk_reduce_kernel<.., SRC = 1> does for one long series;
//   in LDS:    the lanes' kept rows are reduced by tile_cr (NW = 256 threads, the extra waves are role waves);
//   last row:  thread 0 factors the one row left and adds its pivots;
//   results:   per-thread partial sums are added in a fixed order (block_sum2), so the values do not depend on
//              anything but the series itself.  The K workgroup also sums q over the series' rows.
// out4[b] = {v^T K^-1 v, log|K|, log|S|, sum of q}; info2[2b] / info2[2b+1]: 0 or 1 + a local row near a block of
// K_b / S_b that was not positive definite (a zero-length gap included); a failed system's entries are NaN.
// A series with more than max_rows rows is skipped (nothing written: the caller reduces it with another call).
//
// ROWS names where a row's diagonal term comes from (LEG_ROWS_PLAIN: the one block Ag, the same for every row).
// ROWS = LEG_ROWS_TABLE (cgps_leg_loglik_batch_obs): rows differ in what they observe.  Ag is then a table of `entries`
// blocks and row r of series b adds entry pattern[offsets[b] + r] of it (leg_obs_block in cgps_tile_leg.h: the index is
// clamped, the block is read with per-lane vector loads straight from global memory -- at most 256 blocks, they stay in
// cache); `pattern` holds one byte per row of the CONCATENATED batch.  The prior-precision workgroup has a null table
// and reads neither table nor pattern.
// ROWS = LEG_ROWS_WEIGHTED (cgps_leg_loglik_batch_w): every row has noise of its own.  The same arguments carry other
// things, as FoldArgs does for chunk_reduce_kernel<.., SRC = 3>: Ag is a basis of `entries` = Kb blocks and `pattern`
// points at the weights of the CONCATENATED batch, [sum n_b][Kb] values of T; row r of series b adds
// sum_k weights[(offsets[b] + r) Kb + k] basis[k] to the carried toRight term before leg_row assembles the row with no A
// (leg_add_weighted_basis in cgps_tile_leg.h, and its note on that placement).  The prior-precision workgroup has a
// null basis and reads neither basis nor weights.
// ROWS = LEG_ROWS_MODELS (cgps_leg_loglik_models): M models over the same batch, grid (B, 2, M).  blockIdx.z = k names
// the model: the workgroup moves G, A, v, q, out4 and info2 to model k's slices (G[M][d][d], A[M][d][d], v[M][R][d],
// q[M][R] with R = model_rows, out4[M][B][4], info2[M][B][2]) and is a LEG_ROWS_PLAIN workgroup from there on.  k is
// workgroup-uniform, so G[k] and A[k] still arrive through scalar loads.
// ROWS = LEG_ROWS_MODELS_TABLE (cgps_leg_loglik_models_obs) and LEG_ROWS_MODELS_WEIGHTED (cgps_leg_loglik_models_w): the
// product of the two axes, grid (B, 2, M).  "Which model" (leg_rows_models) and "where a row's diagonal term comes
// from" (leg_rows_source) are read off ROWS separately.  The model prologue moves one more slice: the table by
// k entries d d (A_table[M][P][d][d]; `pattern`, one byte per row, describes the batch once and is read by every
// model), or the basis by k entries d d and the weights by k model_rows entries (basis[M][Kb][d][d],
// weights[M][R][Kb]: the weights hold the entries of each model's own Li).  From there on the workgroup is a
// LEG_ROWS_TABLE / LEG_ROWS_WEIGHTED workgroup; the offsets are 64-bit products of workgroup-uniform values.
// LEG_ROWS_PLAIN reads neither argument, and every difference is an `if constexpr` on the kernel itself: each source's
// instruction stream is the one it had before the others existed.  One launcher (run_leg_rows) and one entry-point helper
// (leg_rows_entry) serve all six; the TABLE and WEIGHTED kernels, with and without models, are instantiated by
// cgps_leg_obs.hip, PLAIN and MODELS by cgps_mahal.hip.
#pragma once

namespace cgps {

constexpr int LEG_BATCH_THREADS = 256;
constexpr int LEG_ROWS_PLAIN = 0, LEG_ROWS_TABLE = 1, LEG_ROWS_WEIGHTED = 2, LEG_ROWS_MODELS = 3, LEG_ROWS_MODELS_TABLE = 4,
              LEG_ROWS_MODELS_WEIGHTED = 5;

constexpr bool leg_rows_models(int rows) { return rows >= LEG_ROWS_MODELS; }        // blockIdx.z names a model
constexpr int leg_rows_source(int rows) {                                            // PLAIN, TABLE or WEIGHTED
  return rows == LEG_ROWS_MODELS_TABLE ? LEG_ROWS_TABLE
         : rows == LEG_ROWS_MODELS_WEIGHTED ? LEG_ROWS_WEIGHTED
         : rows == LEG_ROWS_MODELS ? LEG_ROWS_PLAIN : rows;
}

template <typename T, int D>
constexpr int leg_batch_lanes() { return TileCfg<T, D>::NG1; }       // 256, or 128 for 7 x 7 fp64 (LDS)

template <typename T, int D, int NT, int NW, int ROWS = LEG_ROWS_PLAIN>
__global__ __launch_bounds__(NW, 1) void leg_batch_kernel(const T* __restrict__ ts, const int64_t* __restrict__ offsets,
                                                          const T* __restrict__ Gg, const T* __restrict__ Ag,
                                                          const T* __restrict__ vg, const T* __restrict__ qg,
                                                          int64_t max_rows, double* __restrict__ out4,
                                                          int* __restrict__ info2, int entries,
                                                          const unsigned char* __restrict__ pattern,
                                                          int64_t model_rows = 0) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  StageSmem<T, D, NT, NW> sm(smem);
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  constexpr int SRC = leg_rows_source(ROWS);
  if constexpr (leg_rows_models(ROWS)) {                       // model k's slices (workgroup-uniform)
    const int64_t k = blockIdx.z;
    Gg += k * (D * D);
    if constexpr (SRC == LEG_ROWS_PLAIN) {
      if (Ag != nullptr) Ag += k * (D * D);
    } else {                                                   // model k's table / basis; its weights (the bytes are shared)
      Ag += k * (int64_t)entries * (D * D);
      if constexpr (SRC == LEG_ROWS_WEIGHTED) pattern += k * model_rows * (int64_t)entries * (int64_t)sizeof(T);
    }
    if (vg != nullptr) vg += k * model_rows * D;
    if (qg != nullptr) qg += k * model_rows;
    out4 += k * (int64_t)gridDim.x * 4;
    info2 += k * (int64_t)gridDim.x * 2;
  }
  const bool prior = blockIdx.y == 1;
  const int64_t off = offsets[b];
  const int64_t n = offsets[b + 1] - off;
  if (n < 1 || n > max_rows) return;                           // workgroup-uniform
  const T* __restrict__ tsb = ts + off;
  const T* __restrict__ vb = (prior || vg == nullptr) ? nullptr : vg + off * D;
  const T* __restrict__ Ab = prior ? nullptr : Ag;
  // the series' own bytes / weights: what the rows below index is the local row plus the series' offset
  const unsigned char* __restrict__ pb = SRC == LEG_ROWS_TABLE ? pattern + off : nullptr;
  const T* __restrict__ wb = SRC == LEG_ROWS_WEIGHTED ? reinterpret_cast<const T*>(pattern) + off * (int64_t)entries : nullptr;
  if (tid == 0) *sm.sfail = 0x7fffffff;

  const int64_t C = (n + NT - 1) / NT;                         // rows per lane
  int64_t r0 = (int64_t)tid * C, rE = r0 + C;
  if (tid >= NT) r0 = n;                                       // threads past the lanes hold no rows
  if (rE > n) rE = n;
  const int L = r0 < n ? (int)(rE - r0) : 0;
  PivotLog pl;
  double mah = 0.0;
  bool fail = false;
  T Rc[D][D], yc[D], Cc[D][D], dRa[D][D], dya[D], cR[D][D], cB[D][D];
  set_zero<T, D>(dRa);
  set_zero<T, D>(dya);
  set_zero<T, D>(Rc);
  set_zero<T, D>(yc);
  set_zero<T, D>(Cc);
  if (r0 < n) {
    if (r0 >= 1) {
      T tl[D][D];
      if (!leg_gap<T, D>(tsb, Gg, r0 - 1, cR, tl, cB)) fail = true;
    } else {
      set_zero<T, D>(cR);
      set_zero<T, D>(cB);
    }
    if constexpr (SRC == LEG_ROWS_TABLE)
      leg_row<T, D>(tsb, Gg, leg_obs_block<T, D>(Ab, pb, entries, r0), vb, r0, n, cR, cB, Rc, Cc, yc, fail);
    else if constexpr (SRC == LEG_ROWS_WEIGHTED) {
      leg_add_weighted_basis<T, D>(Ab, wb, entries, r0, cR);
      leg_row<T, D>(tsb, Gg, (const T*)nullptr, vb, r0, n, cR, cB, Rc, Cc, yc, fail);
    } else
      leg_row<T, D>(tsb, Gg, Ab, vb, r0, n, cR, cB, Rc, Cc, yc, fail);
  }
#pragma unroll 1
  for (int j = 0; j < L - 1; ++j) {
    T Rn[D][D], On[D][D], yn[D];
    if constexpr (SRC == LEG_ROWS_TABLE)
      leg_row<T, D>(tsb, Gg, leg_obs_block<T, D>(Ab, pb, entries, r0 + j + 1), vb, r0 + j + 1, n, cR, cB, Rn, On, yn, fail);
    else if constexpr (SRC == LEG_ROWS_WEIGHTED) {
      leg_add_weighted_basis<T, D>(Ab, wb, entries, r0 + j + 1, cR);
      leg_row<T, D>(tsb, Gg, (const T*)nullptr, vb, r0 + j + 1, n, cR, cB, Rn, On, yn, fail);
    } else
      leg_row<T, D>(tsb, Gg, Ab, vb, r0 + j + 1, n, cR, cB, Rn, On, yn, fail);
    eliminate_forward<T, D>(Rc, yc, Cc, dRa, dya, On, Rn, yn, pl, mah, fail);
  }
  const bool fail_stream = fail;
  const int n_real = (int)((n + C - 1) / C);                   // lanes that hold rows (<= NT)
  // row 0 of the series has no left neighbour: lane 0's Cc is zero, so its updates for "the row left of the
  // tile" are zero as well and the tile's boundary row is the series' last row
  reduce_tile_and_emit<T, D, NW>(sm.t, Rc, yc, Cc, dRa, dya, n_real, sm.xch, (T*)nullptr, pl, mah, fail);
  if (tid == 0) {                                              // the one row left: the series' last
    T A[D][D], x[D];
    Chol<T, D> c;
    LdsTile<T, D>::load_blk(sm.t.R, n_real - 1, A);
    pl.mul(chol_lower<T, D>(A, c, fail), c);
    load_vec<T, D>(sm.t.y + (n_real - 1) * D, x);
    fwd_subst<T, D>(c, x);
#pragma unroll
    for (int i = 0; i < D; ++i) mah += (double)x[i] * (double)x[i];
  }
  const int fcode = fail_code(fail_stream, fail, r0 < n ? r0 : n - 1);
  if (fcode) atomicMin(sm.sfail, fcode);
  double logp = pl.value();
  block_sum2<NW>(mah, logp, sm.red);                           // contains a barrier (NW > 64)
  double qs = 0.0, unused = 0.0;
  if (!prior && qg != nullptr) {
    for (int64_t i = tid; i < n; i += NW) qs += (double)qg[off + i];
  }
  __syncthreads();                                             // sm.red is reused
  block_sum2<NW>(qs, unused, sm.red);
  if (tid == 0) {
    const int f = *sm.sfail;
    const bool ok = f == 0x7fffffff;
    const double poison = __builtin_nan("");
    double* o = out4 + 4 * b;
    if (prior) {
      o[2] = ok ? logp : poison;
    } else {
      o[0] = ok ? mah : poison;
      o[1] = ok ? logp : poison;
      o[3] = qs;
    }
    info2[2 * b + (prior ? 1 : 0)] = ok ? 0 : (f & ~FAIL_LATE);
  }
}

template <typename T, int D>
constexpr bool leg_batch_supported() { return leg_source_supported<T, D>(); }

template <typename T, int D>
size_t leg_batch_lds_bytes() { return stage_lds_bytes<T, D>(leg_batch_lanes<T, D>(), LEG_BATCH_THREADS); }

// The one launcher of the six forms.  -2: not built for this (d, dtype).  The arguments are the union of what the forms
// take: A is the block, the table or the basis; `entries` and `pattern` are read by the TABLE and WEIGHTED sources (the
// weights travel as bytes); M and model_rows by the models forms alone, whose grid is (B, 2, M).  The ranges of entries and
// M and the non-null pointers are the caller's checks.
template <typename T, int D, int ROWS>
int run_leg_rows(const T* ts, const int64_t* offsets, int64_t B, int64_t M, int64_t model_rows, const T* G, const T* A,
                 int entries, const unsigned char* pattern, const T* v, const T* q, int64_t max_rows, double* out4,
                 int* info2, hipStream_t st) {
  if constexpr (!leg_batch_supported<T, D>()) {
    return -2;
  } else {
    if (B == 0) return 0;                                      // nothing to do: the runtime is not touched
    constexpr int NT = leg_batch_lanes<T, D>(), NW = LEG_BATCH_THREADS;
    const size_t lds = leg_batch_lds_bytes<T, D>();
    static std::once_flag once[TILE_MAX_DEVICES];              // attributes belong to a device (and to an instantiation)
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= TILE_MAX_DEVICES) dev = 0;
    std::call_once(once[dev], [lds] {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&leg_batch_kernel<T, D, NT, NW, ROWS>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
    const dim3 grid((unsigned)B, 2u, leg_rows_models(ROWS) ? (unsigned)M : 1u);
    hipLaunchKernelGGL((leg_batch_kernel<T, D, NT, NW, ROWS>), grid, dim3(NW), lds, st, ts, offsets, G, A, v, q, max_rows, out4,
                       info2, entries, pattern, model_rows);
    return 0;
  }
}

}  // namespace cgps

namespace cgps_host {

// What the six extern "C" entry points (cgps_leg_loglik_batch{,_obs,_w}, cgps_leg_loglik_models{,_obs,_w}) share: the
// argument checks, the dispatch over dtype and d, and the launch.  `name` is the entry point's, `label` names its launch
// in a HIP error; `missing` says that one of the pointers that this form alone requires is null (with B = 0 none is
// looked at).  The plain forms pass entries = 0 and a null pattern, the one-model forms R = 0 and M = 1; the range of
// P / Kb is the entry point's own check.
template <int ROWS>
int leg_rows_entry(const char* name, const char* label, bool missing, const void* ts, const int64_t* offsets, int64_t B,
                   int64_t R, int64_t M, const void* G, const void* A, int entries, const void* pattern, const void* v,
                   const void* q, int d, int dtype, int64_t max_rows, double* out4, int* info2, void* stream) {
  constexpr bool MODELS = cgps::leg_rows_models(ROWS);
  if (MODELS && (M < 1 || M > 65535)) return fail(CGPS_ERR_ARG, "%s: M = %lld models, outside 1..65535", name, (long long)M);
  if (B < 0 || R < 0 || d < 1 || (B > 0 && (missing || !ts || !offsets || !G || !out4 || !info2)))
    return fail(CGPS_ERR_ARG, MODELS ? "%s: null pointer, B < 0 or R < 0" : "%s: null pointer or B < 0", name);
  if (B > 0x7fffffffLL) return fail(CGPS_ERR_ARG, "%s: B = %lld series, at most 2^31 - 1", name, (long long)B);
  return dispatch(dtype, d, [&](auto t, auto dc) {
    using T = decltype(t);
    constexpr int D = decltype(dc)::value;
    const int rc = cgps::run_leg_rows<T, D, ROWS>((const T*)ts, offsets, B, M, R, (const T*)G, (const T*)A, entries,
                                                  (const unsigned char*)pattern, (const T*)v, (const T*)q, max_rows, out4,
                                                  info2, (hipStream_t)stream);
    if (rc == -2) return fail(CGPS_ERR_UNSUPPORTED, "%s: not built for this block size (d = 8, fp64 d = 6)", name);
    if (B == 0) return (int)CGPS_OK;
    return check_launch(label);
  });
}

}  // namespace cgps_host
