// Batched mahal_and_det: many independent block-tridiagonal systems whose blocks are IN MEMORY, in ONE launch
// (cgps_mahal_logdet_batch).  The memory-source sibling of leg_batch_kernel (cgps_tile_leg_batch.h), which assembles
// its rows from time stamps; included from cgps_mahal.hip after cgps_tile.h (the elimination step, the in-LDS
// reduction and the fixed-order sums are reused as they are).
//
// System b is rows [offsets[b], offsets[b+1]) of the concatenated Rs[R][d][d] and x[R][d]; its coupling blocks start
// at block offsets[b] - (os_packed ? b : 0) of Os:
//   os_packed = 0: Os[R-1][d][d] as one concatenated system has it -- the entry between two systems is never read;
//   os_packed = 1: the dense layout [B][n-1][d][d], every system one block shorter than its rows.
// Grid (B), NW = 256 threads, one workgroup per system: no records leave the workgroup, no arrival counters, no atomics
// on global memory.
//   streaming: NT lanes, C = ceil(n_b / NT) rows each, read with load_block / load_vec and eliminated left to right
//              (eliminate_forward), as chunk_reduce_kernel<.., SRC = 0> does for one long system;
//   in LDS:    the lanes' kept rows are reduced by tile_cr (the waves past the lanes are role waves);
//   last row:  thread 0 factors the one row left and adds its pivots;
//   results:   per-thread partial sums are added in a fixed order (block_sum2): a system's two values depend on its own
//              blocks alone, not on where it sits in the batch or what its neighbours hold.
// out2[b] = {x_b^T J_b^-1 x_b, log|J_b|}; info[b]: 0 or 1 + a local row near a block that is not positive definite, that
// system's two values are NaN then.  x == nullptr: the log-determinants alone, out2[b][0] = 0.  A system with n_b < 1 or
// n_b > max_rows is skipped: nothing of its slot is written.
//
// Loads.  The one-system kernel reads odd-d fp64 rows two at a time with 16-byte loads (GROUPED), which needs a lane's
// chunk to start on an even row OF THE ARRAY; a system at an odd offset breaks that, and C is a run-time value here
// anyway.  This kernel uses the ungrouped loads only: load_block takes 16-byte loads exactly when a block is a
// multiple of 16 bytes, and then every block of the array is 16-byte aligned whatever the offset.  YSTAGE (the
// right-hand-side line of four 4 x 4 fp64 rows staged through LDS) is left out: it pays when the grid is many rounds
// of the chip and the line is evicted between a lane's steps; a workgroup here streams at most max_rows rows.
#pragma once

namespace cgps {

constexpr int MAHAL_BATCH_THREADS = 256;

template <typename T, int D, int NT, int NW>
__global__ __launch_bounds__(NW, 1) void mahal_batch_kernel(const T* __restrict__ Rg, const T* __restrict__ Og,
                                                            const T* __restrict__ xg, const int64_t* __restrict__ offsets,
                                                            int os_packed, int64_t max_rows, double* __restrict__ out2,
                                                            int* __restrict__ info) {
  constexpr int DD = D * D;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  StageSmem<T, D, NT, NW> sm(smem);
  const int tid = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int64_t off = offsets[b];
  const int64_t n = offsets[b + 1] - off;
  if (n < 1 || n > max_rows) return;                           // workgroup-uniform
  const T* __restrict__ Rb = Rg + off * DD;
  const T* __restrict__ Ob = Og + (off - (os_packed ? b : 0)) * DD;   // Ob[i] = J_b[i+1][i], i = 0 .. n-2
  const T* __restrict__ xb = xg == nullptr ? nullptr : xg + off * D;
  if (tid == 0) *sm.sfail = 0x7fffffff;

  const int64_t C = (n + NT - 1) / NT;                         // rows per lane
  int64_t r0 = (int64_t)tid * C, rE = r0 + C;
  if (tid >= NT) r0 = n;                                       // threads past the lanes hold no rows
  if (rE > n) rE = n;
  const int L = r0 < n ? (int)(rE - r0) : 0;
  PivotLog pl;
  double mah = 0.0;
  bool fail = false;
  T Rc[D][D], yc[D], Cc[D][D], dRa[D][D], dya[D];
  set_zero<T, D>(dRa);
  set_zero<T, D>(dya);
  set_zero<T, D>(Rc);
  set_zero<T, D>(yc);
  set_zero<T, D>(Cc);
  if (r0 < n) {
    load_block<T, D>(Rb + r0 * DD, Rc);
    if (xb != nullptr) load_vec<T, D>(xb + r0 * D, yc);
    if (r0 >= 1) load_block<T, D>(Ob + (r0 - 1) * DD, Cc);     // row 0 of the system has no left neighbour
  }
#pragma unroll 1
  for (int j = 0; j < L - 1; ++j) {
    const int64_t rn = r0 + j + 1;                             // 1 <= rn <= n - 1: Ob[rn - 1] is the system's own
    T Rn[D][D], On[D][D], yn[D];
    load_block<T, D>(Rb + rn * DD, Rn);
    load_block<T, D>(Ob + (rn - 1) * DD, On);
    if (xb != nullptr) load_vec<T, D>(xb + rn * D, yn);
    else set_zero<T, D>(yn);
    eliminate_forward<T, D>(Rc, yc, Cc, dRa, dya, On, Rn, yn, pl, mah, fail);
  }
  const bool fail_stream = fail;
  const int n_real = (int)((n + C - 1) / C);                   // lanes that hold rows (<= NT)
  // lane 0's Cc is zero, so what the tile owes "the row left of it" is zero as well and the tile's boundary row is
  // the system's last row
  reduce_tile_and_emit<T, D, NW>(sm.t, Rc, yc, Cc, dRa, dya, n_real, sm.xch, (T*)nullptr, pl, mah, fail);
  if (tid == 0) {                                              // the one row left: the system's last
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
  if (tid == 0) {
    const int f = *sm.sfail;
    const bool ok = f == 0x7fffffff;
    const double poison = __builtin_nan("");
    out2[2 * b] = ok ? mah : poison;
    out2[2 * b + 1] = ok ? logp : poison;
    info[b] = ok ? 0 : (f & ~FAIL_LATE);
  }
}

// the block sizes with one lane per row in stage 1: the set of the LEG batch (not d = 8, not fp64 d = 6)
template <typename T, int D>
constexpr bool mahal_batch_supported() { return TileCfg<T, D>::LPR == 1; }

// -2: not built for this (d, dtype)
template <typename T, int D>
int run_mahal_batch(const T* Rs, const T* Os, const T* x, const int64_t* offsets, int64_t B, int os_packed,
                    int64_t max_rows, double* out2, int* info, hipStream_t st) {
  if constexpr (!mahal_batch_supported<T, D>()) {
    return -2;
  } else {
    constexpr int NT = TileCfg<T, D>::NG1, NW = MAHAL_BATCH_THREADS;     // 256 lanes, or 128 for 7 x 7 fp64 (LDS)
    const size_t lds = stage_lds_bytes<T, D>(NT, NW);
    static std::once_flag once[TILE_MAX_DEVICES];              // attributes belong to a device
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (dev < 0 || dev >= TILE_MAX_DEVICES) dev = 0;
    std::call_once(once[dev], [lds] {
      (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&mahal_batch_kernel<T, D, NT, NW>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    });
    hipLaunchKernelGGL((mahal_batch_kernel<T, D, NT, NW>), dim3((unsigned)B), dim3(NW), lds, st, Rs, Os, x, offsets,
                       os_packed, max_rows, out2, info);
    return 0;
  }
}

}  // namespace cgps
