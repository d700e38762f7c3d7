// Developer micro-benchmarks for the fused path (not part of the library).
// Build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -o cyclic-gps_amd/lib/dev_bench cyclic-gps_amd/csrc/dev_bench.hip
// Run on the GPU box: ./cyclic-gps_amd/lib/dev_bench [log2N]
//   dev_bench 20 1: tile_cr alone | 20 2 1: stamps inside the one-launch pipeline | 20 3: one record stage alone |
//   20 4: a full tile's first levels, staged in LDS against in the streaming lanes' registers (cgps_tile_wave.h)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CGPS_FIN_STAMPS 1
#ifndef DEVB_D
#define DEVB_D 4          // block size of the tile_cr and timeline modes (-DDEVB_D=5 ...)
#endif
#ifndef DEVB_T
#define DEVB_T double     // scalar type of the tile_cr mode (-DDEVB_T=float)
#endif
#include "cgps_tile.h"

using namespace cgps;

template <typename T, int D>
__device__ __forceinline__ void set_identity(T (&A)[D][D]) {
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) A[i][j] = (i == j) ? T(1) : T(0);
}

#define CK(x)                                                                      \
  do {                                                                             \
    hipError_t e_ = (x);                                                           \
    if (e_ != hipSuccess) {                                                        \
      printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      exit(1);                                                                     \
    }                                                                              \
  } while (0)

// cheap deterministic SPD block-tridiagonal generator: R = (2 + u) I + small symmetric, O small
template <typename T, int D>
__global__ void gen_kernel(T* R, T* O, T* y, int64_t N) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N) return;
  unsigned h = (unsigned)(i * 2654435761u) ^ 0x9e3779b9u;
  auto rnd = [&]() { h = h * 1664525u + 1013904223u; return (T)((h >> 8) & 0xffff) / (T)65536 - (T)0.5; };
  for (int a = 0; a < D; ++a)
    for (int b = 0; b <= a; ++b) {
      T v = (a == b) ? (T)2.5 + (T)0.2 * rnd() : (T)0.1 * rnd();
      R[i * D * D + a * D + b] = v;
      R[i * D * D + b * D + a] = v;
    }
  if (i < N - 1)
    for (int a = 0; a < D * D; ++a) O[i * D * D + a] = (T)0.3 * rnd();
  for (int a = 0; a < D; ++a) y[i * D + a] = rnd();
}

// ---- V2: the stage-1 access pattern with no arithmetic to speak of ----------------------
template <typename T, int D, int C, int NT>
__global__ __launch_bounds__(NT) void loads_only_kernel(const T* __restrict__ Rg, const T* __restrict__ Og,
                                                        const T* __restrict__ yg, int64_t N, double* out) {
  constexpr int DD = D * D;
  const int64_t r0 = ((int64_t)blockIdx.x * NT + threadIdx.x) * C;
  T acc = 0;
#pragma unroll 1
  for (int j = 0; j < C; ++j) {
    const int64_t rn = r0 + j;
    if (rn < N - 1) {
      T Rn[D][D], On[D][D], yn[D];
      load_block<T, D>(Rg + rn * DD, Rn);
      load_block<T, D>(Og + rn * DD, On);
      load_vec<T, D>(yg + rn * D, yn);
#pragma unroll
      for (int a = 0; a < D; ++a) {
        acc += yn[a];
#pragma unroll
        for (int b = 0; b < D; ++b) acc += Rn[a][b] + On[a][b];
      }
    }
  }
  if (acc == (T)123456.789) out[0] = acc;
}

// ---- V2b: fully coalesced streaming read of the same bytes ------------------------------
__global__ __launch_bounds__(256) void coalesced_read_kernel(const double2* __restrict__ p, int64_t n16, double* out) {
  double acc = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 256) {
    double2 v = p[i];
    acc += v.x + v.y;
  }
  if (acc == 123456.789) out[0] = acc;
}

// ---- V1: chunk phase only (no LDS reduction) ---------------------------------------------
template <typename T, int D, int C, int NT>
__global__ __launch_bounds__(NT) void chunk_only_kernel(const T* __restrict__ Rg, const T* __restrict__ Og,
                                                        const T* __restrict__ yg, int64_t N, double* out) {
  constexpr int DD = D * D;
  const int64_t r0 = ((int64_t)blockIdx.x * NT + threadIdx.x) * C;
  PivotLog pl;
  double mah = 0.0;
  bool fail = false;
  T Rc[D][D], yc[D], Cc[D][D], dRa[D][D], dya[D];
  set_zero<T, D>(dRa);
  set_zero<T, D>(dya);
  if (r0 < N) {
    load_block<T, D>(Rg + r0 * DD, Rc);
    load_vec<T, D>(yg + r0 * D, yc);
  } else {
    set_identity<T, D>(Rc);
    set_zero<T, D>(yc);
  }
  if (r0 >= 1 && r0 < N) load_block<T, D>(Og + (r0 - 1) * DD, Cc);
  else set_zero<T, D>(Cc);
#pragma unroll 1
  for (int j = 0; j < C - 1; ++j) {
    const int64_t rn = r0 + j + 1;
    T Rn[D][D], On[D][D], yn[D];
    if (rn < N) {
      load_block<T, D>(Rg + rn * DD, Rn);
      load_block<T, D>(Og + (rn - 1) * DD, On);
      load_vec<T, D>(yg + rn * D, yn);
    } else {
      set_identity<T, D>(Rn);
      set_zero<T, D>(On);
      set_zero<T, D>(yn);
    }
    eliminate_forward<T, D>(Rc, yc, Cc, dRa, dya, On, Rn, yn, pl, mah, fail);
  }
  double s = mah + pl.value() + (double)Rc[0][0] + (double)Cc[0][0] + (double)dRa[0][0] + (double)dya[0] + (double)yc[0];
  if (s == 123456.789 || fail) out[0] = s;
}

// ---- probe: lane maps of v_mfma_f64_4x4x4_4b_f64 ------------------------------------------
__global__ void mfma_probe_kernel(int* table) {
  const int lane = threadIdx.x;
  for (int la = 0; la < 64; ++la)
    for (int lb = 0; lb < 64; ++lb) {
      double a = (lane == la) ? 1.0 : 0.0, b = (lane == lb) ? 1.0 : 0.0;
      double d = __builtin_amdgcn_mfma_f64_4x4x4f64(a, b, 0.0, 0, 0, 0);
      if (d != 0.0) table[la * 64 + lb] = lane;
    }
}
static void run_mfma_probe() {
  int* table;
  CK(hipMalloc(&table, 4096 * sizeof(int)));
  CK(hipMemset(table, 0xff, 4096 * sizeof(int)));
  hipLaunchKernelGGL(mfma_probe_kernel, dim3(1), dim3(64), 0, 0, table);
  CK(hipDeviceSynchronize());
  std::vector<int> h(4096);
  CK(hipMemcpy(h.data(), table, 4096 * sizeof(int), hipMemcpyDeviceToHost));
  printf("mfma_f64_4x4x4 probe: for A-lane la: list of (B-lane -> D-lane)\n");
  for (int la = 0; la < 64; ++la) {
    if (!(la < 20 || la == 32 || la == 48)) continue;
    printf("  la=%2d:", la);
    for (int lb = 0; lb < 64; ++lb)
      if (h[la * 64 + lb] >= 0) printf(" (%d->%d)", lb, h[la * 64 + lb]);
    printf("\n");
  }
}


// ---- tile_cr alone: one 256-slot tile per workgroup, per-policy wall time of the in-LDS reduction ----
// (wall_clock64: 100 MHz).  n_real rows are regenerated before every repetition; the time of the
// reduction itself is stamped by thread 0 between two barriers.
template <int NTHR, int MW>
__global__ __launch_bounds__(NTHR) void tilecr_bench_kernel(int n_real, int reps, long long* ticks, double* sums) {
  using T = DEVB_T;
  constexpr int D = DEVB_D;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  StageSmem<T, D, 256, NTHR> sm(smem);
  const int tid = threadIdx.x;
  long long acc = 0;
  double mah = 0.0;
  PivotLog pl;
  bool fail = false;
  for (int rep = 0; rep < reps; ++rep) {
    if (tid < n_real) {
      unsigned h = (unsigned)((tid + 977 * blockIdx.x) * 2654435761u) ^ 0x9e3779b9u;
      auto rnd = [&]() { h = h * 1664525u + 1013904223u; return (T)((h >> 8) & 0xffff) / (T)65536 - (T)0.5; };
      T R[D][D], O[D][D], y[D];
      for (int a = 0; a < D; ++a) {
        for (int b = 0; b <= a; ++b) { T v = (a == b) ? (T)2.5 + (T)0.2 * rnd() : (T)0.1 * rnd(); R[a][b] = v; R[b][a] = v; }
        for (int b = 0; b < D; ++b) O[a][b] = (T)0.3 * rnd();
        y[a] = rnd();
      }
      LdsTile<T, D>::store_blk(sm.t.R, tid, R);
      LdsTile<T, D>::store_blk(sm.t.Oc, tid, O);
      store_vec<T, D>(sm.t.y + tid * D, y);
    }
    __syncthreads();
    const long long t0 = wall_clock64();
    tile_cr<T, D, NTHR, MW>(sm.t, n_real, pl, mah, fail);
    const long long t1 = wall_clock64();
    __syncthreads();
    acc += t1 - t0;
  }
  double logp = pl.value();
  block_sum2<NTHR>(mah, logp, sm.red);
  if (tid == 0) {
    ticks[blockIdx.x] = acc;
    sums[2 * blockIdx.x] = mah;
    sums[2 * blockIdx.x + 1] = logp;
  }
}

template <int NTHR, int MW>
void run_tilecr(int grid, hipStream_t st) {
  const size_t lds = stage_lds_bytes<DEVB_T, DEVB_D>(256, NTHR);
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&tilecr_bench_kernel<NTHR, MW>),
                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  long long* ticks;
  double* sums;
  CK(hipMalloc(&ticks, grid * sizeof(long long)));
  CK(hipMalloc(&sums, 2 * grid * sizeof(double)));
  const int reps = 50;
  printf("tile_cr NTHR=%d MW=%d grid=%d :", NTHR, MW, grid);
  double prev = 0;
  for (int n_real : {2, 4, 8, 16, 32, 64, 128, 256}) {
    hipLaunchKernelGGL((tilecr_bench_kernel<NTHR, MW>), dim3(grid), dim3(NTHR), lds, st, n_real, reps, ticks, sums);
    CK(hipStreamSynchronize(st));
    std::vector<long long> h(grid);
    std::vector<double> hs(2 * grid);
    CK(hipMemcpy(h.data(), ticks, grid * sizeof(long long), hipMemcpyDeviceToHost));
    CK(hipMemcpy(hs.data(), sums, 2 * grid * sizeof(double), hipMemcpyDeviceToHost));
    double avg = 0;
    for (auto v : h) avg += (double)v;
    avg = avg / grid / reps * 10.0;   // ns
    printf("  n=%d: %.0f ns (+%.0f)", n_real, avg, avg - prev);
    if (n_real == 256) printf("  [check %.10g %.10g]", hs[0], hs[1]);
    prev = avg;
  }
  printf("\n");
  CK(hipFree(ticks));
  CK(hipFree(sums));
}

// ---- the first L levels of one full 256-row tile alone: staged in LDS + L quad levels of tile_cr against the same
// levels in the streaming lanes' registers + hand-over (cgps_tile_wave.h).  One workgroup of NTHR threads; every lane
// carries a kept row, its coupling and an update owed to the row on its left, regenerated before every repetition;
// thread 0 stamps each form between two barriers.  After the last repetition the LDS state the in-register form
// leaves is compared with what the staged form left, as level L reads it: survivors' rows and right-hand sides LESS
// what is parked for them (the staged levels take earlier levels' updates off a row as they go and park only the
// last level's, the in-register levels park the sum: only the difference is defined), their couplings, and the share
// of the row left of the tile (largest relative difference, elements of size >= 1e-3).
template <int L, int NTHR>
__global__ __launch_bounds__(NTHR) void wave_levels_bench_kernel(int reps, long long* ticks, double* diff, double* sums, double* snap) {
  constexpr int D = 4, NT = 256, S = 1 << L;
  using LT = LdsTile<double, D>;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  StageSmem<double, D, NT, NTHR> sm(smem);
  const int tid = threadIdx.x;
  long long acc[2] = {0, 0};
  double mahs[2] = {0.0, 0.0}, logs[2] = {0.0, 0.0};
  double worst = 0.0;
  for (int rep = 0; rep < reps; ++rep) {
#pragma unroll
    for (int form = 0; form < 2; ++form) {
      double Rc[D][D], yc[D], Cc[D][D], dRa[D][D], dya[D];
      unsigned h = (unsigned)((tid + 977 * rep) * 2654435761u) ^ 0x9e3779b9u;
      auto rnd = [&]() { h = h * 1664525u + 1013904223u; return (double)((h >> 8) & 0xffff) / 65536.0 - 0.5; };
      for (int a = 0; a < D; ++a) {
        for (int b = 0; b <= a; ++b) {
          const double v = (a == b) ? 2.5 + 0.2 * rnd() : 0.1 * rnd(), u = (a == b) ? -0.2 - 0.1 * rnd() : 0.02 * rnd();
          Rc[a][b] = v; Rc[b][a] = v; dRa[a][b] = u; dRa[b][a] = u;
        }
        for (int b = 0; b < D; ++b) Cc[a][b] = 0.3 * rnd();
        yc[a] = rnd();
        dya[a] = 0.1 * rnd();
      }
      if (tid >= NT) { set_zero<double, D>(Rc); set_zero<double, D>(yc); set_zero<double, D>(Cc); set_zero<double, D>(dRa); set_zero<double, D>(dya); }
      PivotLog pl;
      double mah = 0.0;
      bool fail = false;
      __syncthreads();
      const long long t0 = wall_clock64();
      if (form == 0) {
        stage_kept_rows<double, D, NTHR>(sm.t, Rc, yc, Cc, dRa, dya, NT, sm.xch);
        __syncthreads();
        for (int s = 1; s < S; s <<= 1) tile_cr_level_quad<double, D, NTHR>(sm.t, tid, NT - 1, NT / s, s, pl, mah, fail);
      } else {
        wave_levels_and_hand_over<L, NT>(sm.t, tid, Rc, yc, Cc, dRa, dya, sm.xch, pl, mah, fail);
        __syncthreads();
      }
      const long long t1 = wall_clock64();
      acc[form] += t1 - t0;
      mahs[form] += mah;
      logs[form] += pl.value();
      if (rep == reps - 1 && tid < NT && wave_levels::survives(tid, L)) {
        double A[D][D], B[D][D], P[D][D], a[D], p[D];
        LT::load_blk(sm.t.R, tid, A);
        LT::load_blk(sm.t.Oc, wave_levels::coupling_slot(tid, L), B);
        load_vec<double, D>(sm.t.y + tid * D, a);
        if (tid + (S >> 1) < NT - 1) {            // pending for this row: parked by the survivor on its right
          double Q[D][D], q[D];
          LT::load_blk(sm.t.R, tid + (S >> 1), Q);
          load_vec<double, D>(sm.t.y + (tid + (S >> 1)) * D, q);
          for (int i = 0; i < D; ++i) {
            a[i] -= q[i];
            for (int j = 0; j < D; ++j) A[i][j] -= Q[i][j];
          }
        }
        if (wave_levels::parking_slot(tid, L) >= 0) {
          set_zero<double, D>(P);
          set_zero<double, D>(p);
        } else {                                  // the share of the row left of the tile, as the record would take it
          for (int i = 0; i < D; ++i) {
            p[i] = sm.xch[D * D + i];
            for (int j = 0; j < D; ++j) P[i][j] = (i >= j) ? sm.xch[i * D + j] : sm.xch[j * D + i];
          }
          if (form == 0)
            for (int l = 0; l < L; ++l) {
              double Q[D][D], q[D];
              LT::load_blk(sm.t.R, (1 << l) - 1, Q);
              load_vec<double, D>(sm.t.y + ((1 << l) - 1) * D, q);
              for (int i = 0; i < D; ++i) {
                p[i] -= q[i];
                for (int j = 0; j < D; ++j) P[i][j] -= Q[i][j];
              }
            }
        }
        // the staged form's state goes to memory, the in-register form's is compared with it
        auto emit = [&](int idx, double v) {
          double* q = snap + (size_t)tid * (3 * D * D + 2 * D) + idx;
          if (form == 0) { *q = v; return; }
          const double ref = fabs(*q), rel = fabs(v - *q) / (ref >= 1e-3 ? ref : 1e-3);
          worst = (rel > worst || rel != rel) ? rel : worst;
        };
        for (int i = 0; i < D; ++i) {
          emit(3 * D * D + i, a[i]);
          emit(3 * D * D + D + i, p[i]);
          for (int j = 0; j < D; ++j) {
            emit(i * D + j, A[i][j]);
            emit(D * D + i * D + j, B[i][j]);
            emit(2 * D * D + i * D + j, P[i][j]);
          }
        }
      }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const double o = __shfl_down(worst, off, 64);
    worst = (o > worst || o != o) ? o : worst;
  }
  if ((tid & 63) == 0) diff[tid >> 6] = worst;
  for (int form = 0; form < 2; ++form) {
    __syncthreads();
    double m = mahs[form], g = logs[form];
    block_sum2<NTHR>(m, g, sm.red);
    if (tid == 0) { ticks[form] = acc[form]; sums[2 * form] = m; sums[2 * form + 1] = g; }
  }
}

template <int L, int NTHR>
static void run_wave_levels(hipStream_t st) {
  const size_t lds = stage_lds_bytes<double, 4>(256, NTHR);
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&wave_levels_bench_kernel<L, NTHR>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  long long* ticks;
  double *diff, *sums, *snap;
  CK(hipMalloc(&snap, 256 * 56 * sizeof(double)));
  CK(hipMalloc(&ticks, 2 * sizeof(long long)));
  CK(hipMalloc(&diff, 8 * sizeof(double)));
  CK(hipMalloc(&sums, 4 * sizeof(double)));
  const int reps = 200;
  for (int pass = 0; pass < 2; ++pass)        // the second launch is the one reported
    hipLaunchKernelGGL((wave_levels_bench_kernel<L, NTHR>), dim3(1), dim3(NTHR), lds, st, reps, ticks, diff, sums, snap);
  CK(hipStreamSynchronize(st));
  long long t[2];
  double d[8], s[4], worst = 0.0;
  CK(hipMemcpy(t, ticks, sizeof(t), hipMemcpyDeviceToHost));
  CK(hipMemcpy(d, diff, sizeof(d), hipMemcpyDeviceToHost));
  CK(hipMemcpy(s, sums, sizeof(s), hipMemcpyDeviceToHost));
  for (int w = 0; w < NTHR / 64; ++w) worst = (d[w] > worst || d[w] != d[w]) ? d[w] : worst;
  printf("first %d levels of a full 256-row tile, %d threads: staged + quad levels %6.0f ns | in registers + hand-over %6.0f ns"
         "  (per level %.0f ns)  largest relative difference of the LDS state %.3g  [sums %.12g %.12g | %.12g %.12g]\n",
         L, NTHR, (double)t[0] / reps * 10.0, (double)t[1] / reps * 10.0, (double)t[1] / reps * 10.0 / L, worst, s[0], s[1], s[2], s[3]);
  CK(hipFree(ticks));
  CK(hipFree(diff));
  CK(hipFree(sums));
  CK(hipFree(snap));
}

// ---- one record stage alone: n records -> one record (or the two scalars), LDS form against register form ----
// One workgroup of 512 threads, as in the headline launch; the records are read with coherent loads every repetition
// (never from this CU's L1), the time is stamped by thread 0 around the stage.
template <bool REG, bool FINAL>
__global__ __launch_bounds__(512) void record_stage_bench_kernel(const double* rec, int n, int reps, double* rout, double* pout,
                                                                 const double* pin, int n_partial, double* out2, int* info,
                                                                 long long* ticks) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  using RL = RecordLayout<double, 4>;
  long long acc = 0;
  for (int rep = 0; rep < reps; ++rep) {
    __syncthreads();
    const long long t0 = wall_clock64();
    if constexpr (REG) {
      if (threadIdx.x < 64)
        record_stage_reg<true>((int)threadIdx.x, FINAL, rec, n, rout, pout, FINAL ? pin : nullptr, FINAL ? n_partial : 0, out2, info,
                                      0, 4096, (int64_t)n * 4096);
    } else {
      record_reduce_body<double, 4, (FINAL ? FOLD_MAX_GROUPS : FOLD_GROUP), 512, FINAL, true>(smem, 0u, rec, (int64_t)n, 1, rout, pout, FINAL ? pin : nullptr,
                                                                  FINAL ? (int64_t)n_partial : 0, out2, info, 4096,
                                                                  (int64_t)n * 4096, (int64_t)RL::STRIDE, (int64_t)PARTIAL_STRIDE);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const long long t1 = wall_clock64();
    acc += t1 - t0;
  }
  if (threadIdx.x == 0) ticks[0] = acc;
}

template <bool REG, bool FINAL>
static void run_record_stage(const double* rec, int n, double* rout, double* pout, const double* pin, int n_partial, double* out2,
                             int* info, long long* ticks, hipStream_t st) {
  using RL = RecordLayout<double, 4>;
  const size_t lds = stage_lds_bytes<double, 4>(FOLD_MAX_GROUPS, 512);
  const int reps = 200;
  for (int pass = 0; pass < 2; ++pass)        // the second launch is the one reported
    hipLaunchKernelGGL((record_stage_bench_kernel<REG, FINAL>), dim3(1), dim3(512), lds, st, rec, n, reps, rout, pout, pin, n_partial,
                       out2, info, ticks);
  CK(hipStreamSynchronize(st));
  long long t;
  CK(hipMemcpy(&t, ticks, sizeof(t), hipMemcpyDeviceToHost));
  double r[RL::STRIDE], p[4], o[2];
  int inf;
  CK(hipMemcpy(r, rout, sizeof(r), hipMemcpyDeviceToHost));
  CK(hipMemcpy(p, pout, sizeof(p), hipMemcpyDeviceToHost));
  CK(hipMemcpy(o, out2, sizeof(o), hipMemcpyDeviceToHost));
  CK(hipMemcpy(&inf, info, sizeof(inf), hipMemcpyDeviceToHost));
  double cs = 0;
  for (int i = 0; i < RL::STRIDE; ++i) cs += r[i] * (1 + i);
  if (FINAL)
    printf("  %-9s top stage   n=%2d (+%3d partial results): %6.0f ns   [out2 %.15g %.15g info %d]\n", REG ? "registers" : "LDS", n,
           n_partial, (double)t / reps * 10.0, o[0], o[1], inf);
  else
    printf("  %-9s group stage n=%2d: %6.0f ns   [record checksum %.15g partial %.15g %.15g %g]\n", REG ? "registers" : "LDS", n,
           (double)t / reps * 10.0, cs, p[0], p[1], p[2]);
}

static void run_record_stages(hipStream_t st) {
  using RL = RecordLayout<double, 4>;
  constexpr int NREC = 16, NPART = 272;
  std::vector<double> h((size_t)NREC * RL::STRIDE), hp((size_t)NPART * PARTIAL_STRIDE, 0.0);
  unsigned s = 12345u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double)((s >> 8) & 0xffff) / 65536.0 - 0.5; };
  for (int w = 0; w < NREC; ++w) {
    double* r = h.data() + (size_t)w * RL::STRIDE;
    for (int a = 0; a < 4; ++a)
      for (int b = 0; b <= a; ++b) {
        const double v = (a == b) ? 2.5 + 0.2 * rnd() : 0.1 * rnd(), u = (a == b) ? -0.2 - 0.1 * rnd() : 0.02 * rnd();
        r[RL::RS + 4 * a + b] = r[RL::RS + 4 * b + a] = v;
        r[RL::DRA + 4 * a + b] = r[RL::DRA + 4 * b + a] = u;
      }
    for (int a = 0; a < 16; ++a) r[RL::CS + a] = 0.3 * rnd();
    for (int a = 0; a < 4; ++a) { r[RL::YS + a] = rnd(); r[RL::DYA + a] = 0.1 * rnd(); }
  }
  for (int i = 0; i < NPART; ++i) { hp[(size_t)i * PARTIAL_STRIDE] = 1.0 + rnd(); hp[(size_t)i * PARTIAL_STRIDE + 1] = 3.0 + rnd(); }
  double *rec, *rout, *pout, *pin, *out2;
  int* info;
  long long* ticks;
  CK(hipMalloc(&rec, h.size() * sizeof(double)));
  CK(hipMalloc(&rout, RL::STRIDE * sizeof(double)));
  CK(hipMalloc(&pout, 4 * sizeof(double)));
  CK(hipMalloc(&pin, hp.size() * sizeof(double)));
  CK(hipMalloc(&out2, 2 * sizeof(double)));
  CK(hipMalloc(&info, sizeof(int)));
  CK(hipMalloc(&ticks, sizeof(long long)));
  CK(hipMemcpy(rec, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
  CK(hipMemcpy(pin, hp.data(), hp.size() * sizeof(double), hipMemcpyHostToDevice));
  CK(hipMemset(rout, 0, RL::STRIDE * sizeof(double)));
  CK(hipMemset(pout, 0, 4 * sizeof(double)));
  CK(hipMemset(out2, 0, 2 * sizeof(double)));
  CK(hipMemset(info, 0, sizeof(int)));
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&record_stage_bench_kernel<false, false>),
                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)stage_lds_bytes<double, 4>(FOLD_MAX_GROUPS, 512)));
  CK(hipFuncSetAttribute(reinterpret_cast<const void*>(&record_stage_bench_kernel<false, true>),
                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)stage_lds_bytes<double, 4>(FOLD_MAX_GROUPS, 512)));
  printf("one record stage, one workgroup of 512 threads, mean of 200 repetitions inside one launch\n");
  for (int n : {16, 9, 2}) {
    run_record_stage<false, false>(rec, n, rout, pout, pin, NPART, out2, info, ticks, st);
    run_record_stage<true, false>(rec, n, rout, pout, pin, NPART, out2, info, ticks, st);
    run_record_stage<false, true>(rec, n, rout, pout, pin, NPART, out2, info, ticks, st);
    run_record_stage<true, true>(rec, n, rout, pout, pin, NPART, out2, info, ticks, st);
  }
}

template <typename F>
float time_ms(F&& launch, int reps, hipStream_t st) {
  hipEvent_t a, b;
  CK(hipEventCreate(&a));
  CK(hipEventCreate(&b));
  launch();
  CK(hipStreamSynchronize(st));
  CK(hipEventRecord(a, st));
  for (int i = 0; i < reps; ++i) launch();
  CK(hipEventRecord(b, st));
  CK(hipEventSynchronize(b));
  float ms = 0;
  CK(hipEventElapsedTime(&ms, a, b));
  CK(hipGetLastError());
  return ms / reps;
}

template <typename T, int D, int C, int NT>
void run_chunk_variants(const T* R, const T* O, const T* y, int64_t N, double* out, hipStream_t st, double bytes) {
  const int64_t tiles = (N + (int64_t)C * NT - 1) / ((int64_t)C * NT);
  float a = time_ms([&] { hipLaunchKernelGGL((loads_only_kernel<T, D, C, NT>), dim3((unsigned)tiles), dim3(NT), 0, st, R, O, y, N, out); }, 20, st);
  float b = time_ms([&] { hipLaunchKernelGGL((chunk_only_kernel<T, D, C, NT>), dim3((unsigned)tiles), dim3(NT), 0, st, R, O, y, N, out); }, 20, st);
  printf("C=%2d NT=%3d tiles=%6lld : loads-only %7.2f us (%5.2f TB/s)   chunk-only %7.2f us (%5.2f TB/s)\n", C, NT,
         (long long)tiles, a * 1e3, bytes / (a * 1e-3) / 1e12, b * 1e3, bytes / (b * 1e-3) / 1e12);
}

int main(int argc, char** argv) {
  using T = double;
  constexpr int D = DEVB_D;
  const int lg = argc > 1 ? atoi(argv[1]) : 20;
  const int64_t N = (int64_t)1 << lg;
  if (argc > 2 && atoi(argv[2]) == 2) {           // dev_bench 20 2: stamps inside the final reduction of the real pipeline
    hipStream_t s2;
    CK(hipStreamCreate(&s2));
    T *R2, *O2, *y2;
    CK(hipMalloc(&R2, N * D * D * sizeof(T)));
    CK(hipMalloc(&O2, N * D * D * sizeof(T)));
    CK(hipMalloc(&y2, N * D * sizeof(T)));
    hipLaunchKernelGGL((gen_kernel<T, D>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s2, R2, O2, y2, N);
    const size_t wsb = cgps_host::tile_ws(N, D, sizeof(T)).total;
    char* ws;
    double* out2;
    int* info;
    CK(hipMalloc(&ws, wsb));
    CK(hipMalloc(&out2, 16));
    CK(hipMalloc(&info, 4));
    for (int mode = (argc > 3 ? atoi(argv[3]) : 0); mode < 2; ++mode) {     // dev_bench 20 2 <0: two launches | 1: folded>
      setenv("CGPS_NO_FOLD", mode == 0 ? "1" : "0", 1);
      for (int it = 0; it < 30; ++it) {
        hipEvent_t ea, eb;
        CK(hipEventCreate(&ea));
        CK(hipEventCreate(&eb));
        CK(hipEventRecord(ea, s2));
        int rc = run_tile_mahal_logdet<T, D>(R2, O2, y2, N, ws, wsb, out2, info, s2);
        CK(hipEventRecord(eb, s2));
        CK(hipStreamSynchronize(s2));
        float ms;
        CK(hipEventElapsedTime(&ms, ea, eb));
        long long st[16];
        CK(hipMemcpyFromSymbol(st, HIP_SYMBOL(g_fin_stamps), sizeof(st)));
        double o[2];
        CK(hipMemcpy(o, out2, 16, hipMemcpyDeviceToHost));
        if (it >= 28) {
          static long long ks[512][12];
          CK(hipMemcpyFromSymbol(ks, HIP_SYMBOL(g_k_stamps), sizeof(ks)));
          long long t0 = ks[0][0];
          for (int b = 0; b < 256; ++b) t0 = ks[b][0] < t0 ? ks[b][0] : t0;
          static int xcc[512];
          CK(hipMemcpyFromSymbol(xcc, HIP_SYMBOL(g_k_xcc), sizeof(xcc)));
          double sx[8] = {0}, mx[8] = {0};
          int cx[8] = {0};
          for (int b = 0; b < 256; ++b) {
            const int x = xcc[b] & 7;
            const double d = (ks[b][1] - t0) * 0.01;
            sx[x] += d; cx[x]++; mx[x] = d > mx[x] ? d : mx[x];
          }
          printf("   stream end per XCD (avg/max us):");
          for (int x = 0; x < 8; ++x) printf(" [%d: n=%d %.1f/%.1f]", x, cx[x], cx[x] ? sx[x] / cx[x] : 0.0, mx[x]);
          printf("\n   stream end by block index (us):");
          for (int b = 0; b < 256; b += 17) printf(" b%d:%.1f", b, (ks[b][1] - t0) * 0.01);
          printf("\n");
          const char* names[11] = {"start", "streamed", "tile reduced+emitted", "partial written", "arrived(group)",
                                   "group reduced", "arrived(top)", "final done", "rows staged in LDS", "tile_cr done",
                                   "in-register levels"};
          const int order[11] = {0, 1, 10, 8, 9, 2, 3, 4, 5, 6, 7};   // in the order a workgroup passes them
          for (int ki = 0; ki < 11; ++ki) {
            const int k = order[ki];
            long long lo = 1LL << 62, hi = 0;
            int cnt = 0;
            for (int b = 0; b < 256; ++b) {
              if (ks[b][k] < t0) continue;            // not reached in this launch
              lo = ks[b][k] < lo ? ks[b][k] : lo;
              hi = ks[b][k] > hi ? ks[b][k] : hi;
              ++cnt;
            }
            if (cnt) printf("   %-22s first %.2f us  last %.2f us  (%d workgroups)\n", names[k], (lo - t0) * 0.01, (hi - t0) * 0.01, cnt);
          }
        }
        if (it >= 27)
          printf("mode %s rc %d: op %.1f us | final: loads %.2f  lds-stores %.2f  reduce %.2f  last-row %.2f  sums+write %.2f  total %.2f us  [%.10g %.10g]\n",
                 mode == 0 ? "two launches" : "folded", rc, ms * 1e3, (st[1] - st[0]) * 0.01, (st[2] - st[1]) * 0.01,
                 (st[3] - st[2]) * 0.01, (st[4] - st[3]) * 0.01, (st[5] - st[4]) * 0.01, (st[5] - st[0]) * 0.01, o[0], o[1]);
      }
      break;   // fold_final_enabled() latches the environment at first use: one mode per process
    }
    return 0;
  }
  if (argc > 2 && atoi(argv[2]) == 3) {           // dev_bench 20 3: one record stage alone, LDS form against register form
    hipStream_t s3;
    CK(hipStreamCreate(&s3));
    run_record_stages(s3);
    return 0;
  }
  if (argc > 2 && atoi(argv[2]) == 4) {           // dev_bench 20 4: a full tile's first levels, staged against in registers
    hipStream_t s4;
    CK(hipStreamCreate(&s4));
    run_wave_levels<1, 512>(s4);
    run_wave_levels<2, 512>(s4);
    run_wave_levels<3, 512>(s4);
    run_wave_levels<4, 512>(s4);
    run_wave_levels<2, 256>(s4);
    run_wave_levels<3, 256>(s4);
    run_wave_levels<4, 256>(s4);
    return 0;
  }
  if (argc > 2 && atoi(argv[2]) == 1) {           // dev_bench 20 1: only the in-LDS reduction timings
    hipStream_t s2;
    CK(hipStreamCreate(&s2));
    for (int grid : {1, 256}) {
      run_tilecr<256, 1>(grid, s2);
      run_tilecr<256, 2>(grid, s2);
      run_tilecr<256, 4>(grid, s2);
      run_tilecr<512, 1>(grid, s2);
      run_tilecr<512, 2>(grid, s2);
      run_tilecr<512, 4>(grid, s2);
    }
    return 0;
  }
  hipStream_t st;
  CK(hipStreamCreate(&st));
  T *R, *O, *y;
  double* out;
  CK(hipMalloc(&R, N * D * D * sizeof(T)));
  CK(hipMalloc(&O, N * D * D * sizeof(T)));
  CK(hipMalloc(&y, N * D * sizeof(T)));
  CK(hipMalloc(&out, 4096));
  hipLaunchKernelGGL((gen_kernel<T, D>), dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, R, O, y, N);
  CK(hipStreamSynchronize(st));
  const double bytes = ((2.0 * N - 1) * D * D + N * D) * sizeof(T);
  printf("N=2^%d d=%d fp64  algorithmic bytes %.1f MB\n", lg, D, bytes / 1e6);
  run_mfma_probe();

  {  // coalesced streaming read of R and O back to back (ceiling for read-only streaming)
    const int64_t n16 = N * D * D * sizeof(T) / 16;
    float ms = time_ms([&] {
      hipLaunchKernelGGL(coalesced_read_kernel, dim3(2048), dim3(256), 0, st, (const double2*)R, n16, out);
      hipLaunchKernelGGL(coalesced_read_kernel, dim3(2048), dim3(256), 0, st, (const double2*)O, n16, out);
    }, 20, st);
    printf("coalesced read of R+O (2 launches): %7.2f us  (%5.2f TB/s)\n", ms * 1e3, 2.0 * n16 * 16 / (ms * 1e-3) / 1e12);
  }
  run_chunk_variants<T, D, 4, 256>(R, O, y, N, out, st, bytes);
  run_chunk_variants<T, D, 8, 256>(R, O, y, N, out, st, bytes);
  run_chunk_variants<T, D, 16, 256>(R, O, y, N, out, st, bytes);
  run_chunk_variants<T, D, 8, 128>(R, O, y, N, out, st, bytes);
  run_chunk_variants<T, D, 8, 64>(R, O, y, N, out, st, bytes);
  run_chunk_variants<T, D, 16, 64>(R, O, y, N, out, st, bytes);
  run_chunk_variants<T, D, 32, 64>(R, O, y, N, out, st, bytes);

  return 0;
}
