// Operand assembly for LEG models (the step BEFORE the cyclic reduction):
// diagonal and lower off-diagonal blocks of the PEG prior precision from the time stamps and the
// d x d generator G (reference models.py:181-239, restated):
//     E_i  = exp(-1/2 (t_{i+1} - t_i) G)
//     a_i  = (I - E_i^T E_i)^-1 E_i^T,     b_i = (I - E_i E_i^T)^-1 E_i
// evaluated through F_i = E_i - I (mat_expm1, gap_gram), so that a gap far below the length scale 1 / |G| keeps its
// precision: I - E E^T is of size gap |G| and is never formed from two matrices of size 1.
//     Rs_i = I + E_i^T b_i + E_{i-1} a_{i-1},     Os_i = -b_i                     (J[i+1, i] = Os_i)
// Embarrassingly parallel over the time axis: one lane per block row, everything in registers.
// A lane evaluates its own gap (i) and the gap before it (i-1), so no lane waits for a neighbour
// and the result does not depend on the launch geometry.
//
// exp(A): scaling and squaring around a Taylor polynomial in Horner form (degree 13 in fp64, 8 in fp32: with ||A||_1
// <= 1/2 the remainder 0.5^(m+1) / (m+1)! is 7e-16 / 5e-9, below the rounding of the format; rounds 1 and 2 ran
// degree 18 in both, the degree torch.matrix_exp uses in fp64 for norms up to 5.4), ||A||_1 scaled below 1/2; the
// two d x d systems are symmetric positive definite (||E||_2 < 1 because G + G^T is positive
// definite) and go through the Cholesky routines of cgps_math.h.  A gap of zero length makes them
// singular: reported through `info` (1 + row index), like a non-positive-definite block elsewhere.
#pragma once
#include "cgps_math.h"

namespace cgps {

constexpr int LEG_THREADS = 64;

template <typename T, int D>
__device__ __forceinline__ void mat_mul(T (&C)[D][D], const T (&A)[D][D], const T (&B)[D][D]) {
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      T s = T(0);
#pragma unroll
      for (int m = 0; m < D; ++m) s = fmaT(A[i][m], B[m][j], s);
      C[i][j] = s;
    }
}

template <typename T> constexpr int exp_taylor_degree() { return sizeof(T) == 8 ? 13 : 8; }

// E = exp(A); A is destroyed
template <typename T, int D>
__device__ __forceinline__ void mat_exp(T (&E)[D][D], T (&A)[D][D]) {
  T nrm = T(0);
#pragma unroll
  for (int j = 0; j < D; ++j) {
    T c = T(0);
#pragma unroll
    for (int i = 0; i < D; ++i) c += A[i][j] < T(0) ? -A[i][j] : A[i][j];
    nrm = c > nrm ? c : nrm;
  }
  int s = 0;
  T scale = T(1);
  while (nrm * scale > T(0.5) && s < 60) { scale *= T(0.5); ++s; }
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) A[i][j] *= scale;
  // Horner: E = I + A (I + A/2 (I + A/3 (...)))
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) E[i][j] = (i == j) ? T(1) : T(0);
#pragma unroll 1
  for (int k = exp_taylor_degree<T>(); k >= 1; --k) {
    T P[D][D];
    mat_mul<T, D>(P, A, E);
    const T rk = T(1) / T(k);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) E[i][j] = ((i == j) ? T(1) : T(0)) + P[i][j] * rk;
  }
#pragma unroll 1
  for (int q = 0; q < s; ++q) {
    T P[D][D];
    mat_mul<T, D>(P, E, E);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) E[i][j] = P[i][j];
  }
}

// F = exp(A) - I without forming exp(A); A is destroyed.  For a short gap exp(A) is I plus something of the size of A,
// and everything downstream wants that something to full relative precision (gap_gram).  The scaled series is summed
// without its leading I,  F = A (I + A/2 (I + A/3 (...))),  and a squaring  E <- E E  reads  F <- 2 F + F F:  no step
// adds a matrix of size 1 to one of size |A|.  At long gaps F tends to -I and an absolute error of a few eps is all
// that the blocks ask for (exp(A) itself is then far below 1 and so is what it contributes).
template <typename T, int D>
__device__ __forceinline__ void mat_expm1(T (&F)[D][D], T (&A)[D][D]) {
  T nrm = T(0);
#pragma unroll
  for (int j = 0; j < D; ++j) {
    T c = T(0);
#pragma unroll
    for (int i = 0; i < D; ++i) c += A[i][j] < T(0) ? -A[i][j] : A[i][j];
    nrm = c > nrm ? c : nrm;
  }
  int s = 0;
  T scale = T(1);
  while (nrm * scale > T(0.5) && s < 60) { scale *= T(0.5); ++s; }
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      A[i][j] *= scale;
      F[i][j] = (i == j) ? T(1) : T(0);
    }
#pragma unroll 1
  for (int k = exp_taylor_degree<T>(); k >= 2; --k) {
    T P[D][D];
    mat_mul<T, D>(P, A, F);
    const T rk = T(1) / T(k);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) F[i][j] = ((i == j) ? T(1) : T(0)) + P[i][j] * rk;
  }
  {
    T P[D][D];
    mat_mul<T, D>(P, A, F);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) F[i][j] = P[i][j];
  }
#pragma unroll 1
  for (int q = 0; q < s; ++q) {
    T P[D][D];
    mat_mul<T, D>(P, F, F);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) F[i][j] = fmaT(T(2), F[i][j], P[i][j]);
  }
}

// F = exp(-1/2 dt G) - I of one time gap: the one place every assembly (unfused, fused, batched, adjoint) gets it from
template <typename T, int D, typename GT>
__device__ __forceinline__ void gap_expm1(T dt, const GT& G, T (&F)[D][D]) {
  T A[D][D];
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) A[i][j] = T(-0.5) * dt * G(i, j);
  mat_expm1<T, D>(F, A);
}

// M = I - E E^T (OUTER) or I - E^T E (!OUTER) for E = I + F, as -(F + F^T + F F^T) resp. -(F + F^T + F^T F): the
// reference's form subtracts two matrices of size 1 and keeps eps / (gap |G|) of relative precision; here the three
// terms are of the size of the result.
template <typename T, int D, bool OUTER>
__device__ __forceinline__ void gap_gram(const T (&F)[D][D], T (&M)[D][D]) {
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) {
      T s = F[i][j] + F[j][i];
#pragma unroll
      for (int m = 0; m < D; ++m) s = OUTER ? fmaT(F[i][m], F[j][m], s) : fmaT(F[m][i], F[m][j], s);
      M[i][j] = -s;
    }
}

// X = M^-1 B (TRANS: M^-1 B^T) for the symmetric M (lower triangle read); returns false when M is not positive definite
template <typename T, int D, bool TRANS = false>
__device__ __forceinline__ bool spd_solve(const T (&M)[D][D], const T (&B)[D][D], T (&X)[D][D]) {
  Chol<T, D> c;
  bool f = false;
  chol_lower<T, D>(M, c, f);
#pragma unroll
  for (int j = 0; j < D; ++j) {
    T v[D];
#pragma unroll
    for (int i = 0; i < D; ++i) v[i] = TRANS ? B[j][i] : B[i][j];
    fwd_subst<T, D>(c, v);
    bwd_subst<T, D>(c, v);
#pragma unroll
    for (int i = 0; i < D; ++i) X[i][j] = v[i];
  }
  return !f;
}

// X = (I - S)^-1 B for the symmetric S (lower triangle read); returns false when I - S is not
// positive definite.  Only for an S that is not close to I (the prediction glue below); a time gap goes through gap_gram.
template <typename T, int D>
__device__ __forceinline__ bool spd_solve_i_minus(const T (&S)[D][D], const T (&B)[D][D], T (&X)[D][D]) {
  T M[D][D];
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) M[i][j] = ((i == j) ? T(1) : T(0)) - S[i][j];
  return spd_solve<T, D>(M, B, X);
}

template <typename T, int D>
__device__ __forceinline__ void add_identity(T (&E)[D][D]) {
#pragma unroll
  for (int i = 0; i < D; ++i) E[i][i] += T(1);
}

// the two contributions of one time gap: toRight = E a (goes to the row after the gap),
// toLeft = E^T b (to the row before it), b itself (the coupling is -b)
template <typename T, int D>
__device__ __forceinline__ bool gap_terms(T dt, const T (&G)[D][D], bool want_right, bool want_left, T (&toRight)[D][D],
                                          T (&toLeft)[D][D], T (&b)[D][D]) {
  T E[D][D], Ma[D][D], Mb[D][D];
  gap_expm1<T, D>(dt, [&](int i, int j) { return G[i][j]; }, E);       // F
  if (want_right) gap_gram<T, D, false>(E, Ma);
  if (want_left) gap_gram<T, D, true>(E, Mb);
  add_identity<T, D>(E);                                               // E = I + F
  bool ok = true;
  if (want_right) {
    T a[D][D];
    ok = spd_solve<T, D, true>(Ma, E, a) && ok;    // a = (I - E^T E)^-1 E^T
    mat_mul<T, D>(toRight, E, a);
  }
  if (want_left) {
    ok = spd_solve<T, D>(Mb, E, b) && ok;          // b = (I - E E^T)^-1 E
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) {
        T s = T(0);
#pragma unroll
        for (int m = 0; m < D; ++m) s = fmaT(E[m][i], b[m][j], s);
        toLeft[i][j] = s;
      }
  }
  return ok;
}

// cut (nullptr: one series): cut[g] != 0 marks the gap between rows g and g+1 as the boundary between two
// independent series (cgps_peg_precision_seg).  Such a gap is never evaluated -- it may be zero or negative --
// its coupling block is 0 and it adds nothing to either diagonal block; with cut == nullptr the arithmetic is
// the one-series kernel's, unchanged.
//
// TERM (cgps_leg_posterior_blocks_seg): a row's diagonal term of the POSTERIOR precision, added to the finished PEG
// block as the last operation before its store, so that K's diagonal is written once instead of Rs being written, read,
// added to and written again.  PEG_TERM_NONE: nothing (the two assembly entry points: none of the three arguments is
// read, and every difference below is an `if constexpr`).  PEG_TERM_PLAIN: the one block term[d][d].  PEG_TERM_TABLE:
// entry rows[i] (a byte) of term[entries][d][d], the index clamped to entries - 1 as leg_obs_block clamps it.
// PEG_TERM_WEIGHTED: sum_k w[i][k] term[k] with w = rows as T[N][entries], summed over k in registers and added once.
//
// MODELS (cgps_peg_precision_models): the same N rows under gridDim.y generators.  blockIdx.y = k names the model: the
// workgroup moves G, Rs and Os to model k's slices (G[M][d][d], rows k N .. (k+1) N - 1 of the concatenated Rs / Os) and
// is the one-model workgroup from there on; ts and cut are every model's.  The last row of a model that is not the last
// also writes the zero coupling block between two models, Os[(k+1) N - 1]; failures report the concatenated row.
//
// MODELS with a TERM (cgps_leg_posterior_blocks_models): the term is per model as well -- term[M][d][d] (PLAIN),
// term[M][entries][d][d] (TABLE, WEIGHTED) and the weights w[M][N][entries] -- and the workgroup moves to model k's slices
// of those too; the pattern bytes of the table source belong to the data and stay every model's.
constexpr int PEG_TERM_NONE = 0, PEG_TERM_PLAIN = 1, PEG_TERM_TABLE = 2, PEG_TERM_WEIGHTED = 3;

// the block sizes of cgps_leg_loglik_models, whose backward the models forms of the assembly serve
template <typename T, int D>
constexpr bool peg_models_supported() { return D <= 7 && !(D == 6 && sizeof(T) == 8); }

template <typename T, int D, int TERM = PEG_TERM_NONE, bool MODELS = false>
__global__ __launch_bounds__(LEG_THREADS) void peg_precision_kernel(const T* __restrict__ ts, const T* __restrict__ Gg,
                                                                    int64_t N, T* __restrict__ Rs, T* __restrict__ Os,
                                                                    int* __restrict__ info,
                                                                    const unsigned char* __restrict__ cut = nullptr,
                                                                    const T* __restrict__ term = nullptr,
                                                                    const void* __restrict__ rows = nullptr,
                                                                    int entries = 0) {
  constexpr int DD = D * D;
  const int64_t i = (int64_t)blockIdx.x * LEG_THREADS + threadIdx.x;
  if (i >= N) return;
  if constexpr (MODELS) {
    const int64_t k = blockIdx.y;
    Gg += k * DD;
    Rs += k * N * DD;
    Os += k * N * DD;
    if constexpr (TERM == PEG_TERM_PLAIN) term += k * DD;                              // term[M][d][d]
    else if constexpr (TERM != PEG_TERM_NONE) term += k * (int64_t)entries * DD;       // term[M][entries][d][d]
  }
  T G[D][D];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) G[a][b] = Gg[a * D + b];
  T R[D][D];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) R[a][b] = (a == b) ? T(1) : T(0);
  bool ok = true;
  if (i + 1 < N && cut != nullptr && cut[i]) {    // the gap after this row ends a series: no coupling
    T z[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) z[a][b] = T(0);
    store_block<T, D>(Os + i * DD, z);
  } else if (i + 1 < N) {                          // the gap after this row
    T c1[D][D], c2[D][D], bb[D][D];
    ok = gap_terms<T, D>(ts[i + 1] - ts[i], G, false, true, c1, c2, bb) && ok;
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) { R[a][b] += c2[a][b]; bb[a][b] = -bb[a][b]; }
    store_block<T, D>(Os + i * DD, bb);
  } else if constexpr (MODELS) {                   // a model's last row: the next model does not couple to it
    if (blockIdx.y + 1 < gridDim.y) {
      T z[D][D];
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) z[a][b] = T(0);
      store_block<T, D>(Os + i * DD, z);
    }
  }
  if (i >= 1 && !(cut != nullptr && cut[i - 1])) { // the gap before it (unless it starts a series)
    T c1[D][D], c2[D][D], bb[D][D];
    ok = gap_terms<T, D>(ts[i] - ts[i - 1], G, true, false, c1, c2, bb) && ok;
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) R[a][b] += c1[a][b];
  }
  if constexpr (TERM == PEG_TERM_PLAIN || TERM == PEG_TERM_TABLE) {
    const T* __restrict__ tb = term;
    if constexpr (TERM == PEG_TERM_TABLE) {
      const int p = (int)static_cast<const unsigned char*>(rows)[i];
      tb = term + (size_t)(p < entries - 1 ? p : entries - 1) * DD;
    }
    T A[D][D];
    load_block<T, D>(tb, A);
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) R[a][b] += A[a][b];
  } else if constexpr (TERM == PEG_TERM_WEIGHTED) {
    int64_t wi = i;
    if constexpr (MODELS) wi += (int64_t)blockIdx.y * N;                               // w[M][N][entries]
    const T* __restrict__ w = static_cast<const T*>(rows) + wi * (int64_t)entries;
    T S[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) S[a][b] = T(0);
#pragma unroll 1
    for (int k = 0; k < entries; ++k) {
      const T wk = w[k];
      const T* __restrict__ bk = term + (size_t)k * DD;
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) S[a][b] = fmaT(wk, bk[a * D + b], S[a][b]);
    }
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) R[a][b] += S[a][b];
  }
  store_block<T, D>(Rs + i * DD, R);
  if constexpr (MODELS) {
    if (!ok) report_fail(info, (int64_t)blockIdx.y * N + i);
  } else {
    if (!ok) report_fail(info, i);
  }
}


// ---- prediction glue (the step AFTER the cyclic reduction) ----------------------------
// Posterior of the latent at arbitrary target times from the in-sample posterior (mean[n][d], diagonal
// covariance blocks P[n][d][d], lower off-diagonal blocks C[n-1][d][d] = Cov(z_{i+1}, z_i)): the
// reference walks the targets in a Python loop (intercast, models.py:455-514: searchsorted, one or two
// matrix exponentials, one gaussian_stitch of a 2d x 2d or 3d x 3d Gaussian, model_utils.py:64-107).
// Here one lane per target, everything in registers, and the stitches reduced to d x d algebra:
//   forecast from a neighbour with posterior N(mu, P) over a gap with E = exp(-1/2 gap G)
//   (E transposed when the target lies BEFORE the first observation):
//       mean = E mu,   cov = I - E E^T + E P E^T
//   interpolation between neighbours j-1 (mu0, P0) and j (mu1, P1), C = Cov(z_j, z_j-1),
//   E1 = exp(-1/2 (t - t_j-1) G), E2 = exp(-1/2 (t_j - t) G), E3 = E1 E2: the prior of
//   (z_j-1, z_j) has covariance [[I, E3^T], [E3, I]], whose inverse through the Schur complement
//   S = I - E3 E3^T (symmetric positive definite) gives the 2d-wide mean transformer as two d x d blocks
//       W = (E2^T - E1 E3^T) S^-1,   Ma = E1 - W E3,   Mb = W
//       mean = Ma mu0 + Mb mu1
//       cov  = I - (Ma E1^T + Mb E2) + Ma P0 Ma^T + Ma C^T Mb^T + Mb C Ma^T + Mb P1 Mb^T
// Branches as the reference takes them: t before the first / after the last observation -> forecast;
// t at the first / last observation (torch.allclose defaults: |a - b| <= 1e-8 + 1e-5 |b|) -> the
// in-sample values; otherwise interpolation between searchsorted's neighbours.
template <typename T, int D>
__device__ __forceinline__ void leg_forecast(const T (&E)[D][D], const T* __restrict__ mu, const T* __restrict__ Pg,
                                             T (&mean)[D], T (&cov)[D][D]) {
  T P[D][D], EP[D][D];
  load_block<T, D>(Pg, P);
  mat_mul<T, D>(EP, E, P);
#pragma unroll
  for (int i = 0; i < D; ++i) {
    T s = T(0);
#pragma unroll
    for (int m = 0; m < D; ++m) s = fmaT(E[i][m], mu[m], s);
    mean[i] = s;
#pragma unroll
    for (int j = 0; j < D; ++j) {
      T c = (i == j) ? T(1) : T(0);
#pragma unroll
      for (int m = 0; m < D; ++m) c = fmaT(EP[i][m] - E[i][m], E[j][m], c);   // + (E P - E) E^T
      cov[i][j] = c;
    }
  }
}

// One target of one series: ts[n] the series' own time stamps, mu[n][d], Pd[n][d][d], Co[n-1][d][d] its own posterior,
// t the target.  Reads rows 0 .. n-1 and off-diagonal blocks 0 .. n-2 of what it is handed and nothing else, so a caller
// that hands it a slice of a concatenated batch (leg_intercast_seg_kernel) never touches a neighbouring series.
template <typename T, int D>
__device__ __forceinline__ void leg_intercast_target(const T* __restrict__ ts, int64_t n, const T* __restrict__ Gg,
                                                     const T* __restrict__ mu, const T* __restrict__ Pd,
                                                     const T* __restrict__ Co, const T t, T* __restrict__ out_mean,
                                                     T* __restrict__ out_cov) {
  constexpr int DD = D * D;
  int64_t lo = 0, hi = n;                          // first index with ts[idx] >= t (torch.searchsorted, right = False)
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (ts[mid] < t) lo = mid + 1; else hi = mid;
  }
  const int64_t idx = lo;
  auto close = [](T a, T b) {
    const T dlt = a > b ? a - b : b - a, ab = b < T(0) ? -b : b;
    return dlt <= T(1e-8) + T(1e-5) * ab;
  };
  const T t_first = ts[0], t_last = ts[n - 1];
  const bool at_first = idx == 0 && close(t, t_first);
  const bool at_last = idx > 0 && close(t, t_last);
  const bool back = idx == 0 && !at_first, fwd = idx == n && !at_last;
  // (every branch stores its own result: nothing of the d + d*d values is carried across the branches)
  if (at_first || at_last) {
    const int64_t r = at_first ? 0 : n - 1;
    T mean[D], cov[D][D];
    load_vec<T, D>(mu + r * D, mean);
    load_block<T, D>(Pd + r * DD, cov);
    store_vec<T, D>(out_mean, mean);
    store_block<T, D>(out_cov, cov);
  } else {
    T G[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) G[a][b] = Gg[a * D + b];
    auto exp_gap = [&](T gap, T (&E)[D][D]) {
      T A[D][D];
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) A[a][b] = T(-0.5) * gap * G[a][b];
      mat_exp<T, D>(E, A);
    };
    if (back || fwd) {
      T E[D][D];
      exp_gap(back ? t_first - t : t - t_last, E);
      if (back) {
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
          for (int b = a + 1; b < D; ++b) { const T v = E[a][b]; E[a][b] = E[b][a]; E[b][a] = v; }
      }
      const int64_t r = back ? 0 : n - 1;
      T m0[D], mean[D], cov[D][D];
      load_vec<T, D>(mu + r * D, m0);
      leg_forecast<T, D>(E, m0, Pd + r * DD, mean, cov);
      store_vec<T, D>(out_mean, mean);
      store_block<T, D>(out_cov, cov);
    } else {
      int64_t j = idx < 1 ? 1 : idx;
      if (j > n - 1) j = n - 1;
      T E1[D][D], E2[D][D], E3[D][D], W[D][D], Ma[D][D];
      exp_gap(t - ts[j - 1], E1);
      exp_gap(ts[j] - t, E2);
      mat_mul<T, D>(E3, E1, E2);
      {
        T S[D][D], Xt[D][D], Wt[D][D];
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
          for (int b = 0; b < D; ++b) {
            T s = T(0), x = E2[a][b];              // X^T[a][b] = X[b][a] = E2[a][b] - (E1 E3^T)[b][a]
#pragma unroll
            for (int m = 0; m < D; ++m) {
              s = fmaT(E3[a][m], E3[b][m], s);     // (E3 E3^T)[a][b]
              x = fmaT(-E1[b][m], E3[a][m], x);
            }
            S[a][b] = s;
            Xt[a][b] = x;
          }
        (void)spd_solve_i_minus<T, D>(S, Xt, Wt);  // W^T = S^-1 X^T
#pragma unroll
        for (int a = 0; a < D; ++a)
#pragma unroll
          for (int b = 0; b < D; ++b) W[a][b] = Wt[b][a];
      }
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) {
          T s = E1[a][b];
#pragma unroll
          for (int m = 0; m < D; ++m) s = fmaT(-W[a][m], E3[m][b], s);
          Ma[a][b] = s;
        }
      T m0[D], m1[D], mean[D], cov[D][D];
      load_vec<T, D>(mu + (j - 1) * D, m0);
      load_vec<T, D>(mu + j * D, m1);
#pragma unroll
      for (int a = 0; a < D; ++a) {
        T s = T(0);
#pragma unroll
        for (int m = 0; m < D; ++m) s = fmaT(Ma[a][m], m0[m], fmaT(W[a][m], m1[m], s));
        mean[a] = s;
      }
      // cov = I - (Ma E1^T + W E2) + (Ma P0 + W C) Ma^T + (Ma C^T + W P1) W^T
      T Q[D][D], U[D][D], V[D][D];
      load_block<T, D>(Pd + (j - 1) * DD, Q);      // P0
      mat_mul<T, D>(U, Ma, Q);
      load_block<T, D>(Co + (j - 1) * DD, Q);      // C
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) {
          T u = U[a][b], v = T(0);
#pragma unroll
          for (int m = 0; m < D; ++m) {
            u = fmaT(W[a][m], Q[m][b], u);         // + W C
            v = fmaT(Ma[a][m], Q[b][m], v);        // Ma C^T
          }
          U[a][b] = u;
          V[a][b] = v;
        }
      load_block<T, D>(Pd + j * DD, Q);            // P1
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) {
          T v = V[a][b];
#pragma unroll
          for (int m = 0; m < D; ++m) v = fmaT(W[a][m], Q[m][b], v);
          V[a][b] = v;
        }
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) {
          T c = (a == b) ? T(1) : T(0);
#pragma unroll
          for (int m = 0; m < D; ++m) {
            c = fmaT(-Ma[a][m], E1[b][m], c);      // - Ma E1^T
            c = fmaT(-W[a][m], E2[m][b], c);       // - W E2
            c = fmaT(U[a][m], Ma[b][m], c);        // + U Ma^T
            c = fmaT(V[a][m], W[b][m], c);         // + V W^T
          }
          cov[a][b] = c;
        }
      store_vec<T, D>(out_mean, mean);
      store_block<T, D>(out_cov, cov);
    }
  }
}

template <typename T, int D>
__global__ __launch_bounds__(LEG_THREADS) void leg_intercast_kernel(const T* __restrict__ ts, int64_t n,
                                                                    const T* __restrict__ tt, int64_t p,
                                                                    const T* __restrict__ Gg, const T* __restrict__ mu,
                                                                    const T* __restrict__ Pd, const T* __restrict__ Co,
                                                                    T* __restrict__ out_mean, T* __restrict__ out_cov) {
  const int64_t k = (int64_t)blockIdx.x * LEG_THREADS + threadIdx.x;
  if (k >= p) return;
  leg_intercast_target<T, D>(ts, n, Gg, mu, Pd, Co, tt[k], out_mean + k * D, out_cov + k * (D * D));
}

// The same for B series concatenated (cgps_leg_intercast_seg): series b is rows roff[b] .. roff[b+1]-1 of ts, mu, Pd
// (and of Co, whose entry at a series' last row is the cut gap and is never read), its targets are
// tt[toff[b] .. toff[b+1]-1].  One lane per target: it finds its series as the one b with toff[b] <= k < toff[b+1]
// (binary search; series without targets are stepped over), then works on that series' slices alone.
//
// MODELS (cgps_leg_intercast_models): the same rows and targets under gridDim.y models.  blockIdx.y names the model: the
// workgroup moves G, mu, Pd, Co (R = roff[B] rows per model; Co's entry between two models is a series' last and never
// read) and both outputs (p targets per model) to that model's slices and is the one-model workgroup from there on.
template <typename T, int D, bool MODELS = false>
__global__ __launch_bounds__(LEG_THREADS) void leg_intercast_seg_kernel(
    const T* __restrict__ ts, const int64_t* __restrict__ roff, const T* __restrict__ tt,
    const int64_t* __restrict__ toff, int64_t B, int64_t p, const T* __restrict__ Gg, const T* __restrict__ mu,
    const T* __restrict__ Pd, const T* __restrict__ Co, T* __restrict__ out_mean, T* __restrict__ out_cov) {
  constexpr int DD = D * D;
  const int64_t k = (int64_t)blockIdx.x * LEG_THREADS + threadIdx.x;
  if (k >= p) return;
  if constexpr (MODELS) {
    const int64_t m = blockIdx.y, R = roff[B];
    Gg += m * DD;
    mu += m * R * D;
    Pd += m * R * DD;
    Co += m * R * DD;
    out_mean += m * p * D;
    out_cov += m * p * DD;
  }
  int64_t lo = 0, hi = B;                          // first b with toff[b + 1] > k
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (toff[mid + 1] <= k) lo = mid + 1; else hi = mid;
  }
  if (lo >= B) return;                             // (offsets that do not cover p targets: nothing is written)
  const int64_t r0 = roff[lo], n = roff[lo + 1] - r0;
  if (n < 1) return;                               // (a series needs a row)
  leg_intercast_target<T, D>(ts + r0, n, Gg, mu + r0 * D, Pd + r0 * DD, Co + r0 * DD, tt[k], out_mean + k * D,
                             out_cov + k * DD);
}

// ---- adjoint of the assembly (training through the path, reference models.py:374-381) -----------------
// Given gRs[N] = d loss / d Rs and gOs[N-1] = d loss / d Os, one lane per time gap i recomputes the
// gap's E, a, b and walks the expressions above backwards:
//   c2 = E^T b -> Rs_i  (upstream U2 = gRs_i),  c1 = E a -> Rs_{i+1}  (U1 = gRs_{i+1}),  Os_i = -b
//   bbar = E U2 - gOs_i ;          W = (I - E E^T)^-1 bbar ;  Ebar  = b U2^T + W + (W b^T + b W^T) E
//   abar = E^T U1 ;                V = (I - E^T E)^-1 abar ;  Ebar += U1 a^T + V^T + E (a V^T + V a^T)
//   E = exp(A), A = -1/2 tau G:    Abar = L_exp(A^T, Ebar)    (the adjoint of the Frechet derivative of
//                                   exp at A is the Frechet derivative at A^T), by the same scaling and
//                                   squaring, carried for the pair (exp, derivative)
//   Gbar += -1/2 tau Abar ;        taubar = -1/2 <Abar, G>
// Gbar is summed over the lanes of a workgroup in a fixed order and written per workgroup
// (gG_partial[block][d][d]: the caller adds the few partial sums -- deterministic, no atomics);
// gtau[i] = d loss / d (t_{i+1} - t_i).  With a cut mask (see peg_precision_kernel) a gap between two series
// gets gtau = 0 and adds nothing to Gbar.

// (E, L) <- (exp(A), L_exp(A, dA)); A and dA are destroyed
template <typename T, int D>
__device__ __forceinline__ void mat_exp_frechet(T (&E)[D][D], T (&L)[D][D], T (&A)[D][D], T (&dA)[D][D]) {
  T nrm = T(0);
#pragma unroll
  for (int j = 0; j < D; ++j) {
    T c = T(0);
#pragma unroll
    for (int i = 0; i < D; ++i) c += A[i][j] < T(0) ? -A[i][j] : A[i][j];
    nrm = c > nrm ? c : nrm;
  }
  int s = 0;
  T scale = T(1);
  while (nrm * scale > T(0.5) && s < 60) { scale *= T(0.5); ++s; }
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) { A[i][j] *= scale; dA[i][j] *= scale; }
  // Horner for the pair: P = I + (A / k) P,  dP = (dA / k) P + (A / k) dP
#pragma unroll
  for (int i = 0; i < D; ++i)
#pragma unroll
    for (int j = 0; j < D; ++j) { E[i][j] = (i == j) ? T(1) : T(0); L[i][j] = T(0); }
#pragma unroll 1
  for (int k = exp_taylor_degree<T>(); k >= 1; --k) {
    T P[D][D], Q[D][D], R[D][D];
    mat_mul<T, D>(P, A, E);
    mat_mul<T, D>(Q, dA, E);
    mat_mul<T, D>(R, A, L);
    const T rk = T(1) / T(k);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) {
        E[i][j] = ((i == j) ? T(1) : T(0)) + P[i][j] * rk;
        L[i][j] = (Q[i][j] + R[i][j]) * rk;
      }
  }
#pragma unroll 1
  for (int q = 0; q < s; ++q) {                          // (E, L) <- (E E, E L + L E)
    T P[D][D], Q[D][D], R[D][D];
    mat_mul<T, D>(Q, E, L);
    mat_mul<T, D>(R, L, E);
    mat_mul<T, D>(P, E, E);
#pragma unroll
    for (int i = 0; i < D; ++i)
#pragma unroll
      for (int j = 0; j < D; ++j) { E[i][j] = P[i][j]; L[i][j] = Q[i][j] + R[i][j]; }
  }
}

// MODELS (cgps_peg_precision_adjoint_models): blockIdx.y names the model as in peg_precision_kernel; gG_partial and
// gtau are [M][gridDim.x][d][d] and [M][N - 1].  The gap after a model's last row belongs to no workgroup.
template <typename T, int D, bool MODELS = false>
__global__ __launch_bounds__(LEG_THREADS) void peg_precision_adjoint_kernel(
    const T* __restrict__ ts, const T* __restrict__ Gg, int64_t N, const T* __restrict__ gRs, const T* __restrict__ gOs,
    T* __restrict__ gG_partial, T* __restrict__ gtau, const unsigned char* __restrict__ cut = nullptr) {
  constexpr int DD = D * D;
  __shared__ T red[DD];
  const int64_t i = (int64_t)blockIdx.x * LEG_THREADS + threadIdx.x;      // the gap between rows i and i + 1
  if constexpr (MODELS) {
    const int64_t k = blockIdx.y;
    Gg += k * DD;
    gRs += k * N * DD;
    gOs += k * N * DD;
    gG_partial += k * (int64_t)gridDim.x * DD;
    if (gtau != nullptr) gtau += k * (N - 1);
  }
  T Gbar[D][D];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) Gbar[a][b] = T(0);
  if (i + 1 < N && cut != nullptr && cut[i]) {   // a gap between two series: evaluated nowhere, contributes nothing
    if (gtau != nullptr) gtau[i] = T(0);
  } else if (i + 1 < N) {
    T G[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) G[a][b] = Gg[a * D + b];
    const T tau = ts[i + 1] - ts[i];
    T E[D][D], Et[D][D], Mb[D][D], Ma[D][D];                 // Mb = I - E E^T, Ma = I - E^T E, both from F = E - I
    gap_expm1<T, D>(tau, [&](int a, int b) { return G[a][b]; }, E);
    gap_gram<T, D, true>(E, Mb);
    gap_gram<T, D, false>(E, Ma);
    add_identity<T, D>(E);
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) Et[a][b] = E[b][a];
    T Ebar[D][D];
    {   // through c2 = E^T b (to Rs_i) and Os_i = -b
      T bm[D][D], U2[D][D], gO[D][D], bbar[D][D], W[D][D], X[D][D], Y[D][D];
      (void)spd_solve<T, D>(Mb, E, bm);                        // b = (I - E E^T)^-1 E
      load_block<T, D>(gRs + i * DD, U2);
      load_block<T, D>(gOs + i * DD, gO);
      mat_mul<T, D>(bbar, E, U2);
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) bbar[a][b] -= gO[a][b];
      (void)spd_solve<T, D>(Mb, bbar, W);                      // W = (I - E E^T)^-1 bbar
      // Ebar = b U2^T + W + (W b^T + b W^T) E
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) {
          T s = T(0), z = W[a][b];
#pragma unroll
          for (int m = 0; m < D; ++m) {
            s = fmaT(W[a][m], bm[b][m], s);
            s = fmaT(bm[a][m], W[b][m], s);
            z = fmaT(bm[a][m], U2[b][m], z);
          }
          X[a][b] = s;
          Ebar[a][b] = z;
        }
      mat_mul<T, D>(Y, X, E);
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) Ebar[a][b] += Y[a][b];
    }
    {   // through c1 = E a (to Rs_{i+1})
      T am[D][D], U1[D][D], abar[D][D], V[D][D], X[D][D], Y[D][D];
      (void)spd_solve<T, D>(Ma, Et, am);                       // a = (I - E^T E)^-1 E^T
      load_block<T, D>(gRs + (i + 1) * DD, U1);
      mat_mul<T, D>(abar, Et, U1);
      (void)spd_solve<T, D>(Ma, abar, V);                      // V = (I - E^T E)^-1 abar
      // Ebar += U1 a^T + V^T + E (a V^T + V a^T)
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) {
          T s = T(0), z = V[b][a];
#pragma unroll
          for (int m = 0; m < D; ++m) {
            s = fmaT(am[a][m], V[b][m], s);
            s = fmaT(V[a][m], am[b][m], s);
            z = fmaT(U1[a][m], am[b][m], z);
          }
          X[a][b] = s;
          Ebar[a][b] += z;
        }
      mat_mul<T, D>(Y, E, X);
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int b = 0; b < D; ++b) Ebar[a][b] += Y[a][b];
    }
    // Abar = L_exp(A^T, Ebar)
    T At[D][D], Ex[D][D], Abar[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) At[a][b] = T(-0.5) * tau * G[b][a];
    mat_exp_frechet<T, D>(Ex, Abar, At, Ebar);
    T tb = T(0);
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int b = 0; b < D; ++b) {
        Gbar[a][b] = T(-0.5) * tau * Abar[a][b];
        tb = fmaT(Abar[a][b], G[a][b], tb);
      }
    if (gtau != nullptr) gtau[i] = T(-0.5) * tb;
  }
  // sum over the wave (LEG_THREADS = 64: one wave per workgroup), fixed order
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int b = 0; b < D; ++b) {
      T v = Gbar[a][b];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
      if (threadIdx.x == 0) red[a * D + b] = v;
    }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int q = 0; q < DD; ++q) gG_partial[(size_t)blockIdx.x * DD + q] = red[q];
  }
}

}  // namespace cgps
