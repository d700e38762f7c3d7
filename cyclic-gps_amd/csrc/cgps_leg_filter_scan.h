// The time-parallel form of the LEG filter: the recursion of cgps_leg_filter.h is a composition of
// linear-fractional maps, the composition is associative, and a chunked scan over it hands every chunk of L rows the
// exact state it starts from; the walking kernel of cgps_leg_filter.h then runs over the chunks as if they were series.
//
// The element of rows j+1..i is (A, b, C, eta, J):  z_i | z_j, x_{j+1:i} ~ N(A z_j + b, C), and the likelihood of
// x_{j+1:i} as a function of z_j is proportional to exp(eta^T z_j - 1/2 z_j^T J z_j).  Earlier element 1 and later
// element 2 combine through X = (I + C1 J2)^-1 [A1 | b1 + C1 eta2 | C1] = [XA | xv | XC]:
//     A = A2 XA,  b = A2 xv + b2,  C = A2 XC A2^T + C2,  eta = XA^T (eta2 - J2 b1) + eta1,  J = A1^T J2 XA + J1
// (I + C1 J2 is not symmetric: LU with partial pivoting, in registers, the row exchanges as selects).  An element
// followed by ONE row with gap E = I + F, Q = I - E E^T = -(F + F^T + F F^T) (gap_gram: from F, never from E - I) needs
// the obs x obs factor alone:  A^- = E A1, b^- = E b1, C^- = E C1 E^T + Q,  S = (H C^- H^T + Cn)[o, o] = T T^T,
// W = T^-1 H C^-, U = T^-1 H A^-, r = T^-1 (x - H b^-):
//     A = A^- - W^T U,  b = b^- + W^T r,  C = C^- - W^T W,  eta = eta1 + U^T r,  J = J1 + U^T U.
// A series' first chunk starts from the reset element (0, m, P, 0, 0) of its start state (the prior N(0, I) at the first
// row, or the caller's state at t0) and carries the reset flag; a combination whose right operand is flagged IS the
// right operand (selected, not multiplied: a failed series before it holds NaN).
//
// Phases, each one launch per level at most, on one stream:
//   gaps      leg_fscan_gaps_kernel   one lane per (row, model): F of the gap before every row into the row's slot of
//                                     z_cov (scratch until the final phase writes E, then the row's z_cov, over it)
//   1 chunks  leg_fscan_chunk_kernel  one lane per (chunk, model) composes its L rows, writes the chunk's summary
//   2 up      leg_fscan_up_kernel     one lane per group of F elements: inclusive local prefixes in place, the last up
//   3 down    leg_fscan_down_kernel   one lane per element applies the completed prefix of the group before its own
//     starts  leg_fscan_starts_kernel one lane per (chunk, model): t0, m0, P0 of the chunk from the prefix before it
//   4 rows    launch_filter           leg_filter_gaps_kernel and leg_filter_kernel over the chunks, untouched
//   5 series  leg_fscan_series_kernel one lane per (series, model): the chunks' log-likelihoods in chunk order, the
//                                     last chunk's end state
// A row with a negative or non-finite gap, a pivot of S that is not positive or a result that is not finite poisons its
// chunk's summary (all NaN, the flag kept): the later chunks of that series start from NaN and fail in phase 4, the
// rows before the failing row come out of phase 4 from good states.  No LDS, no atomics (report_fail's are phase 4's).
#pragma once
#include "cgps_leg_filter.h"
#include "cgps_plan.h"

namespace cgps {

using cgps_host::filter_scan_elem_scalars;

// An element, and where its scalars live in a level: A, b, C, h (eta), J row-major in that order, then the reset flag.
template <typename T, int D>
struct ScanElem {
  T A[D][D], b[D], C[D][D], h[D], J[D][D];
  static constexpr int OFF_A = 0, OFF_B = OFF_A + D * D, OFF_C = OFF_B + D, OFF_H = OFF_C + D * D, OFF_J = OFF_H + D,
                       OFF_FLAG = OFF_J + D * D;
  static_assert(OFF_FLAG + 1 == filter_scan_elem_scalars(D), "the element's scalars and the flag: cgps_plan.h owns the count");
  // f(offset, scalar) for every scalar of e (a ScanElem or a const one) in the stored order
  template <typename E, typename Fn>
  static __device__ __forceinline__ void visit(E& e, Fn&& f) {
    mat(OFF_A, e.A, f);
    vec(OFF_B, e.b, f);
    mat(OFF_C, e.C, f);
    vec(OFF_H, e.h, f);
    mat(OFF_J, e.J, f);
  }
  template <typename V, typename Fn>
  static __device__ __forceinline__ void vec(int off, V (&v)[D], Fn&& f) {
#pragma unroll
    for (int a = 0; a < D; ++a) f(off + a, v[a]);
  }
  template <typename V, typename Fn>
  static __device__ __forceinline__ void mat(int off, V (&m)[D][D], Fn&& f) {
#pragma unroll
    for (int a = 0; a < D; ++a) vec(off + a * D, m[a], f);
  }
};

// element c of a level of n elements under one model: scalar v lives at p[v * n], p = level + model offset + c
template <typename T, int D>
__device__ __forceinline__ void scan_load(const T* p, int64_t n, ScanElem<T, D>& e, bool& flag) {
  ScanElem<T, D>::visit(e, [&](int v, T& x) { x = p[v * n]; });
  flag = p[ScanElem<T, D>::OFF_FLAG * n] != T(0);
}

template <typename T, int D>
__device__ __forceinline__ void scan_store(T* p, int64_t n, const ScanElem<T, D>& e, bool flag, bool poison) {
  const T nan = (T)__builtin_nan("");
  ScanElem<T, D>::visit(e, [&](int v, const T& x) { p[v * n] = poison ? nan : x; });
  p[ScanElem<T, D>::OFF_FLAG * n] = flag ? T(1) : T(0);
}

// K = P L U in place (unit lower L below the diagonal, U on and above it, 1 / U_cc in inv), the exchanges of whole rows
// in piv: partial pivoting with every index a compile-time one (the exchange is a select over the rows below)
template <typename T, int D>
__device__ __forceinline__ void lu_factor(T (&K)[D][D], int (&piv)[D], T (&inv)[D]) {
#pragma unroll
  for (int col = 0; col < D; ++col) {
    int p = col;
    T best = K[col][col] < T(0) ? -K[col][col] : K[col][col];
#pragma unroll
    for (int r = col + 1; r < D; ++r) {
      const T a = K[r][col] < T(0) ? -K[r][col] : K[r][col];
      if (a > best) { best = a; p = r; }
    }
    piv[col] = p;
#pragma unroll
    for (int r = col + 1; r < D; ++r) {
      const bool sw = r == p;
#pragma unroll
      for (int c = 0; c < D; ++c) {
        const T u = K[col][c], w = K[r][c];
        K[col][c] = sw ? w : u;
        K[r][c] = sw ? u : w;
      }
    }
    inv[col] = T(1) / K[col][col];
#pragma unroll
    for (int r = col + 1; r < D; ++r) {
      K[r][col] *= inv[col];
#pragma unroll
      for (int c = col + 1; c < D; ++c) K[r][c] = fmaT(-K[r][col], K[col][c], K[r][c]);
    }
  }
}

template <typename T, int D>
__device__ __forceinline__ void lu_solve(const T (&K)[D][D], const int (&piv)[D], const T (&inv)[D], T (&x)[D]) {
#pragma unroll
  for (int col = 0; col < D; ++col)
#pragma unroll
    for (int r = col + 1; r < D; ++r) {
      const bool sw = r == piv[col];
      const T u = x[col], w = x[r];
      x[col] = sw ? w : u;
      x[r] = sw ? u : w;
    }
#pragma unroll
  for (int i = 1; i < D; ++i)
#pragma unroll
    for (int j = 0; j < i; ++j) x[i] = fmaT(-K[i][j], x[j], x[i]);
#pragma unroll
  for (int i = D - 1; i >= 0; --i) {
#pragma unroll
    for (int j = i + 1; j < D; ++j) x[i] = fmaT(-K[i][j], x[j], x[i]);
    x[i] *= inv[i];
  }
}

// e1 <- the element of e1's rows followed by e2's (f2: e2 starts a series, the result is e2 itself)
template <typename T, int D>
__device__ __forceinline__ void scan_combine(ScanElem<T, D>& e1, const ScanElem<T, D>& e2, bool f2) {
  if (f2) {
    e1 = e2;
    return;
  }
  T K[D][D], inv[D];
  int piv[D];
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int c = 0; c < D; ++c) {
      T s = a == c ? T(1) : T(0);
#pragma unroll
      for (int q = 0; q < D; ++q) s = fmaT(e1.C[a][q], e2.J[q][c], s);
      K[a][c] = s;
    }
  lu_factor<T, D>(K, piv, inv);
  T xv[D], u[D];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    T s = e1.b[a], w = e2.h[a];
#pragma unroll
    for (int q = 0; q < D; ++q) {
      s = fmaT(e1.C[a][q], e2.h[q], s);
      w = fmaT(-e2.J[a][q], e1.b[q], w);
    }
    xv[a] = s;
    u[a] = w;
  }
  lu_solve<T, D>(K, piv, inv, xv);
  T XA[D][D], XC[D][D];                            // column j of K^-1 A1 is XA[.][j]
#pragma unroll
  for (int j = 0; j < D; ++j) {
    T va[D], vc[D];
#pragma unroll
    for (int a = 0; a < D; ++a) {
      va[a] = e1.A[a][j];
      vc[a] = e1.C[a][j];
    }
    lu_solve<T, D>(K, piv, inv, va);
    lu_solve<T, D>(K, piv, inv, vc);
#pragma unroll
    for (int a = 0; a < D; ++a) {
      XA[a][j] = va[a];
      XC[a][j] = vc[a];
    }
  }
  // eta and J first: they read A1, which A overwrites
  T JX[D][D];
  mat_mul<T, D>(JX, e2.J, XA);
#pragma unroll
  for (int a = 0; a < D; ++a) {
    T s = e1.h[a];
#pragma unroll
    for (int q = 0; q < D; ++q) s = fmaT(XA[q][a], u[q], s);
    e1.h[a] = s;
  }
  {
    T Jn[D][D];
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int c = 0; c < D; ++c) {
        T s = T(0);
#pragma unroll
        for (int q = 0; q < D; ++q) s = fmaT(e1.A[q][a], JX[q][c], s);
        Jn[a][c] = s;
      }
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int c = 0; c <= a; ++c) e1.J[a][c] = e1.J[c][a] = e1.J[a][c] + T(0.5) * (Jn[a][c] + Jn[c][a]);
  }
  mat_mul<T, D>(e1.A, e2.A, XA);
#pragma unroll
  for (int a = 0; a < D; ++a) {
    T s = e2.b[a];
#pragma unroll
    for (int q = 0; q < D; ++q) s = fmaT(e2.A[a][q], xv[q], s);
    e1.b[a] = s;
  }
  {
    T AX[D][D];
    mat_mul<T, D>(AX, e2.A, XC);
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int c = 0; c < D; ++c) {
        T s = T(0);
#pragma unroll
        for (int q = 0; q < D; ++q) s = fmaT(AX[a][q], e2.A[c][q], s);
        XC[a][c] = s;
      }
#pragma unroll
    for (int a = 0; a < D; ++a)
#pragma unroll
      for (int c = 0; c <= a; ++c) e1.C[a][c] = e1.C[c][a] = e2.C[a][c] + T(0.5) * (XC[a][c] + XC[c][a]);
  }
}

// F = expm1(-1/2 gap G) of the gap before every row but the first of the R, under every model, into that row's slot of
// z_cov: leg_filter_gaps_kernel without the identity.  A gap that is negative or not finite is evaluated as zero; the
// lane that walks the chunk poisons its summary from the time stamps themselves.
template <typename T, int D>
__global__ __launch_bounds__(FILTER_THREADS) void leg_fscan_gaps_kernel(const T* __restrict__ ts, int64_t R,
                                                                         const T* __restrict__ Gg, T* __restrict__ z_cov) {
  const int64_t i = (int64_t)blockIdx.x * FILTER_THREADS + threadIdx.x;
  if (i < 1 || i >= R) return;
  const int64_t k = blockIdx.y;
  const T* __restrict__ Gk = Gg + (size_t)k * D * D;
  const T dt = ts[i] - ts[i - 1];
  T F[D][D];
  gap_expm1<T, D>((dt >= T(0) && finiteT(dt)) ? dt : T(0), [&](int a, int c) { return Gk[a * D + c]; }, F);
  T* __restrict__ out = z_cov + (k * R + i) * D * D;
#pragma unroll
  for (int a = 0; a < D; ++a)
#pragma unroll
    for (int c = 0; c < D; ++c) out[a * D + c] = F[a][c];
}

// Phase 1.  coff[NC + 1]: the chunks' row offsets; cser[NC]: the series of every chunk; scoff[B + 1]: the first chunk
// of every series (chunk c starts its series when scoff[cser[c]] == c, and ends it when scoff[cser[c] + 1] == c + 1:
// nobody combines with the summary of a series' last chunk, whose lane stores zeros and walks nothing).
template <typename T, int D, int O>
__global__ __launch_bounds__(FILTER_THREADS) void leg_fscan_chunk_kernel(
    const T* __restrict__ ts, const T* __restrict__ xs, const unsigned char* __restrict__ pattern,
    const T* __restrict__ noise, const int64_t* __restrict__ coff, const int64_t* __restrict__ cser,
    const int64_t* __restrict__ scoff, int64_t NC, int64_t B, int64_t R, const T* __restrict__ Gg,
    const T* __restrict__ Bg, const T* __restrict__ LLTg, int obs_rt, const T* __restrict__ t0,
    const T* __restrict__ m0, const T* __restrict__ P0, const T* __restrict__ Fg, T* __restrict__ elems) {
  const int obs = O <= 4 ? O : obs_rt;
  const int64_t c = (int64_t)blockIdx.x * FILTER_THREADS + threadIdx.x;
  if (c >= NC) return;
  const int64_t k = blockIdx.y;
  const int64_t b = cser[c];
  if (b < 0 || b >= B) return;
  int64_t r0 = coff[c], r1 = coff[c + 1];
  r0 = r0 < 0 ? 0 : r0;
  r1 = r1 > R ? R : r1;
  const bool first = scoff[b] == c, last = scoff[b + 1] == c + 1;
  const T* __restrict__ Gk = Gg + (size_t)k * D * D;
  const T* __restrict__ Bk = Bg + (size_t)k * obs * D;
  const T* __restrict__ Ck = LLTg + (size_t)k * obs * obs;
  const unsigned full = (1u << obs) - 1u;
  auto Bm = [&](int q, int a) -> T { return q < obs ? Bk[q * D + a] : T(0); };
  T* __restrict__ out = elems + (size_t)k * filter_scan_elem_scalars(D) * NC + c;

  ScanElem<T, D> e;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    e.b[a] = e.h[a] = T(0);
#pragma unroll
    for (int q = 0; q < D; ++q) {
      e.A[a][q] = (!first && a == q) ? T(1) : T(0);          // the identity element, or a reset
      e.C[a][q] = (first && a == q) ? T(1) : T(0);           // ... from the prior N(0, I)
      e.J[a][q] = T(0);
    }
  }
  if (last) {
    scan_store<T, D>(out, NC, e, first, false);
    return;
  }
  T tprev = T(0);
  bool have = true;                                // a gap to cross before the chunk's first row
  if (first) {
    have = t0 != nullptr;
    if (have) {
      const int64_t s = k * B + b;
      tprev = t0[b];
      load_vec<T, D>(m0 + s * D, e.b);
#pragma unroll
      for (int a = 0; a < D; ++a)
#pragma unroll
        for (int q = 0; q <= a; ++q) e.C[a][q] = e.C[q][a] = P0[(s * D + a) * D + q];
    }
  } else {
    tprev = ts[r0 - 1];
  }

  bool fail = false;
  for (int64_t i = r0; i < r1 && !fail; ++i) {
    const T t = ts[i];
    if (have) {
      // ---- across the gap:  A^- = E A, b^- = E b, C^- = E C E^T + Q
      const T dt = t - tprev;
      fail = !(dt >= T(0)) || !finiteT(dt);
      T F[D][D], Q[D][D];
      if (first && i == r0) {                      // the gap from t0 to the series' first row
        gap_expm1<T, D>(fail ? T(0) : dt, [&](int a, int q) { return Gk[a * D + q]; }, F);
      } else {
#pragma unroll
        for (int a = 0; a < D; ++a) load_vec<T, D>(Fg + ((k * R + i) * D + a) * D, F[a]);
      }
      gap_gram<T, D, true>(F, Q);
      add_identity<T, D>(F);                       // E
      T EA[D][D], EC[D][D], eb[D];
      mat_mul<T, D>(EA, F, e.A);
      mat_mul<T, D>(EC, F, e.C);
#pragma unroll
      for (int a = 0; a < D; ++a) {
        T s = T(0);
#pragma unroll
        for (int q = 0; q < D; ++q) s = fmaT(F[a][q], e.b[q], s);
        eb[a] = s;
#pragma unroll
        for (int q = 0; q <= a; ++q) {
          T w = T(0.5) * (Q[a][q] + Q[q][a]);
#pragma unroll
          for (int p = 0; p < D; ++p) w = fmaT(EC[a][p], F[q][p], w);
          e.C[a][q] = e.C[q][a] = w;
        }
      }
#pragma unroll
      for (int a = 0; a < D; ++a) {
        e.b[a] = eb[a];
#pragma unroll
        for (int q = 0; q < D; ++q) e.A[a][q] = EA[a][q];
      }
    }
    have = true;
    tprev = t;

    // ---- the row's observation
    // (a row that observes nothing has S = I, W = U = 0, r = 0: (E A, E b, E C E^T + Q, eta, J) to the bit)
    const unsigned p = pattern != nullptr ? ((unsigned)pattern[i] & full) : full;
    bool on[O];
    T x[O], s[O];
#pragma unroll
    for (int q = 0; q < O; ++q) {
      on[q] = (p >> q) & 1u;
      x[q] = on[q] ? xs[i * obs + q] : T(0);
      s[q] = (on[q] && noise != nullptr) ? noise[i * obs + q] : T(0);
    }
    T hc[O][D], ha[O][D], r[O];                    // H C^-, H A^-, x - H b^-
#pragma unroll
    for (int q = 0; q < O; ++q) {
      T w = T(0);
#pragma unroll
      for (int a = 0; a < D; ++a) {
        T u = T(0), v = T(0);
#pragma unroll
        for (int j = 0; j < D; ++j) {
          u = fmaT(Bm(q, j), e.C[j][a], u);
          v = fmaT(Bm(q, j), e.A[j][a], v);
        }
        hc[q][a] = u;
        ha[q][a] = v;
        w = fmaT(Bm(q, a), e.b[a], w);
      }
      r[q] = on[q] ? x[q] - w : T(0);
    }
    Chol<T, O> Tw;
    {
      T S[O][O];
#pragma unroll
      for (int q = 0; q < O; ++q)
#pragma unroll
        for (int j = 0; j <= q; ++j) {
          T u = (q < obs && j < obs) ? Ck[q * obs + j] : T(0);
#pragma unroll
          for (int a = 0; a < D; ++a) u = fmaT(hc[q][a], Bm(j, a), u);
          if (q == j) u += s[q];
          S[q][j] = S[j][q] = (on[q] && on[j]) ? u : (q == j ? T(1) : T(0));
        }
      chol_lower<T, O>(S, Tw, fail);
    }
    fwd_subst<T, O>(Tw, r);
    T chk = T(0);
    {
      T Wt[D][O], Ut[D][O];                        // column a of W = T^-1 H C^- is Wt[a], of U = T^-1 H A^- is Ut[a]
#pragma unroll
      for (int a = 0; a < D; ++a) {
#pragma unroll
        for (int q = 0; q < O; ++q) {
          Wt[a][q] = on[q] ? hc[q][a] : T(0);
          Ut[a][q] = on[q] ? ha[q][a] : T(0);
        }
        fwd_subst<T, O>(Tw, Wt[a]);
        fwd_subst<T, O>(Tw, Ut[a]);
      }
#pragma unroll
      for (int a = 0; a < D; ++a) {
        T u = e.b[a], v = e.h[a];
#pragma unroll
        for (int q = 0; q < O; ++q) {
          u = fmaT(Wt[a][q], r[q], u);
          v = fmaT(Ut[a][q], r[q], v);
        }
        e.b[a] = u;
        e.h[a] = v;
        chk += u + v;
#pragma unroll
        for (int j = 0; j < D; ++j) {
          T w = e.A[a][j];
#pragma unroll
          for (int q = 0; q < O; ++q) w = fmaT(-Wt[a][q], Ut[j][q], w);
          e.A[a][j] = w;
          chk += w;
        }
#pragma unroll
        for (int j = 0; j <= a; ++j) {
          T w = e.C[a][j], y = e.J[a][j];
#pragma unroll
          for (int q = 0; q < O; ++q) {
            w = fmaT(-Wt[a][q], Wt[j][q], w);
            y = fmaT(Ut[a][q], Ut[j][q], y);
          }
          e.C[a][j] = e.C[j][a] = w;
          e.J[a][j] = e.J[j][a] = y;
          chk += w + y;
        }
      }
    }
    fail = fail || !finiteT(chk);
  }
  scan_store<T, D>(out, NC, e, first, fail);
}

// Phase 2 at one level of n elements per model: lane g turns elements [g F, min(n, g F + F)) into inclusive local
// prefixes in place and, when a level follows (up != nullptr, of nup elements), leaves the last one there.
template <typename T, int D>
__global__ __launch_bounds__(FILTER_THREADS) void leg_fscan_up_kernel(T* __restrict__ lev, int64_t n, int64_t F,
                                                                       T* __restrict__ up, int64_t nup) {
  const int64_t g = (int64_t)blockIdx.x * FILTER_THREADS + threadIdx.x;
  const int64_t j0 = g * F;
  if (j0 >= n) return;
  const int64_t j1 = j0 + F < n ? j0 + F : n;
  const int64_t k = blockIdx.y;
  constexpr int NV = filter_scan_elem_scalars(D);
  T* __restrict__ mine = lev + (size_t)k * NV * n;
  ScanElem<T, D> acc;
  bool flag;
  scan_load<T, D>(mine + j0, n, acc, flag);
  for (int64_t j = j0 + 1; j < j1; ++j) {
    ScanElem<T, D> e;
    bool f;
    scan_load<T, D>(mine + j, n, e, f);
    scan_combine<T, D>(acc, e, f);
    flag = flag || f;
    scan_store<T, D>(mine + j, n, acc, flag, false);
  }
  if (up != nullptr && g < nup) scan_store<T, D>(up + (size_t)k * NV * nup + g, nup, acc, flag, false);
}

// Phase 3 at one level: element j >= F becomes (completed prefix of group j / F - 1, from the level above) o (its local
// prefix); an element that holds a reset stays as it is.
template <typename T, int D>
__global__ __launch_bounds__(FILTER_THREADS) void leg_fscan_down_kernel(T* __restrict__ lev, int64_t n, int64_t F,
                                                                         const T* __restrict__ up, int64_t nup) {
  const int64_t j = (int64_t)blockIdx.x * FILTER_THREADS + threadIdx.x + F;
  if (j >= n) return;
  const int64_t g = j / F - 1;
  if (g >= nup) return;
  const int64_t k = blockIdx.y;
  constexpr int NV = filter_scan_elem_scalars(D);
  T* __restrict__ mine = lev + (size_t)k * NV * n + j;
  ScanElem<T, D> e;
  bool f;
  scan_load<T, D>(mine, n, e, f);
  if (f) return;
  ScanElem<T, D> acc;
  bool fa;
  scan_load<T, D>(up + (size_t)k * NV * nup + g, nup, acc, fa);
  scan_combine<T, D>(acc, e, false);
  scan_store<T, D>(mine, n, acc, fa, false);
}

// The state every chunk starts from, as leg_filter_kernel takes it: a series' first chunk the caller's (t0, m0, P0) or
// (the first row's time stamp, 0, I), which the kernel carries across a gap of zero to the prior's bits; any other
// chunk (the time stamp of the row before, b and C of the completed prefix of the chunk before).
template <typename T, int D>
__global__ __launch_bounds__(FILTER_THREADS) void leg_fscan_starts_kernel(
    const T* __restrict__ ts, const int64_t* __restrict__ coff, const int64_t* __restrict__ cser,
    const int64_t* __restrict__ scoff, int64_t NC, int64_t B, int64_t R, const T* __restrict__ t0,
    const T* __restrict__ m0, const T* __restrict__ P0, const T* __restrict__ elems, T* __restrict__ t0c,
    T* __restrict__ m0c, T* __restrict__ P0c) {
  const int64_t c = (int64_t)blockIdx.x * FILTER_THREADS + threadIdx.x;
  if (c >= NC) return;
  const int64_t k = blockIdx.y;
  const int64_t b = cser[c];
  if (b < 0 || b >= B) return;
  int64_t r0 = coff[c];
  r0 = r0 < 0 ? 0 : (r0 >= R ? R - 1 : r0);
  const int64_t slot = k * NC + c;
  const bool first = scoff[b] == c;
  using Elem = ScanElem<T, D>;
  constexpr int NV = filter_scan_elem_scalars(D);
  const T* __restrict__ prev = elems + (size_t)k * NV * NC + (c > 0 ? c - 1 : 0);
  const int64_t s = k * B + b;
  if (k == 0) t0c[c] = first ? (t0 != nullptr ? t0[b] : ts[r0]) : ts[r0 > 0 ? r0 - 1 : 0];
#pragma unroll
  for (int a = 0; a < D; ++a) {
    m0c[slot * D + a] = first ? (m0 != nullptr ? m0[s * D + a] : T(0)) : prev[(size_t)(Elem::OFF_B + a) * NC];
#pragma unroll
    for (int q = 0; q < D; ++q)
      P0c[(slot * D + a) * D + q] = first ? (P0 != nullptr ? P0[(s * D + a) * D + q] : (a == q ? T(1) : T(0)))
                                          : prev[(size_t)(Elem::OFF_C + a * D + q) * NC];
  }
}

// Phase 5: one lane per (series, model) adds its chunks' log-likelihoods in chunk order; the end state is the last chunk's.
template <typename T, int D>
__global__ __launch_bounds__(FILTER_THREADS) void leg_fscan_series_kernel(
    const int64_t* __restrict__ scoff, int64_t NC, int64_t B, const double* __restrict__ llc, const T* __restrict__ mc,
    const T* __restrict__ Pc, double* __restrict__ loglik, T* __restrict__ m_end, T* __restrict__ P_end) {
  const int64_t b = (int64_t)blockIdx.x * FILTER_THREADS + threadIdx.x;
  if (b >= B) return;
  const int64_t k = blockIdx.y;
  int64_t c0 = scoff[b], c1 = scoff[b + 1];
  c0 = c0 < 0 ? 0 : c0;
  c1 = c1 > NC ? NC : c1;
  if (c1 <= c0) return;
  double ll = 0.0;
  for (int64_t c = c0; c < c1; ++c) ll += llc[k * NC + c];
  const int64_t slot = k * B + b, from = k * NC + c1 - 1;
  loglik[slot] = ll;
#pragma unroll
  for (int a = 0; a < D; ++a) {
    m_end[slot * D + a] = mc[from * D + a];
#pragma unroll
    for (int q = 0; q < D; ++q) P_end[(slot * D + a) * D + q] = Pc[(from * D + a) * D + q];
  }
}

template <typename T, int D>
void launch_filter_scan(const T* ts, const T* xs, const unsigned char* pattern, const T* noise, int64_t B, int64_t R,
                        int64_t M, const T* G, const T* Bm, const T* LLT, int obs, const T* t0, const T* m0, const T* P0,
                        const int64_t* coff, const int64_t* cser, const int64_t* scoff, int64_t NC, int64_t fanout,
                        char* ws, const cgps_host::FilterScanWs& w, T* pred_mean, T* pred_cov, T* logpdf, T* z_mean,
                        T* z_cov, double* loglik, T* m_end, T* P_end, int* info, hipStream_t st) {
  using cgps_host::at;
  const dim3 block(FILTER_THREADS);
  auto grid = [&](int64_t n) { return dim3((unsigned)((n + FILTER_THREADS - 1) / FILTER_THREADS), (unsigned)M); };
  T* lev0 = at<T>(ws, w.elem[0]);
  if (R > 1) hipLaunchKernelGGL((leg_fscan_gaps_kernel<T, D>), grid(R), block, 0, st, ts, R, G, z_cov);
  cgps_host::dispatch_obs(obs, [&](auto oc) {
    hipLaunchKernelGGL((leg_fscan_chunk_kernel<T, D, decltype(oc)::value>), grid(NC), block, 0, st, ts, xs, pattern, noise,
                       coff, cser, scoff, NC, B, R, G, Bm, LLT, obs, t0, m0, P0, (const T*)z_cov, lev0);
  });
  for (int l = 0; l < w.levels; ++l) {
    if (w.n[l] < 2) break;
    const bool has_up = l + 1 < w.levels;
    const int64_t groups = (w.n[l] + fanout - 1) / fanout;
    hipLaunchKernelGGL((leg_fscan_up_kernel<T, D>), grid(groups), block, 0, st, at<T>(ws, w.elem[l]), w.n[l], fanout,
                       has_up ? at<T>(ws, w.elem[l + 1]) : (T*)nullptr, has_up ? w.n[l + 1] : (int64_t)0);
  }
  for (int l = w.levels - 2; l >= 0; --l)
    hipLaunchKernelGGL((leg_fscan_down_kernel<T, D>), grid(w.n[l] - fanout), block, 0, st, at<T>(ws, w.elem[l]), w.n[l],
                       fanout, (const T*)at<T>(ws, w.elem[l + 1]), w.n[l + 1]);
  T *t0c = at<T>(ws, w.t0), *m0c = at<T>(ws, w.m0), *P0c = at<T>(ws, w.P0);
  double* llc = at<double>(ws, w.loglik);
  T *mc = at<T>(ws, w.m_end), *Pc = at<T>(ws, w.P_end);
  hipLaunchKernelGGL((leg_fscan_starts_kernel<T, D>), grid(NC), block, 0, st, ts, coff, cser, scoff, NC, B, R, t0, m0, P0,
                     (const T*)lev0, t0c, m0c, P0c);
  launch_filter<T, D>(ts, xs, pattern, noise, coff, NC, R, M, G, Bm, LLT, obs, t0c, m0c, P0c, pred_mean, pred_cov, logpdf,
                      z_mean, z_cov, llc, mc, Pc, info, st);
  hipLaunchKernelGGL((leg_fscan_series_kernel<T, D>), grid(B), block, 0, st, scoff, NC, B, (const double*)llc,
                     (const T*)mc, (const T*)Pc, loglik, m_end, P_end);
}

}  // namespace cgps
