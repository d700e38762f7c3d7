// Counter-based standard normals: element (r, s) of a [rows][cols] array is a pure function of (seed, stream, r, s).
// Nothing is carried from one element to the next, so a kernel can make the noise it needs in registers, and what it
// makes depends neither on how many columns are asked for, nor on which lane, panel or device makes it.
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), standard constants.
//   key     = (seed & 0xffffffff, seed >> 32)
//   counter = (r & 0xffffffff, r >> 32, g, stream)    r: 64-bit row-element index, g: column group, stream: caller's word
// fp64: group g gives columns 2g, 2g + 1 from the words w0..w3 of one block:
//   k1 = (w0 >> 6) 2^27 + (w1 >> 5), u1 = (k1 + 1) 2^-53 in (0, 1];  k2 = (w2 >> 6) 2^27 + (w3 >> 5), u2 = k2 2^-53 in [0, 1)
//   rho = sqrt(-2 ln u1);  column 2g = rho cos(2 pi u2), column 2g + 1 = rho sin(2 pi u2)
// fp32: group g gives columns 4g .. 4g + 3; (w0, w1) give 4g, 4g + 1 and (w2, w3) give 4g + 2, 4g + 3, each pair with
//   u1 = ((w >> 8) + 1) 2^-24, u2 = (w >> 8) 2^-24 (both exact in fp32) and the same Box-Muller form.
// Column s of row-element r therefore never depends on cols, and groups line up with the 2- and 4-column sub-panels
// of a lane (cgps_sample_tile.h).  Accurate log / sqrt / sincospi only: the library is built without fast-math.
//
// Host-pure: a plain C++17 compiler builds this header (tests/rng_check.cpp); under hipcc the same functions are
// __host__ __device__.  The host has no sincospi, so there the quarter turn is taken off exactly first.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define CGPS_HD __host__ __device__ __forceinline__
#else
#define CGPS_HD inline
#endif

namespace cgps {

struct Philox4 {
  uint32_t w[4];
};

CGPS_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += W0;
    k1 += W1;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// the block of row-element r, column group g
CGPS_HD Philox4 rng_block(uint64_t seed, uint32_t stream, uint64_t r, uint32_t g) {
  return philox4x32_10((uint32_t)r, (uint32_t)(r >> 32), g, stream, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// sin(pi x), cos(pi x) for 0 <= x < 2
CGPS_HD void rng_sincospi(double x, double* s, double* c) {
#if defined(__HIP_DEVICE_COMPILE__)
  ::sincospi(x, s, c);
#else
  const int q = (int)(2.0 * x + 0.5);                      // nearest quarter turn; x - q / 2 is exact, |.| <= 1/4
  const double t = 3.14159265358979323846 * (x - 0.5 * q), sr = sin(t), cr = cos(t);
  *s = (q & 1) ? ((q & 2) ? -cr : cr) : ((q & 2) ? -sr : sr);
  *c = (q & 1) ? ((q & 2) ? sr : -sr) : ((q & 2) ? -cr : cr);
#endif
}
CGPS_HD void rng_sincospi(float x, float* s, float* c) {
#if defined(__HIP_DEVICE_COMPILE__)
  ::sincospif(x, s, c);
#else
  const int q = (int)(2.0f * x + 0.5f);
  const float t = 3.14159265358979323846f * (x - 0.5f * q), sr = sinf(t), cr = cosf(t);
  *s = (q & 1) ? ((q & 2) ? -cr : cr) : ((q & 2) ? -sr : sr);
  *c = (q & 1) ? ((q & 2) ? sr : -sr) : ((q & 2) ? -cr : cr);
#endif
}

// Box-Muller: u1 in (0, 1], u2 in [0, 1)
CGPS_HD void box_muller(double u1, double u2, double* zc, double* zs) {
  const double rho = sqrt(-2.0 * log(u1));
  double s, c;
  rng_sincospi(2.0 * u2, &s, &c);
  *zc = rho * c;
  *zs = rho * s;
}
CGPS_HD void box_muller(float u1, float u2, float* zc, float* zs) {
  const float rho = sqrtf(-2.0f * logf(u1));
  float s, c;
  rng_sincospi(2.0f * u2, &s, &c);
  *zc = rho * c;
  *zs = rho * s;
}

// the pair of fp32 normals of two words
CGPS_HD void normal_pair_f32(uint32_t wa, uint32_t wb, float* z0, float* z1) {
  box_muller((float)((wa >> 8) + 1u) * 0x1.0p-24f, (float)(wb >> 8) * 0x1.0p-24f, z0, z1);
}

template <typename T> struct RngGroup;
template <> struct RngGroup<double> { static constexpr int COLS = 2; };
template <> struct RngGroup<float> { static constexpr int COLS = 4; };

// the RngGroup<T>::COLS normals of row-element r, column group g
CGPS_HD void normal_group(uint64_t seed, uint32_t stream, uint64_t r, uint32_t g, double* z) {
  const Philox4 p = rng_block(seed, stream, r, g);
  const uint64_t k1 = ((uint64_t)(p.w[0] >> 6) << 27) + (p.w[1] >> 5), k2 = ((uint64_t)(p.w[2] >> 6) << 27) + (p.w[3] >> 5);
  box_muller((double)(k1 + 1) * 0x1.0p-53, (double)k2 * 0x1.0p-53, &z[0], &z[1]);
}
CGPS_HD void normal_group(uint64_t seed, uint32_t stream, uint64_t r, uint32_t g, float* z) {
  const Philox4 p = rng_block(seed, stream, r, g);
  normal_pair_f32(p.w[0], p.w[1], &z[0], &z[1]);
  normal_pair_f32(p.w[2], p.w[3], &z[2], &z[3]);
}
// fp32, a two-column sub-panel: columns col, col + 1 (col even) are one half of group col / 4
CGPS_HD void normal_half_group(uint64_t seed, uint32_t stream, uint64_t r, uint64_t col, float* z) {
  const Philox4 p = rng_block(seed, stream, r, (uint32_t)(col >> 2));
  const bool hi = (col & 2) != 0;
  normal_pair_f32(hi ? p.w[2] : p.w[0], hi ? p.w[3] : p.w[1], &z[0], &z[1]);
}

}  // namespace cgps
