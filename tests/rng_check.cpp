// Includes csrc/cgps_rng.h ALONE and is built by a plain C++17 host compiler (the header is host-pure).  Prints what
// tests/test_rng_spec.py compares with the numpy restatement of the specification (tests/_rngref.py):
//   kat <8 hex words>                three Philox4x32-10 known answers
//   f64 <row> <col> <value>          the fp64 normals of a [64][9] array, seed 2024, stream 0
//   f32 <row> <col> <value>          the fp32 normals of the same array
#include <cstdio>

#include "cgps_rng.h"

int main() {
  const uint32_t kat[3][6] = {{0, 0, 0, 0, 0, 0},
                              {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                              {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u}};
  for (const auto& k : kat) {
    const cgps::Philox4 p = cgps::philox4x32_10(k[0], k[1], k[2], k[3], k[4], k[5]);
    std::printf("kat %08x %08x %08x %08x\n", p.w[0], p.w[1], p.w[2], p.w[3]);
  }
  const int rows = 64, cols = 9;
  const uint64_t seed = 2024;
  for (int r = 0; r < rows; ++r) {
    for (int g = 0; 2 * g < cols; ++g) {
      double z[2];
      cgps::normal_group(seed, 0u, (uint64_t)r, (uint32_t)g, z);
      for (int u = 0; u < 2 && 2 * g + u < cols; ++u) std::printf("f64 %d %d %.17g\n", r, 2 * g + u, z[u]);
    }
    for (int g = 0; 4 * g < cols; ++g) {
      float z[4];
      cgps::normal_group(seed, 0u, (uint64_t)r, (uint32_t)g, z);
      for (int u = 0; u < 4 && 4 * g + u < cols; ++u) std::printf("f32 %d %d %.9g\n", r, 4 * g + u, (double)z[u]);
      // a two-column sub-panel takes half a group: the same values
      float h[2];
      for (int c = 0; c < 4; c += 2) {
        cgps::normal_half_group(seed, 0u, (uint64_t)r, (uint64_t)(4 * g + c), h);
        if (h[0] != z[c] || h[1] != z[c + 1]) {
          std::printf("half group differs at row %d column %d\n", r, 4 * g + c);
          return 1;
        }
      }
    }
  }
  return 0;
}
