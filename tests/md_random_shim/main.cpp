// Stand-alone host program over admp_amd/csrc/md_math.h (tests/test_md_random_cpu.py compiles and runs it).
//   md_random_shim                         the generator's three published known answers, one line of four hex words each
//   md_random_shim seed step stream n      atoms 0 .. n-1 of that counter: four hex words and three normals (%.17g) per line
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "md_math.h"

int main(int argc, char** argv) {
  if (argc == 5) {
    const uint64_t seed = strtoull(argv[1], nullptr, 0), step = strtoull(argv[2], nullptr, 0);
    const uint32_t stream = (uint32_t)strtoul(argv[3], nullptr, 0);
    const long n = strtol(argv[4], nullptr, 0);
    for (long i = 0; i < n; ++i) {
      uint32_t w[4];
      double xi[3];
      admp::md_random_words(seed, step, stream, (uint32_t)i, w);
      admp::md_random_normals(seed, step, stream, (uint32_t)i, xi);
      printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %.17g %.17g %.17g\n", w[0], w[1], w[2], w[3], xi[0], xi[1],
             xi[2]);
    }
    return 0;
  }
  if (argc != 1) {
    fprintf(stderr, "usage: %s [seed step stream n]\n", argv[0]);
    return 2;
  }
  const uint32_t cases[3][6] = {{0u, 0u, 0u, 0u, 0u, 0u},
                                {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu},
                                {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u, 0xa4093822u, 0x299f31d0u}};
  for (const auto& c : cases) {
    uint32_t w[4];
    admp::philox4x32_10(c, c + 4, w);
    printf("%08" PRIx32 " %08" PRIx32 " %08" PRIx32 " %08" PRIx32 "\n", w[0], w[1], w[2], w[3]);
  }
  return 0;
}
