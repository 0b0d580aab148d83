// Stand-alone host program over admp_amd/csrc/md_vrescale_math.h (tests/test_md_vrescale_cpu.py compiles and runs it).
//   vrescale_shim prec s0 .. s7 K n_dof kT_acc c seed step     prec 4 / 8: the type of the velocities; s: the 8 state words
// prints one line: scales (0 / 1), the returned factor, the 8 words of the new state (%.17g), the tries of the noise alone (-1:
// out of tries), then the 4 Philox words of counter index 0 and the 4 of counter index 1 (hex)
#include <cinttypes>
#include <cstdio>
#include <cstdlib>

#include "md_vrescale_math.h"

int main(int argc, char** argv) {
  if (argc != 16) {
    fprintf(stderr, "usage: %s prec state[8] K n_dof kT_acc c seed step\n", argv[0]);
    return 2;
  }
  const int prec = atoi(argv[1]);
  double in[admp::VR_STATE_WORDS], out[admp::VR_STATE_WORDS];
  for (int k = 0; k < admp::VR_STATE_WORDS; ++k) in[k] = strtod(argv[2 + k], nullptr);
  const double K = strtod(argv[10], nullptr), kT_acc = strtod(argv[12], nullptr), c = strtod(argv[13], nullptr);
  const int64_t n_dof = strtoll(argv[11], nullptr, 10);
  const uint64_t seed = strtoull(argv[14], nullptr, 10), step = strtoull(argv[15], nullptr, 10);
  int scales = 0;
  const double alpha = prec == 4 ? admp::md_vrescale_rule<float>(in, K, n_dof, kT_acc, c, seed, step, out, &scales)
                                 : admp::md_vrescale_rule<double>(in, K, n_dof, kT_acc, c, seed, step, out, &scales);
  double R1, S;
  const int tries = admp::md_vrescale_noise(seed, step, n_dof, &R1, &S);
  printf("%d %.17g", scales, alpha);
  for (int w = 0; w < admp::VR_STATE_WORDS; ++w) printf(" %.17g", out[w]);
  printf(" %d", tries);
  for (uint32_t index = 0; index < 2; ++index) {
    uint32_t w[4];
    admp::md_random_words(seed, step, admp::kStreamVRescale, index, w);
    for (int k = 0; k < 4; ++k) printf(" %08" PRIx32, w[k]);
  }
  printf("\n");
  return 0;
}
