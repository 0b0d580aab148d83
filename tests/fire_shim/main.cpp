// Stand-alone host program over admp_amd/csrc/md_fire_math.h (tests/test_md_fire_cpu.py compiles and runs it).
//   fire_shim s0 .. s7  w0 .. w5  p0 .. p8  ftol     the 8 state words, the 6 reduced words, the 9 parameters, ftol
// prints one line: moves (0 / 1), the 8 words of the new state, the 4 coefficients (a, b, back, dtv), all %.17g
#include <cstdio>
#include <cstdlib>

#include "md_fire_math.h"

int main(int argc, char** argv) {
  const int n_in = admp::FIRE_STATE_WORDS + admp::FIRE_SUM_WORDS + admp::FIRE_PARAM_WORDS + 1;
  if (argc != n_in + 1) {
    fprintf(stderr, "usage: %s state[8] sums[6] params[9] ftol\n", argv[0]);
    return 2;
  }
  double in[n_in];
  for (int k = 0; k < n_in; ++k) in[k] = strtod(argv[k + 1], nullptr);
  const double* state = in;
  const double* sums = state + admp::FIRE_STATE_WORDS;
  const double* par = sums + admp::FIRE_SUM_WORDS;
  double out[admp::FIRE_STATE_WORDS], coef[4];
  const int moves = admp::md_fire_control(state, sums, par, par[admp::FIRE_PARAM_WORDS], out, coef);
  printf("%d", moves);
  for (int w = 0; w < admp::FIRE_STATE_WORDS; ++w) printf(" %.17g", out[w]);
  for (int w = 0; w < 4; ++w) printf(" %.17g", coef[w]);
  printf("\n");
  return 0;
}
