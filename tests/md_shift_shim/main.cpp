// Stand-alone host program over the minimum-image helpers of admp_amd/csrc/pme_math.h as md_kernels.hip k_md_bonded_box uses
// them (tests/test_md_shift_cpu.py compiles and runs it).
//   md_shift_shim f|d h0 .. h8 dx dy dz     (box rows, raw bond vector; f: float, d: double arithmetic)
// prints: crosses (0/1), the lattice translation image_shift removes (3), the minimum-image vector (3), all %.17g
#include <cstdio>
#include <cstdlib>

#include "pme_math.h"

template <class T>
static int run(char** a) {
  double h[9], inv[9];
  for (int k = 0; k < 9; ++k) h[k] = strtod(a[k], nullptr);
  const double det = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
  inv[0] = (h[4] * h[8] - h[5] * h[7]) / det; inv[1] = (h[2] * h[7] - h[1] * h[8]) / det; inv[2] = (h[1] * h[5] - h[2] * h[4]) / det;
  inv[3] = (h[5] * h[6] - h[3] * h[8]) / det; inv[4] = (h[0] * h[8] - h[2] * h[6]) / det; inv[5] = (h[2] * h[3] - h[0] * h[5]) / det;
  inv[6] = (h[3] * h[7] - h[4] * h[6]) / det; inv[7] = (h[1] * h[6] - h[0] * h[7]) / det; inv[8] = (h[0] * h[4] - h[1] * h[3]) / det;
  admp::Box<T> b;
  for (int k = 0; k < 9; ++k) { b.h[k] = (T)h[k]; b.hinv[k] = (T)inv[k]; }
  T d[3] = {(T)strtod(a[9], nullptr), (T)strtod(a[10], nullptr), (T)strtod(a[11], nullptr)}, sh[3];
  const bool crosses = admp::image_shift(b, d, sh);
  admp::min_image(b, d);
  printf("%d %.17g %.17g %.17g %.17g %.17g %.17g\n", crosses ? 1 : 0, (double)sh[0], (double)sh[1], (double)sh[2], (double)d[0],
         (double)d[1], (double)d[2]);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 14 || (argv[1][0] != 'f' && argv[1][0] != 'd')) {
    fprintf(stderr, "usage: %s f|d h0 .. h8 dx dy dz\n", argv[0]);
    return 2;
  }
  return argv[1][0] == 'f' ? run<float>(argv + 2) : run<double>(argv + 2);
}
