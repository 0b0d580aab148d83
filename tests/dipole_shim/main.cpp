// Stand-alone host program over the arithmetic of the dipole observable (admp_amd/csrc/dipole_math.h), the text the kernels of
// dipole_kernels.hip compile; tests/test_dipole_cpu.py compiles and runs it.
//   dipole_shim f|d < input   walks the groups as a lane of k_dipole_groups does, in float or double arithmetic, and adds the
//                             groups' words in group order; prints the 16 words, then mu_c (n_groups x 3)
// input (whitespace separated): n_atoms n_groups has_U, box (9, rows), then per atom r (3), Q_local (9), U (3), inv_mass,
// axis_type, axis atoms (3); then group_start (n_groups + 1) and group_atoms (n_atoms)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dipole_math.h"

namespace {

template <class T>
int run() {
  int n = 0, ng = 0, has_u = 0;
  if (scanf("%d %d %d", &n, &ng, &has_u) != 3 || n < 0 || ng < 0 || n > (1 << 24) || ng > (1 << 24)) return 2;
  double h[9], inv[9];
  for (double& x : h)
    if (scanf("%lf", &x) != 1) return 2;
  const size_t N = (size_t)n;
  std::vector<T> R(3 * N + 1), Q(9 * N + 1), U(3 * N + 1), IM(N + 1);
  std::vector<int> at(N + 1), ai(3 * N + 1), start((size_t)ng + 1), atoms(N + 1);
  for (size_t i = 0; i < N; ++i) {
    double x[16];
    for (double& y : x)
      if (scanf("%lf", &y) != 1) return 2;
    for (int c = 0; c < 3; ++c) { R[3 * i + c] = (T)x[c]; U[3 * i + c] = (T)x[12 + c]; }
    for (int c = 0; c < 9; ++c) Q[9 * i + c] = (T)x[3 + c];
    IM[i] = (T)x[15];
    if (scanf("%d %d %d %d", &at[i], &ai[3 * i], &ai[3 * i + 1], &ai[3 * i + 2]) != 4) return 2;
  }
  for (int g = 0; g <= ng; ++g)
    if (scanf("%d", &start[g]) != 1) return 2;
  for (size_t i = 0; i < N; ++i)
    if (scanf("%d", &atoms[i]) != 1) return 2;
  const double det = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
  inv[0] = (h[4] * h[8] - h[5] * h[7]) / det; inv[1] = (h[2] * h[7] - h[1] * h[8]) / det; inv[2] = (h[1] * h[5] - h[2] * h[4]) / det;
  inv[3] = (h[5] * h[6] - h[3] * h[8]) / det; inv[4] = (h[0] * h[8] - h[2] * h[6]) / det; inv[5] = (h[2] * h[3] - h[0] * h[5]) / det;
  inv[6] = (h[3] * h[7] - h[4] * h[6]) / det; inv[7] = (h[1] * h[6] - h[0] * h[7]) / det; inv[8] = (h[0] * h[4] - h[1] * h[3]) / det;
  admp::Box<T> box;
  for (int k = 0; k < 9; ++k) { box.h[k] = (T)h[k]; box.hinv[k] = (T)inv[k]; }
  double out[admp::kDipoleOutWords];
  for (double& x : out) x = 0.0;
  std::vector<double> mu(3 * (size_t)ng + 1);
  for (int g = 0; g < ng; ++g) {
    int a0 = start[g], a1 = start[g + 1];
    if (a0 < 0 || a1 > n || a1 < a0) a0 = a1 = 0;
    double part[9];
    admp::dipole_group<T>(at.data(), ai.data(), n, R.data(), box, Q.data(), has_u ? U.data() : nullptr, IM.data(), atoms.data() + a0,
                          a1 - a0, part);
    const double len = admp::dipole_total(part, &mu[3 * (size_t)g]);
    for (int k = 0; k < 9; ++k) out[k] += part[k];
    out[9] += len;
    out[10] += mu[3 * (size_t)g] * mu[3 * (size_t)g] + mu[3 * (size_t)g + 1] * mu[3 * (size_t)g + 1] + mu[3 * (size_t)g + 2] * mu[3 * (size_t)g + 2];
    out[11] = std::fmax(out[11], len);
  }
  out[12] = (double)ng;
  for (double x : out) printf("%.17g\n", x);
  for (int g = 0; g < ng; ++g) printf("%.17g %.17g %.17g\n", mu[3 * (size_t)g], mu[3 * (size_t)g + 1], mu[3 * (size_t)g + 2]);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && (argv[1][0] == 'f' || argv[1][0] == 'd')) return argv[1][0] == 'f' ? run<float>() : run<double>();
  fprintf(stderr, "usage: %s f|d   (input on stdin)\n", argv[0]);
  return 2;
}
