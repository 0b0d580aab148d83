// Stand-alone host program over the plan of the molecular-scaling kernels (admp_amd/csrc/mol_plan.h) and the arithmetic the
// kernels share with the host (md_mol_math.h); tests/test_mol_plan_cpu.py compiles and runs it.
//   mol_shim consts                  prints: the largest and the default tile capacity
//   mol_shim plan < input            prints the plan, one named array per line, or "error <message>"
//   mol_shim sums|scale f|d < input  runs what the kernel of that name does tile by tile, serially, in float or double
//                                    arithmetic; sums prints the 18 words, scale prints r, v (n_atoms x 3 each)
// input (whitespace separated): n_atoms tile_atoms, the labels (n_atoms); for the two runs also: box (9, rows), mu_minus_1
// inv_mu_minus_1, then per atom r (3), v (3), gradient (3), inv_mass
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "md_mol_math.h"
#include "mol_plan.h"

namespace {

struct Input {
  int n_atoms = 0, tile_atoms = 0;
  std::vector<int32_t> labels;
};

bool read_labels(Input& in) {
  if (scanf("%d %d", &in.n_atoms, &in.tile_atoms) != 2 || in.n_atoms < 0 || in.n_atoms > (1 << 24)) return false;
  in.labels.resize((size_t)in.n_atoms + 1);
  for (int k = 0; k < in.n_atoms; ++k)
    if (scanf("%d", &in.labels[k]) != 1) return false;
  return true;
}

void print_ints(const char* name, const std::vector<int>& v) {
  printf("%s", name);
  for (int x : v) printf(" %d", x);
  printf("\n");
}

int run_plan() {
  Input in;
  if (!read_labels(in)) return 2;
  const admp::MolPlan p = admp::mol_make_plan(in.n_atoms, in.labels.data(), in.tile_atoms);
  if (!p.error.empty()) { printf("error %s\n", p.error.c_str()); return 0; }
  printf("scalars %d %d %d %d %d %d %d %zu %zu %d\n", p.n_atoms, p.tile_atoms, p.n_tiles, p.n_groups, p.max_group, p.dims.atoms,
         p.dims.groups, admp::mol_lds_bytes(p.dims, sizeof(float)), admp::mol_lds_bytes(p.dims, sizeof(double)),
         admp::mts_threads(p.tile_atoms));
  print_ints("tile_atom0", p.tile_atom0); print_ints("atom_id", p.atom_id); print_ints("tile_grp0", p.tile_grp0);
  print_ints("grp_atom0", p.grp_atom0); print_ints("slot_grp", p.slot_grp);
  return 0;
}

// what a workgroup of k_md_mol_sums (op 0) or k_md_mol_scale (1) does with tile t, one atom after the other
template <class T>
void tile_run(int op, const admp::MolPlan& p, int t, const admp::Box<T>& box, double mu_m1, double inv_mu_m1, std::vector<T>& R,
              std::vector<T>& V, const std::vector<T>& G, const std::vector<T>& IM, double acc[18]) {
  const int a0 = p.tile_atom0[t], n = p.tile_atom0[t + 1] - a0, g0 = p.tile_grp0[t], ng = p.tile_grp0[t + 1] - g0;
  std::vector<T> d(3 * (size_t)n + 1), v(3 * (size_t)n + 1), s(3 * (size_t)n + 1), ra(3 * (size_t)n + 1), im((size_t)n + 1);
  std::vector<double> grp(admp::kMolGroupWords * (size_t)ng + 1);
  for (int l = 0; l < n; ++l) {
    const int atom = p.atom_id[a0 + l], anchor = p.atom_id[p.grp_atom0[g0 + p.slot_grp[a0 + l]]];
    for (int c = 0; c < 3; ++c) { ra[3 * l + c] = R[3 * (size_t)anchor + c]; v[3 * l + c] = V[3 * (size_t)atom + c]; }
    admp::md_mol_image(box, &R[3 * (size_t)atom], &ra[3 * l], &d[3 * l], &s[3 * l]);
    im[l] = IM[atom];
  }
  for (int g = 0; g < ng; ++g)
    admp::md_mol_group(d.data(), v.data(), im.data(), p.grp_atom0[g0 + g] - a0, p.grp_atom0[g0 + g + 1] - a0, &grp[admp::kMolGroupWords * g]);
  if (op == 0)
    for (int g = 0; g < ng; ++g) {
      const double* w = &grp[admp::kMolGroupWords * g];
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) acc[3 * a + b] += w[0] * w[4 + a] * w[4 + b];
    }
  for (int l = 0; l < n; ++l) {
    const int atom = p.atom_id[a0 + l];
    const double* w = &grp[admp::kMolGroupWords * p.slot_grp[a0 + l]];
    double Rc[3];
    admp::md_mol_centre(&ra[3 * l], w, &s[3 * l], Rc);
    if (op == 0) {
      for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) acc[9 + 3 * a + b] += Rc[a] * (double)G[3 * (size_t)atom + b];
    } else {
      admp::md_mol_scale(&R[3 * (size_t)atom], &V[3 * (size_t)atom], Rc, w, mu_m1, inv_mu_m1);
    }
  }
}

template <class T>
int run(int op) {
  Input in;
  if (!read_labels(in)) return 2;
  double h[9], inv[9], mu_m1, inv_mu_m1;
  for (double& x : h)
    if (scanf("%lf", &x) != 1) return 2;
  if (scanf("%lf %lf", &mu_m1, &inv_mu_m1) != 2) return 2;
  const size_t n = (size_t)in.n_atoms;
  std::vector<T> R(3 * n + 1), V(3 * n + 1), G(3 * n + 1), IM(n + 1);
  for (size_t i = 0; i < n; ++i) {
    double x[10];
    for (double& y : x)
      if (scanf("%lf", &y) != 1) return 2;
    for (int c = 0; c < 3; ++c) { R[3 * i + c] = (T)x[c]; V[3 * i + c] = (T)x[3 + c]; G[3 * i + c] = (T)x[6 + c]; }
    IM[i] = (T)x[9];
  }
  const admp::MolPlan p = admp::mol_make_plan(in.n_atoms, in.labels.data(), in.tile_atoms);
  if (!p.error.empty()) { printf("error %s\n", p.error.c_str()); return 0; }
  const double det = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
  inv[0] = (h[4] * h[8] - h[5] * h[7]) / det; inv[1] = (h[2] * h[7] - h[1] * h[8]) / det; inv[2] = (h[1] * h[5] - h[2] * h[4]) / det;
  inv[3] = (h[5] * h[6] - h[3] * h[8]) / det; inv[4] = (h[0] * h[8] - h[2] * h[6]) / det; inv[5] = (h[2] * h[3] - h[0] * h[5]) / det;
  inv[6] = (h[3] * h[7] - h[4] * h[6]) / det; inv[7] = (h[1] * h[6] - h[0] * h[7]) / det; inv[8] = (h[0] * h[4] - h[1] * h[3]) / det;
  admp::Box<T> box;
  for (int k = 0; k < 9; ++k) { box.h[k] = (T)h[k]; box.hinv[k] = (T)inv[k]; }
  double acc[18];
  for (double& x : acc) x = 0.0;
  // scaling in place is safe tile by tile: a tile reads only its own atoms (the anchors are its own)
  for (int t = 0; t < p.n_tiles; ++t) tile_run<T>(op, p, t, box, mu_m1, inv_mu_m1, R, V, G, IM, acc);
  if (op == 0) {
    for (double x : acc) printf("%.17g\n", x);
  } else {
    for (const std::vector<T>* q : {&R, &V})
      for (size_t i = 0; i < n; ++i) printf("%.17g %.17g %.17g\n", (double)(*q)[3 * i], (double)(*q)[3 * i + 1], (double)(*q)[3 * i + 2]);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "consts")) {
    printf("%d %d\n", admp::kMolMaxTileAtoms, admp::kMolDefaultTileAtoms);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "plan")) return run_plan();
  if (argc == 3 && (argv[2][0] == 'f' || argv[2][0] == 'd')) {
    const int op = !strcmp(argv[1], "sums") ? 0 : (!strcmp(argv[1], "scale") ? 1 : -1);
    if (op >= 0) return argv[2][0] == 'f' ? run<float>(op) : run<double>(op);
  }
  fprintf(stderr, "usage: %s consts | plan | sums|scale f|d   (input on stdin)\n", argv[0]);
  return 2;
}
