// Stand-alone host program over the plan of the multiple-time-step kernel (admp_amd/csrc/mts_plan.h) and the arithmetic the
// kernel shares with the host (md_bonded_math.h, md_math.h); tests/test_mts_plan_cpu.py compiles and runs it.
//   mts_shim consts                prints: the largest and the default tile capacity
//   mts_shim plan < input          prints the plan, one named array per line, or "error <message>"
//   mts_shim step f|d < input      runs one outer step tile by tile, serially, in float or double arithmetic, and prints
//                                  r, v, the bonded gradient at the returned r (n_atoms x 3 each) and the two energy words
// input (whitespace separated): n_atoms tile_atoms n_bonds n_angles, bonds (i j k r0 each), angles (i j k k_theta theta0 each);
// for step also: box (9, rows), n_inner, half_dt_acc_outer, dt_outer, c1, c2sq_kT_acc, seed, outer_step, then per atom
// r (3), v (3), grad_slow (3), inv_mass
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "md_bonded_math.h"
#include "mts_plan.h"

namespace {

struct Input {
  int n_atoms = 0, tile_atoms = 0, nb = 0, na = 0;
  std::vector<int32_t> bonds, angles;
  std::vector<double> bpar, apar;
};

bool read_lists(Input& in) {
  if (scanf("%d %d %d %d", &in.n_atoms, &in.tile_atoms, &in.nb, &in.na) != 4 || in.nb < 0 || in.na < 0) return false;
  in.bonds.resize(2 * (size_t)in.nb); in.bpar.resize(2 * (size_t)in.nb);
  in.angles.resize(3 * (size_t)in.na); in.apar.resize(2 * (size_t)in.na);
  for (int b = 0; b < in.nb; ++b)
    if (scanf("%d %d %lf %lf", &in.bonds[2 * b], &in.bonds[2 * b + 1], &in.bpar[2 * b], &in.bpar[2 * b + 1]) != 4) return false;
  for (int a = 0; a < in.na; ++a)
    if (scanf("%d %d %d %lf %lf", &in.angles[3 * a], &in.angles[3 * a + 1], &in.angles[3 * a + 2], &in.apar[2 * a], &in.apar[2 * a + 1]) != 5)
      return false;
  return true;
}

admp::MtsPlan plan_of(const Input& in) {
  return admp::mts_make_plan(in.n_atoms, in.nb, in.bonds.data(), in.bpar.data(), in.na, in.angles.data(), in.apar.data(), in.tile_atoms);
}

void print_ints(const char* name, const std::vector<int>& v) {
  printf("%s", name);
  for (int x : v) printf(" %d", x);
  printf("\n");
}
void print_reals(const char* name, const std::vector<double>& v) {
  printf("%s", name);
  for (double x : v) printf(" %.17g", x);
  printf("\n");
}

int run_plan() {
  Input in;
  if (!read_lists(in)) return 2;
  const admp::MtsPlan p = plan_of(in);
  if (!p.error.empty()) { printf("error %s\n", p.error.c_str()); return 0; }
  printf("scalars %d %d %d %d %d %d %d %d %d %d %zu\n", p.n_atoms, p.tile_atoms, p.n_tiles, p.max_component, p.n_bonds, p.n_angles,
         p.dims.atoms, p.dims.bonds, p.dims.angles, p.dims.refs, admp::mts_lds_bytes(p.dims, sizeof(double)));
  print_ints("tile_atom0", p.tile_atom0); print_ints("atom_id", p.atom_id);
  print_ints("tile_bond0", p.tile_bond0); print_ints("bond_slot", p.bond_slot); print_reals("bond_par", p.bond_par);
  print_ints("tile_angle0", p.tile_angle0); print_ints("angle_slot", p.angle_slot); print_reals("angle_par", p.angle_par);
  print_ints("ref0", p.ref0); print_ints("ref", p.ref);
  return 0;
}

// what a workgroup of k_md_mts does with tile t, one atom after the other
template <class T>
void tile_step(const admp::MtsPlan& p, int t, const admp::Box<T>& box, T hdo, T hdi, T hd, int n_inner, T c1, T c2sq, uint64_t seed,
               uint64_t step0, std::vector<T>& R, std::vector<T>& V, const std::vector<T>& GS, const std::vector<T>& IM, std::vector<T>& F,
               double E[2]) {
  const int a0 = p.tile_atom0[t], n = p.tile_atom0[t + 1] - a0;
  const int b0 = p.tile_bond0[t], nb = p.tile_bond0[t + 1] - b0, g0 = p.tile_angle0[t], na = p.tile_angle0[t + 1] - g0;
  std::vector<T> r(3 * (size_t)n), v(3 * (size_t)n), f(3 * (size_t)n), slots(3 * ((size_t)nb + 2 * (size_t)na));
  for (int a = 0; a < n; ++a) {
    const int atom = p.atom_id[a0 + a];
    for (int c = 0; c < 3; ++c) { r[3 * a + c] = R[3 * (size_t)atom + c]; v[3 * a + c] = V[3 * (size_t)atom + c]; }
    admp::md_mts_kick(&v[3 * a], &GS[3 * (size_t)atom], IM[atom], hdo);
  }
  const bool noisy = c1 < T(1);
  double eb = 0.0, ea = 0.0;
  for (int k = 0; k <= n_inner; ++k) {
    if (k > 0)
      for (int a = 0; a < n; ++a) {
        const int atom = p.atom_id[a0 + a];
        admp::md_mts_kick(&v[3 * a], &f[3 * a], IM[atom], hdi);
        admp::md_mts_drift(&r[3 * a], &v[3 * a], hd, noisy, c1, admp::m_sqrt(c2sq * IM[atom]), seed, step0 + (uint64_t)(k - 1), (uint32_t)atom);
      }
    eb = ea = 0.0;
    for (int i = 0; i < nb; ++i) {
      const int* s = &p.bond_slot[2 * ((size_t)b0 + i)];
      eb += admp::md_bond_item(box, &r[3 * s[0]], &r[3 * s[1]], (T)p.bond_par[2 * ((size_t)b0 + i)], (T)p.bond_par[2 * ((size_t)b0 + i) + 1], &slots[3 * i]);
    }
    for (int i = 0; i < na; ++i) {
      const int* s = &p.angle_slot[3 * ((size_t)g0 + i)];
      T* o = &slots[3 * (nb + 2 * i)];
      ea += admp::md_angle_item(box, &r[3 * s[0]], &r[3 * s[1]], &r[3 * s[2]], (T)p.angle_par[2 * ((size_t)g0 + i)],
                                (T)p.angle_par[2 * ((size_t)g0 + i) + 1], o, o + 3);
    }
    for (int a = 0; a < n; ++a) {
      const int atom = p.atom_id[a0 + a];
      T* fa = &f[3 * a];
      fa[0] = fa[1] = fa[2] = T(0);
      for (int q = p.ref0[a0 + a]; q < p.ref0[a0 + a + 1]; ++q) admp::md_mts_add_ref(slots.data(), p.ref[q], fa);
      if (k > 0) admp::md_mts_kick(&v[3 * a], fa, IM[atom], hdi);
    }
  }
  for (int a = 0; a < n; ++a) {
    const int atom = p.atom_id[a0 + a];
    for (int c = 0; c < 3; ++c) { R[3 * (size_t)atom + c] = r[3 * a + c]; V[3 * (size_t)atom + c] = v[3 * a + c]; F[3 * (size_t)atom + c] = f[3 * a + c]; }
  }
  E[0] += eb; E[1] += ea;
}

template <class T>
int run_step() {
  Input in;
  if (!read_lists(in)) return 2;
  double h[9], inv[9], hdo, dt, c1, c2sq;
  int n_inner;
  unsigned long long seed, outer;
  for (double& x : h)
    if (scanf("%lf", &x) != 1) return 2;
  if (scanf("%d %lf %lf %lf %lf %llu %llu", &n_inner, &hdo, &dt, &c1, &c2sq, &seed, &outer) != 7 || n_inner < 1) return 2;
  const size_t n = (size_t)in.n_atoms;
  std::vector<T> R(3 * n), V(3 * n), GS(3 * n), IM(n), F(3 * n, T(0));
  for (size_t i = 0; i < n; ++i) {
    double x[10];
    for (double& y : x)
      if (scanf("%lf", &y) != 1) return 2;
    for (int c = 0; c < 3; ++c) { R[3 * i + c] = (T)x[c]; V[3 * i + c] = (T)x[3 + c]; GS[3 * i + c] = (T)x[6 + c]; }
    IM[i] = (T)x[9];
  }
  const admp::MtsPlan p = plan_of(in);
  if (!p.error.empty()) { printf("error %s\n", p.error.c_str()); return 0; }
  const double det = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
  inv[0] = (h[4] * h[8] - h[5] * h[7]) / det; inv[1] = (h[2] * h[7] - h[1] * h[8]) / det; inv[2] = (h[1] * h[5] - h[2] * h[4]) / det;
  inv[3] = (h[5] * h[6] - h[3] * h[8]) / det; inv[4] = (h[0] * h[8] - h[2] * h[6]) / det; inv[5] = (h[2] * h[3] - h[0] * h[5]) / det;
  inv[6] = (h[3] * h[7] - h[4] * h[6]) / det; inv[7] = (h[1] * h[6] - h[0] * h[7]) / det; inv[8] = (h[0] * h[4] - h[1] * h[3]) / det;
  admp::Box<T> box;
  for (int k = 0; k < 9; ++k) { box.h[k] = (T)h[k]; box.hinv[k] = (T)inv[k]; }
  double E[2] = {0.0, 0.0};
  for (int t = 0; t < p.n_tiles; ++t)      // (the roundings of the launcher: launch_md_mts)
    tile_step<T>(p, t, box, (T)hdo, (T)(hdo / n_inner), (T)(0.5 * dt / n_inner), n_inner, (T)c1, (T)c2sq, (uint64_t)seed,
                 (uint64_t)outer * (uint64_t)n_inner, R, V, GS, IM, F, E);
  for (const std::vector<T>* a : {&R, &V, &F})
    for (size_t i = 0; i < n; ++i) printf("%.17g %.17g %.17g\n", (double)(*a)[3 * i], (double)(*a)[3 * i + 1], (double)(*a)[3 * i + 2]);
  printf("%.17g %.17g\n", E[0], E[1]);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "consts")) {
    printf("%d %d\n", admp::kMtsMaxTileAtoms, admp::kMtsDefaultTileAtoms);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "plan")) return run_plan();
  if (argc == 3 && !strcmp(argv[1], "step") && (argv[2][0] == 'f' || argv[2][0] == 'd')) return argv[2][0] == 'f' ? run_step<float>() : run_step<double>();
  fprintf(stderr, "usage: %s consts | plan | step f|d   (input on stdin)\n", argv[0]);
  return 2;
}
