// Stand-alone host program over the plan of the constraint kernels (admp_amd/csrc/con_plan.h) and the arithmetic the kernels
// share with the host (md_con_math.h); tests/test_con_plan_cpu.py compiles and runs it.
//   con_shim consts                          prints: the largest and the default tile capacity
//   con_shim plan < input                    prints the plan, one named array per line, or "error <message>"
//   con_shim step|kick|project f|d < input   runs what the kernel of that name does tile by tile, serially, in float or double
//                                            arithmetic, and prints r, v (n_atoms x 3 each), then: failed clusters, most sweeps
//                                            of a cluster, sum m v^2 / 2
// input (whitespace separated): n_atoms tile_atoms n_constraints, constraints (i j d each); for the three runs also: box (9,
// rows), half_dt_acc dt c1 c2sq_kT_acc seed step tolerance max_sweeps with_gradient, then per atom a (3), b (3), c (3),
// inv_mass -- step: a = r, b = v, c = gradient; kick: the same (c ignored without a gradient); project: a = r, b = reference
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "con_plan.h"
#include "md_con_math.h"

namespace {

struct Input {
  int n_atoms = 0, tile_atoms = 0, nc = 0;
  std::vector<int32_t> pairs;
  std::vector<double> lengths;
};

bool read_lists(Input& in) {
  if (scanf("%d %d %d", &in.n_atoms, &in.tile_atoms, &in.nc) != 3 || in.nc < 0) return false;
  in.pairs.resize(2 * (size_t)in.nc + 1); in.lengths.resize((size_t)in.nc + 1);
  for (int k = 0; k < in.nc; ++k)
    if (scanf("%d %d %lf", &in.pairs[2 * k], &in.pairs[2 * k + 1], &in.lengths[k]) != 3) return false;
  return true;
}

void print_ints(const char* name, const std::vector<int>& v) {
  printf("%s", name);
  for (int x : v) printf(" %d", x);
  printf("\n");
}

int run_plan() {
  Input in;
  if (!read_lists(in)) return 2;
  const admp::ConPlan p = admp::con_make_plan(in.n_atoms, in.nc, in.pairs.data(), in.lengths.data(), in.tile_atoms);
  if (!p.error.empty()) { printf("error %s\n", p.error.c_str()); return 0; }
  printf("scalars %d %d %d %d %d %d %d %d %d %zu %zu\n", p.n_atoms, p.tile_atoms, p.n_tiles, p.n_clusters, p.max_cluster, p.n_cons,
         p.dims.atoms, p.dims.clusters, p.dims.cons, admp::con_lds_bytes(p.dims, sizeof(double), false),
         admp::con_lds_bytes(p.dims, sizeof(double), true));
  print_ints("tile_atom0", p.tile_atom0); print_ints("atom_id", p.atom_id); print_ints("tile_clu0", p.tile_clu0);
  print_ints("clu_atom0", p.clu_atom0); print_ints("clu_con0", p.clu_con0); print_ints("con_slot", p.con_slot);
  print_ints("con_order", p.con_order);
  printf("con_d2");
  for (double x : p.con_d2) printf(" %.17g", x);
  printf("\n");
  return 0;
}

template <class T>
struct Args {
  admp::Box<T> box;
  T half_dt_acc, half_dt, dt, c1, c2sq, tol2, tol_dt;      // (the roundings of the launchers of con_kernels.hip)
  uint64_t seed, step;
  int max_sweeps;
  bool with_grad;
};

// what a workgroup of k_con_step (op 0), k_con_kick (1) or k_con_project (2) does with tile t, one atom after the other
template <class T>
void tile_run(int op, const admp::ConPlan& p, int t, const Args<T>& a, std::vector<T>& A, std::vector<T>& B, const std::vector<T>& C,
              const std::vector<T>& IM, long& failures, int& most, double& ekin) {
  const int a0 = p.tile_atom0[t], n = p.tile_atom0[t + 1] - a0, k0 = p.tile_clu0[t], ncl = p.tile_clu0[t + 1] - k0;
  const int q0 = p.clu_con0[k0], nq = p.clu_con0[k0 + ncl] - q0;
  std::vector<T> x(3 * (size_t)n + 1), ref(3 * (size_t)n + 1), im((size_t)n + 1), d2((size_t)nq + 1), s(3 * (size_t)nq + 1),
      b(3 * (size_t)nq + 1), v(3 * (size_t)n + 1), du(3 * (size_t)n + 1);
  std::vector<int> slot(p.con_slot.begin() + 2 * (size_t)q0, p.con_slot.begin() + 2 * ((size_t)q0 + nq));
  slot.push_back(0);
  for (int q = 0; q < nq; ++q) d2[q] = (T)p.con_d2[(size_t)q0 + q];
  for (int l = 0; l < n; ++l) {
    const int atom = p.atom_id[a0 + l];
    im[l] = IM[atom];
    for (int c = 0; c < 3; ++c) {
      x[3 * l + c] = A[3 * (size_t)atom + c];
      if (op == 2) ref[3 * l + c] = B[3 * (size_t)atom + c]; else v[3 * l + c] = B[3 * (size_t)atom + c];
    }
    if (op == 0)
      admp::md_con_half_step(&v[3 * l], &du[3 * l], &C[3 * (size_t)atom], im[l], a.half_dt_acc, a.half_dt, a.c1 < T(1), a.c1,
                             admp::m_sqrt(a.c2sq * im[l]), a.seed, a.step, (uint32_t)atom);
    if (op == 1 && a.with_grad) admp::md_mts_kick(&v[3 * l], &C[3 * (size_t)atom], im[l], a.half_dt_acc);
  }
  for (int q = 0; q < nq; ++q) {
    admp::md_con_vector(a.box, &x[3 * slot[2 * q]], &x[3 * slot[2 * q + 1]], &b[3 * q]);
    if (op == 2) admp::md_con_vector(a.box, &ref[3 * slot[2 * q]], &ref[3 * slot[2 * q + 1]], &s[3 * q]);
    else for (int c = 0; c < 3; ++c) s[3 * q + c] = b[3 * q + c];
  }
  // the solved vector: the displacement of the half step (step), the velocity (kick), a displacement from zero (project)
  std::vector<T> d(du);
  if (op == 2) d.assign(3 * (size_t)n + 1, T(0));
  T* solved = op == 1 ? v.data() : d.data();
  for (int c = 0; c < ncl; ++c) {
    bool failed = false;
    const int c0 = p.clu_con0[k0 + c] - q0, c1 = p.clu_con0[k0 + c + 1] - q0;
    const int sweeps = op == 1 ? admp::md_con_solve_rattle(solved, im.data(), slot.data(), d2.data(), s.data(), c0, c1, a.tol_dt, a.max_sweeps, failed)
                               : admp::md_con_solve_shake(solved, im.data(), slot.data(), d2.data(), s.data(), b.data(), c0, c1, a.tol2,
                                                          a.max_sweeps, failed);
    failures += failed ? 1 : 0;
    most = sweeps > most ? sweeps : most;
  }
  for (int l = 0; l < n; ++l) {
    const int atom = p.atom_id[a0 + l];
    if (op == 0) {
      T r[3];
      admp::md_con_finish(r, &v[3 * l], &x[3 * l], &d[3 * l], &du[3 * l], a.dt);
      for (int c = 0; c < 3; ++c) { A[3 * (size_t)atom + c] = r[c]; B[3 * (size_t)atom + c] = v[3 * l + c]; }
    } else if (op == 1) {
      for (int c = 0; c < 3; ++c) {
        B[3 * (size_t)atom + c] = v[3 * l + c];
        ekin += 0.5 * (double)v[3 * l + c] * (double)v[3 * l + c] / (double)im[l];
      }
    } else {
      for (int c = 0; c < 3; ++c) A[3 * (size_t)atom + c] = x[3 * l + c] + d[3 * l + c];
    }
  }
}

template <class T>
int run(int op) {
  Input in;
  if (!read_lists(in)) return 2;
  double h[9], inv[9], hda, dt, c1, c2sq, tol;
  unsigned long long seed, step;
  int max_sweeps, with_grad;
  for (double& x : h)
    if (scanf("%lf", &x) != 1) return 2;
  if (scanf("%lf %lf %lf %lf %llu %llu %lf %d %d", &hda, &dt, &c1, &c2sq, &seed, &step, &tol, &max_sweeps, &with_grad) != 9) return 2;
  if (!(dt > 0.0) || max_sweeps < 1 || !(tol >= 0.0)) return 2;
  const size_t n = in.n_atoms > 0 ? (size_t)in.n_atoms : 0;
  std::vector<T> A(3 * n + 1), B(3 * n + 1), C(3 * n + 1), IM(n + 1);
  for (size_t i = 0; i < n; ++i) {
    double x[10];
    for (double& y : x)
      if (scanf("%lf", &y) != 1) return 2;
    for (int c = 0; c < 3; ++c) { A[3 * i + c] = (T)x[c]; B[3 * i + c] = (T)x[3 + c]; C[3 * i + c] = (T)x[6 + c]; }
    IM[i] = (T)x[9];
  }
  const admp::ConPlan p = admp::con_make_plan(in.n_atoms, in.nc, in.pairs.data(), in.lengths.data(), in.tile_atoms);
  if (!p.error.empty()) { printf("error %s\n", p.error.c_str()); return 0; }
  const double det = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
  inv[0] = (h[4] * h[8] - h[5] * h[7]) / det; inv[1] = (h[2] * h[7] - h[1] * h[8]) / det; inv[2] = (h[1] * h[5] - h[2] * h[4]) / det;
  inv[3] = (h[5] * h[6] - h[3] * h[8]) / det; inv[4] = (h[0] * h[8] - h[2] * h[6]) / det; inv[5] = (h[2] * h[3] - h[0] * h[5]) / det;
  inv[6] = (h[3] * h[7] - h[4] * h[6]) / det; inv[7] = (h[1] * h[6] - h[0] * h[7]) / det; inv[8] = (h[0] * h[4] - h[1] * h[3]) / det;
  Args<T> a;
  for (int k = 0; k < 9; ++k) { a.box.h[k] = (T)h[k]; a.box.hinv[k] = (T)inv[k]; }
  a.half_dt_acc = (T)hda; a.half_dt = (T)(0.5 * dt); a.dt = (T)dt; a.c1 = (T)c1; a.c2sq = (T)c2sq;
  a.tol2 = (T)(2.0 * tol); a.tol_dt = (T)(tol / dt);
  a.seed = (uint64_t)seed; a.step = (uint64_t)step; a.max_sweeps = max_sweeps; a.with_grad = with_grad != 0;
  long failures = 0;
  int most = 0;
  double ekin = 0.0;
  for (int t = 0; t < p.n_tiles; ++t) tile_run<T>(op, p, t, a, A, B, C, IM, failures, most, ekin);
  for (const std::vector<T>* q : {&A, &B})
    for (size_t i = 0; i < n; ++i) printf("%.17g %.17g %.17g\n", (double)(*q)[3 * i], (double)(*q)[3 * i + 1], (double)(*q)[3 * i + 2]);
  printf("%ld %d %.17g\n", failures, most, ekin);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "consts")) {
    printf("%d %d\n", admp::kConMaxTileAtoms, admp::kConDefaultTileAtoms);
    return 0;
  }
  if (argc == 2 && !strcmp(argv[1], "plan")) return run_plan();
  if (argc == 3 && (argv[2][0] == 'f' || argv[2][0] == 'd')) {
    const int op = !strcmp(argv[1], "step") ? 0 : (!strcmp(argv[1], "kick") ? 1 : (!strcmp(argv[1], "project") ? 2 : -1));
    if (op >= 0) return argv[2][0] == 'f' ? run<float>(op) : run<double>(op);
  }
  fprintf(stderr, "usage: %s consts | plan | step|kick|project f|d   (input on stdin)\n", argv[0]);
  return 2;
}
