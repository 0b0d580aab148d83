// Stand-alone host program over the predictor-corrector arithmetic of the engine (admp_amd/csrc/scf_aspc.h: coefficient table,
// omega, argument checks, the ring of dipole sets); tests/test_scf_aspc_cpu.py compiles and runs it.
//   aspc_shim table            per order one line: k  B_1 .. B_{k+2} as num/den  omega as num/den  omega as %.17g
//   aspc_shim predict k        reads k + 2 doubles U(n-1) .. U(n-k-2), prints sum_j B_j U(n-j) accumulated in double from j = 1
//                              upwards, as the predictor kernel does
//   aspc_shim script           runs commands from stdin against one AspcRing whose slots hold an integer tag each:
//                                cfg ORDER N_CORRECTOR OMEGA   -> "ok" or "refused"        (OMEGA: a number, or nan)
//                                push TAG                      -> writes TAG to next_slot(), then push(); prints the slot
//                                drop                          -> drop()
//                                state                         -> on order n_corrector omega slots count full next_slot | tags of U(n-1) ..
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "scf_aspc.h"

namespace {

int run_table() {
  for (int k = 0; k <= kAspcMaxOrder; ++k) {
    printf("%d", k);
    for (int j = 1; j <= aspc_sets(k); ++j) printf(" %d/%d", aspc_coef_frac(k, j).num, aspc_coef_frac(k, j).den);
    printf(" %d/%d %.17g\n", aspc_omega_frac(k).num, aspc_omega_frac(k).den, aspc_omega(k));
  }
  printf("limits %d %d %d\n", kAspcMaxOrder, kAspcMaxSets, kScfChainSteps);
  return 0;
}

int run_predict(int k) {
  if (k < 0 || k > kAspcMaxOrder) return 2;
  double acc = 0.0;
  for (int j = 1; j <= aspc_sets(k); ++j) {
    double u;
    if (scanf("%lf", &u) != 1) return 2;
    acc += aspc_coef(k, j) * u;
  }
  printf("%.17g\n", acc);
  return 0;
}

int run_script() {
  AspcRing ring;
  long tags[kAspcMaxSets] = {0, 0, 0, 0, 0, 0};
  char cmd[32];
  while (scanf("%31s", cmd) == 1) {
    if (!strcmp(cmd, "cfg")) {
      int order, nc;
      char om[64];
      if (scanf("%d %d %63s", &order, &nc, om) != 3) return 2;
      const double omega = !strcmp(om, "nan") ? std::nan("") : atof(om);
      printf("%s\n", ring.configure(order, nc, omega) ? "ok" : "refused");
    } else if (!strcmp(cmd, "push")) {
      long tag;
      if (scanf("%ld", &tag) != 1 || !ring.on()) return 2;
      const int s = ring.next_slot();
      if (s < 0 || s >= ring.slots()) return 3;
      tags[s] = tag;
      ring.push();
      printf("%d\n", s);
    } else if (!strcmp(cmd, "drop")) {
      ring.drop();
    } else if (!strcmp(cmd, "state")) {
      printf("%d %d %d %.17g %d %d %d %d |", ring.on() ? 1 : 0, ring.order(), ring.n_corrector(), ring.omega(), ring.slots(),
             ring.count(), ring.full() ? 1 : 0, ring.on() ? ring.next_slot() : -1);
      for (int j = 1; j <= ring.count(); ++j) printf(" %ld", tags[ring.slot(j)]);
      printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "table")) return run_table();
  if (argc == 3 && !strcmp(argv[1], "predict")) return run_predict(atoi(argv[2]));
  if (argc == 2 && !strcmp(argv[1], "script")) return run_script();
  fprintf(stderr, "usage: %s table | predict k | script   (input on stdin)\n", argv[0]);
  return 2;
}
