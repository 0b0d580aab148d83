// Host program around admp_amd/csrc/disp_plan.h for tests/test_disp_plan_cpu.py: reads rows of the eleven inputs of disp_path
// (snranks use_dft use_pfa use_fx bricks single_precision nch disp_nt have_types types_on batch_on) and prints the path of each.
#include <cstdio>

#include "disp_plan.h"

int main() {
  int v[11];
  for (;;) {
    for (int k = 0; k < 11; ++k)
      if (std::scanf("%d", &v[k]) != 1) return k == 0 ? 0 : 1;      // (a partial row is an error)
    admp::DispPathIn in;
    in.snranks = v[0];
    in.use_dft = v[1] != 0; in.use_pfa = v[2] != 0; in.use_fx = v[3] != 0; in.bricks = v[4] != 0;
    in.single_precision = v[5] != 0;
    in.nch = v[6]; in.disp_nt = v[7];
    in.have_types = v[8] != 0; in.types_on = v[9] != 0; in.batch_on = v[10] != 0;
    std::puts(admp::disp_path_name(admp::disp_path(in)));
  }
}
