// Host program around admp_amd/csrc/mesh_path.h for tests/test_mesh_path_cpu.py: reads rows of the ten inputs of mesh_path
// (K0 K1 K2 snranks dft_mode pfa_on fused_x_on fftx_ok splits zy_fits) and prints the path of each.
#include <cstdio>

#include "mesh_path.h"

int main() {
  int v[10];
  for (;;) {
    for (int k = 0; k < 10; ++k)
      if (std::scanf("%d", &v[k]) != 1) return k == 0 ? 0 : 1;      // (a partial row is an error)
    admp::MeshPathIn in;
    for (int d = 0; d < 3; ++d) in.K[d] = v[d];
    in.snranks = v[3];
    in.dft_mode = v[4];
    in.pfa_on = v[5] != 0; in.fused_x_on = v[6] != 0; in.fftx_ok = v[7] != 0; in.splits = v[8] != 0; in.zy_fits = v[9] != 0;
    std::puts(admp::mesh_path_name(admp::mesh_path(in)));
  }
}
