// Host build of the cell-list plan (admp_amd/csrc/cell_plan.h): the cell-grid rule and the size of the row kernels'
// partial-count buffer; tests/test_neighbour_ref_cpu.py.
#include <cstdint>

#include "../../admp_amd/csrc/cell_plan.h"

extern "C" {
void cell_plan_dims(const double* heights, double rc, int32_t* n) {
  int m[3];
  admp::cell_grid_dims(heights, rc, m);
  n[0] = m[0]; n[1] = m[1]; n[2] = m[2];
}
int64_t cell_plan_partial_words(int na) { return (int64_t)admp::cell_partial_words(na); }
int cell_plan_brute_max() { return admp::kBruteMax; }
}
