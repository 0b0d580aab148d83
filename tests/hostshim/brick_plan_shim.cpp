// Host build of the brick rule of the LDS-tiled spread (admp_amd/csrc/brick_plan.h); tests/test_mesh_ref_cpu.py.
#include <cstdint>

#include "../../admp_amd/csrc/brick_plan.h"

extern "C" {
void brick_plan_grid(const int32_t* K, int32_t* nb4) {
  const int k[3] = {K[0], K[1], K[2]};
  const admp::BrickGrid b = admp::make_bricks(k);
  nb4[0] = b.nb[0]; nb4[1] = b.nb[1]; nb4[2] = b.nb[2]; nb4[3] = b.ncell;
}
int brick_plan_of(int i, int nb, int K) { return admp::brick_of(i, nb, K); }
void brick_plan_codes(int n, const int32_t* bases, const int32_t* K, int32_t* codes) {
  const int k[3] = {K[0], K[1], K[2]};
  const admp::BrickGrid b = admp::make_bricks(k);
  for (int i = 0; i < n; ++i) {
    const int base[3] = {bases[3 * i], bases[3 * i + 1], bases[3 * i + 2]};
    codes[i] = admp::brick_code(base, k, b);
  }
}
}
