// Host build of the block-id layout of the x pass that carries the closing pair kernel (admp_amd/csrc/rider_layout.h) and of
// the x pass's launch plan (admp_amd/csrc/dft_plan.h); tests/test_pair_rider_layout_cpu.py.
#include <cstdint>

#include "../../admp_amd/csrc/dft_plan.h"
#include "../../admp_amd/csrc/rider_layout.h"

using namespace admp;

extern "C" {
unsigned rider_blocks(unsigned npair, unsigned nind, unsigned nbx, unsigned ny) {
  RiderGrid g;
  g.npair = npair; g.nind = nind; g.nbx = nbx; g.ny = ny;
  return rider_grid_blocks(g);
}
// out[4 * (by * gdx + bx) ..] = kind, rank, tile, y row for every block of a (gdx, gdy) grid
void rider_map(unsigned npair, unsigned nind, unsigned nbx, unsigned ny, unsigned gdx, unsigned gdy, int64_t* out) {
  RiderGrid g;
  g.npair = npair; g.nind = nind; g.nbx = nbx; g.ny = ny;
  for (unsigned by = 0; by < gdy; ++by)
    for (unsigned bx = 0; bx < gdx; ++bx) {
      const RiderBlock b = rider_block(g, bx, by, gdx);
      int64_t* o = out + 4 * ((int64_t)by * gdx + bx);
      o[0] = b.kind; o[1] = b.rank; o[2] = b.bx; o[3] = b.by;
    }
}
// out[6] = N, Kh, TK, NC, nbx, dynamic LDS bytes of the x pass of mesh (k0, k1, k2) in words of w bytes
void x_pass_plan(int k0, int k1, int k2, int w, int circ, int64_t* out) {
  const int K[3] = {k0, k1, k2};
  const XPassPlan p = dft_x_plan(K, (size_t)w, circ != 0);
  out[0] = p.N; out[1] = p.Kh; out[2] = p.TK; out[3] = p.NC; out[4] = p.nbx; out[5] = (int64_t)p.lds;
}
}
