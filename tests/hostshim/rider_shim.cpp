// Host build of the block-id layout of the x pass that carries the closing pair kernel (admp_amd/csrc/rider_layout.h;
// tests/test_pair_rider_layout_cpu.py).
#include <cstdint>

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
}
