// Block-id layout of an x pass that carries the closing pair kernel (pair_kernels.hip k_xconv_pair_full).  Plain integer
// arithmetic with no device-only construct, in a header of its own (included by dft_lines.h) so that the host-compiled test
// shim can drive it (tests/test_pair_rider_layout_cpu.py).
//
// Workgroups start in the order of their linear id  lin = blockIdx.y * gridDim.x + blockIdx.x.  The launch lasts as long as
// its longest workgroups, the pair ones (one wave of 256 registers per SIMD slot, ~15 us), so those take the lowest ids and
// all start at once; the workgroups of the second rider (k_pair_field_ind, a few us) follow, then the x-pass tiles, which
// fill the slots that are left and those the first tiles free:
//     [0, npair)                      closing pair kernel, rank = lin
//     [npair, npair + nind)           field increment, rank = lin - npair
//     [.., .. + nbx * ny)             tile t = lin - npair - nind  ->  (bx, by) = (t % nbx, t / nbx)
//     the rest of the grid            idle
// npair and nind are multiples of 8 (xcd_grid): workgroups are dealt to the 8 XCDs by lin % 8, so a rider rank sits on the
// XCD that xcd_block assumes for it, and tile t on the XCD it has in a launch of its own (grid (nbx, ny), same t).
#pragma once

#if defined(__HIPCC__)
#define ADMP_LAYOUT_HD __host__ __device__ __forceinline__
#else
#define ADMP_LAYOUT_HD inline
#endif

namespace admp {

enum { RIDER_PAIR = 0, RIDER_IND = 1, RIDER_TILE = 2, RIDER_IDLE = 3 };
struct RiderGrid {
  unsigned npair = 0, nind = 0;   // workgroups of the two riders (each a multiple of 8)
  unsigned nbx = 0, ny = 0;       // x-pass tiles per y row, y rows
};
struct RiderBlock {
  int kind;
  unsigned rank;                  // RIDER_PAIR / RIDER_IND: the workgroup's index in a launch of its own
  unsigned bx, by;                // RIDER_TILE: tile and y row
};
ADMP_LAYOUT_HD unsigned rider_grid_blocks(const RiderGrid& g) { return g.npair + g.nind + g.nbx * g.ny; }
ADMP_LAYOUT_HD RiderBlock rider_block(const RiderGrid& g, unsigned bx, unsigned by, unsigned gdx) {
  unsigned lin = by * gdx + bx;
  if (lin < g.npair) return RiderBlock{RIDER_PAIR, lin, 0u, 0u};
  lin -= g.npair;
  if (lin < g.nind) return RiderBlock{RIDER_IND, lin, 0u, 0u};
  lin -= g.nind;
  if (lin < g.nbx * g.ny) return RiderBlock{RIDER_TILE, 0u, lin % g.nbx, lin / g.nbx};
  return RiderBlock{RIDER_IDLE, 0u, 0u, 0u};
}

}  // namespace admp
