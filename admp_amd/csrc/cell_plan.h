// Host-side plan of the cell-list neighbour search (cell_kernels.hip): how many cells each lattice direction gets and how
// many words the row kernels' partial-count buffer needs.  Plain C++ (no HIP), so that tests/hostshim/cell_plan_shim.cpp can
// compile it for the host and tests/test_neighbour_ref_cpu.py can check it without a GPU.
#pragma once
#include <cstddef>

namespace admp {

constexpr int kBruteMax = 4096;            // up to this many atoms the table builder tests every atom (k_brute_rows): no cells
constexpr int kCellAxisMax = 1024;         // cells along one lattice direction
constexpr long kCellTableMax = 64L * 1024 * 1024;   // cells in all (the table of cell starts stays at 256 MB)

// n_d = floor(height_d / rc) cells along lattice direction d (perpendicular height: the cell width is then >= rc and a
// sphere of radius rc around any point stays within the 27 neighbouring cells), clamped to 1..kCellAxisMax, then halved
// (rounding up) on every axis until the table holds at most kCellTableMax cells.  Halving only widens the cells.
inline void cell_grid_dims(const double* heights, double rc, int n[3]) {
  for (int d = 0; d < 3; ++d) {
    const double q = heights[d] / rc;
    n[d] = q < 1.0 ? 1 : (q > (double)kCellAxisMax ? kCellAxisMax : (int)q);
  }
  while ((long)n[0] * n[1] * n[2] > kCellTableMax)
    for (int d = 0; d < 3; ++d) n[d] = (n[d] + 1) / 2;
}

// Words of the partial row lengths (CellScratch::deg4) for a table of na atoms: k_brute_rows keeps 16 per row (its 16 lanes),
// k_cell_rows 4.  The kernel is chosen by na alone, so the size is a function of na, not of the largest na seen so far.
inline size_t cell_partial_words(int na) { return (size_t)(na <= kBruteMax ? 16 : 4) * ((size_t)na + 1); }

}  // namespace admp
