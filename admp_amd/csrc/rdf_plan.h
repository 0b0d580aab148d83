// Host-side plan of an admp_md_rdf call (rdf_kernels.hip): which form runs, how many workgroups, the cell grid for r_max and the
// LDS words of a workgroup.  Plain C++ (no HIP), so that tests/rdf_shim compiles it for the host and tests/test_rdf_cpu.py can
// check it without a GPU.
//
//   tiles  up to kBruteMax atoms (cell_plan.h: below that the launches of the binning cost more than they save), and whenever
//          force = 1: one workgroup per pair (I <= J) of tiles of kRdfTile atoms, numbered by the triangular index of rdf_math.h.
//   cells  above kBruteMax atoms, and whenever force = 2: cell_grid_dims at cell width >= r_max, one workgroup per home cell,
//          the half sweep of rdf_math.h.
//
// LDS of a workgroup: channels x n_bins 32-bit counters (at most kRdfMaxCounters, 64 KB: with the staged positions a workgroup
// stays below 80 KB and two share a CU's 160 KB), then the staged atoms: three reals and a tag each, two tiles in the tile form,
// one chunk of kRdfChunk atoms of a neighbour cell in the cell form.
#pragma once
#include <cstddef>
#include <cstdint>

#include "cell_plan.h"
#include "rdf_math.h"

namespace admp {

constexpr int kRdfTile = 256;        // atoms of a tile = lanes of a workgroup
constexpr int kRdfChunk = 256;       // atoms of a neighbour cell staged at a time
constexpr int kRdfMaxTiles = 32768;  // the triangular index of a tile pair stays below 2^31
enum { RDF_FORM_NONE = 0, RDF_FORM_TILES = 1, RDF_FORM_CELLS = 2 };

struct RdfPlan {
  const char* error = nullptr;      // set: the call is refused with this text
  int form = RDF_FORM_NONE;         // RDF_FORM_NONE: nothing to launch (no atoms)
  int channels = 0, counters = 0;
  int n_tiles = 0;
  int grid[3] = {0, 0, 0};
  long n_cells = 0;
  long workgroups = 0;
  size_t lds_bytes = 0;
};

inline size_t rdf_lds_bytes(int form, int counters, size_t real_bytes) {
  const size_t staged = (size_t)(form == RDF_FORM_TILES ? 2 * kRdfTile : kRdfChunk);
  // (counters and tags are 4 bytes: the reals come first so that doubles stay 8-byte aligned)
  return staged * 3 * real_bytes + staged * sizeof(int32_t) + (size_t)counters * sizeof(uint32_t);
}

// heights: the three perpendicular heights of the cell.  The caller has checked the box; everything else is checked here.
inline RdfPlan rdf_make_plan(int n_atoms, const double* heights, double r_max, int n_types, int n_bins, size_t real_bytes, int force) {
  RdfPlan p;
  if (n_atoms < 0) { p.error = "n_atoms must not be negative"; return p; }
  if (n_types < 1 || n_types > kRdfMaxTypes) { p.error = "n_types must lie in 1..8"; return p; }
  if (n_bins < 1) { p.error = "n_bins must be at least 1"; return p; }
  p.channels = rdf_channels(n_types);
  if ((long)p.channels * n_bins > kRdfMaxCounters) { p.error = "channels * n_bins exceeds 16384 counters"; return p; }
  p.counters = p.channels * n_bins;
  if (!(r_max > 0.0)) { p.error = "r_max must be positive"; return p; }
  for (int d = 0; d < 3; ++d)
    if (!(r_max <= 0.5 * heights[d])) { p.error = "r_max exceeds half a cell height (minimum image)"; return p; }
  if (force < 0 || force > 2) { p.error = "force must be 0 (auto), 1 (tiles) or 2 (cells)"; return p; }
  if (n_atoms == 0) return p;
  p.form = force != 0 ? force : (n_atoms <= kBruteMax ? RDF_FORM_TILES : RDF_FORM_CELLS);
  if (p.form == RDF_FORM_TILES) {
    p.n_tiles = (n_atoms + kRdfTile - 1) / kRdfTile;
    if (p.n_tiles > kRdfMaxTiles) { p.error = "too many atoms for the tile form"; return p; }
    p.workgroups = (long)p.n_tiles * (p.n_tiles + 1) / 2;
  } else {
    cell_grid_dims(heights, r_max, p.grid);
    p.n_cells = (long)p.grid[0] * p.grid[1] * p.grid[2];
    p.workgroups = p.n_cells;
  }
  p.lds_bytes = rdf_lds_bytes(p.form, p.counters, real_bytes);
  return p;
}

}  // namespace admp
