// Host-side plan of the molecular-scaling kernels (mol_kernels.hip k_md_mol_sums / k_md_mol_scale): a partition of the atoms
// into groups ("molecules": every atom in exactly one, a singleton is a group) packed whole into tiles, one workgroup each.
// Plain C++ (no HIP), so that tests/mol_shim/main.cpp can compile it for the host and tests/test_mol_plan_cpu.py can check it
// without a GPU.  The packing rule is that of mts_plan.h / con_plan.h over the caller's labels.
//
// Groups: group_of[i] is any int32 label >= 0; the labels need not be dense or ordered.  Packing: groups in the order of their
// smallest atom, a group's atoms in ascending order -- its first slot is its anchor, the lowest-numbered atom --; a new tile
// is opened when the next group does not fit (next fit: a tile is a contiguous run of groups).  A group larger than a tile
// refuses the plan: one lane sums a group over the workgroup's LDS.
//
// Determinism: a group's sums are formed by one lane in slot order, so they do not depend on the tile capacity, the grid or
// the launch.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

#include "mts_plan.h"      // mts_threads

namespace admp {

// Capacity: one lane per atom, as in k_md_mts and the constraint kernels, hence at most 256.  Default: the fastest of 64 / 128 /
// 256 (tools/md_mol_bench.py; k_md_mol_sums in double, us): 52.4 / 51.5 / 46.1 at 98 304 atoms of water,
// 164.9 / 103.6 / 82.4 at 1 048 575; k_md_mol_scale is level over the three (5.5 and 24 us).  As in those kernels the time
// follows the number of workgroups.
constexpr int kMolMaxTileAtoms = 256;
constexpr int kMolDefaultTileAtoms = 256;

// largest counts over the tiles: what the kernels' LDS is carved for
struct MolDims {
  int atoms = 0, groups = 0;
};
// LDS of one workgroup.  Doubles first: per group M, sum m d / M (3), sum m v / M (3).  Reals: per atom d (3), v (3), 1/m.
constexpr int kMolGroupWords = 7;
inline size_t mol_lds_bytes(const MolDims& d, size_t real_bytes) {
  return kMolGroupWords * (size_t)d.groups * sizeof(double) + 7 * (size_t)d.atoms * real_bytes;
}

struct MolPlan {
  int n_atoms = 0, tile_atoms = 0, n_tiles = 0, n_groups = 0, max_group = 0;
  MolDims dims;
  std::vector<int> tile_atom0;      // (n_tiles + 1) first global slot of a tile; global slot = tile_atom0[t] + local slot
  std::vector<int> atom_id;         // (n_atoms) global slot -> atom
  std::vector<int> tile_grp0;       // (n_tiles + 1) first group of a tile
  std::vector<int> grp_atom0;       // (n_groups + 1) first global slot of a group: its anchor
  std::vector<int> slot_grp;        // (n_atoms) global slot -> its group's index within the tile
  std::string error;                // empty: the plan is valid
};

// group_of (n_atoms).  On refusal plan.error says why and the arrays are unspecified.
inline MolPlan mol_make_plan(int n_atoms, const int32_t* group_of, int tile_atoms) {
  MolPlan p;
  p.n_atoms = n_atoms; p.tile_atoms = tile_atoms;
  if (n_atoms < 1) { p.error = "n_atoms must be positive"; return p; }
  if (tile_atoms < 1 || tile_atoms > kMolMaxTileAtoms) {
    p.error = "tile_atoms " + std::to_string(tile_atoms) + " outside 1.." + std::to_string(kMolMaxTileAtoms);
    return p;
  }
  // groups in the order of their first (= smallest) atom
  std::unordered_map<int32_t, int> index;
  std::vector<int> grp(n_atoms), size, first;
  for (int i = 0; i < n_atoms; ++i) {
    const int32_t label = group_of[i];
    if (label < 0) { p.error = "atom " + std::to_string(i) + " has the negative group label " + std::to_string(label); return p; }
    const auto it = index.find(label);
    if (it == index.end()) {
      index.emplace(label, p.n_groups);
      grp[i] = p.n_groups++;
      size.push_back(1);
      first.push_back(i);
    } else {
      grp[i] = it->second;
      size[it->second] += 1;
    }
  }
  for (int g = 0; g < p.n_groups; ++g) {
    if (size[g] > p.max_group) p.max_group = size[g];
    if (size[g] > tile_atoms) {      // (ascending g: the first one found has the smallest atom)
      p.error = "a group of " + std::to_string(size[g]) + " atoms (smallest atom " + std::to_string(first[g]) + ") exceeds tile_atoms " +
                std::to_string(tile_atoms) + ": a group's sums are formed in one workgroup";
      return p;
    }
  }
  // tiles by next fit
  std::vector<int> tile_of_grp(p.n_groups);
  int used = 0;
  for (int g = 0; g < p.n_groups; ++g) {
    if (p.n_tiles == 0 || used + size[g] > tile_atoms) { p.n_tiles += 1; used = 0; p.tile_grp0.push_back(g); }
    tile_of_grp[g] = p.n_tiles - 1;
    used += size[g];
  }
  p.tile_grp0.push_back(p.n_groups);
  p.grp_atom0.assign(p.n_groups + 1, 0);
  for (int g = 0; g < p.n_groups; ++g) p.grp_atom0[g + 1] = p.grp_atom0[g] + size[g];
  p.tile_atom0.assign(p.n_tiles + 1, 0);
  for (int t = 0; t <= p.n_tiles; ++t) p.tile_atom0[t] = p.grp_atom0[p.tile_grp0[t]];
  std::vector<int> next(p.grp_atom0.begin(), p.grp_atom0.end() - 1);
  p.atom_id.assign(n_atoms, 0);
  p.slot_grp.assign(n_atoms, 0);
  for (int i = 0; i < n_atoms; ++i) {      // ascending i: a group's slots ascend with its atoms
    const int g = grp[i], slot = next[g]++;
    p.atom_id[slot] = i;
    p.slot_grp[slot] = g - p.tile_grp0[tile_of_grp[g]];
  }
  for (int t = 0; t < p.n_tiles; ++t) {
    const int n = p.tile_atom0[t + 1] - p.tile_atom0[t], ng = p.tile_grp0[t + 1] - p.tile_grp0[t];
    p.dims.atoms = n > p.dims.atoms ? n : p.dims.atoms;
    p.dims.groups = ng > p.dims.groups ? ng : p.dims.groups;
  }
  return p;
}

}  // namespace admp
