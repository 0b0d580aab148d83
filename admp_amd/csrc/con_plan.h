// Host-side plan of the constraint kernels (con_kernels.hip k_con_step / k_con_kick / k_con_project): the connected components
// ("clusters") of a list of pairwise distance constraints (i, j, d) packed whole into tiles, one workgroup each, with the
// tile's constraints in local slots.  Plain C++ (no HIP), so that tests/con_shim/main.cpp can compile it for the host and
// tests/test_con_plan_cpu.py can check it without a GPU.  The packing rule is that of mts_plan.h over the constraint list.
//
// Clusters: an atom is connected to every atom it shares a constraint with; an atom in no constraint is a cluster of its own
// and goes through the same kernels.  Packing: clusters in the order of their smallest atom, a cluster's atoms in ascending
// order; a new tile is opened when the next cluster does not fit (next fit: a tile is a contiguous run of clusters).  A
// cluster larger than a tile refuses the plan: one lane sweeps a cluster's constraints over the workgroup's LDS.
//
// Sweep order: a tile's constraints are ordered by cluster, within a cluster they keep the caller's order.  One lane walks
// them in that order, so the result does not depend on the tile capacity, the grid or the launch.  Duplicates are kept.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "mts_plan.h"      // mts_detail::find / join (the root of a component is its smallest atom), mts_threads

namespace admp {

// Capacity: one lane per atom for the elementwise work, as in k_md_mts, hence at most 256.  Default: the fastest of 64 / 128 /
// 256 at 98 304 atoms of rigid water (tools/md_con_bench.py; k_con_step + k_con_kick, us, friction 0 /
// 0.05 per fs): double 109.4 / 122.6, 89.7 / 101.0, 90.0 / 99.3; single 79.2 / 91.9, 62.5 / 73.5, 56.5 / 65.4 -- 256, level
// with 128 in double and ahead in single; at 1 048 575 atoms 256 leads by 20 to 30 %, at 648 atoms the three are level.  As
// in k_md_mts the time follows the number of workgroups: the solve is one lane per cluster whatever the capacity.
constexpr int kConMaxTileAtoms = 256;
constexpr int kConDefaultTileAtoms = 256;
constexpr size_t kConLdsLimit = 64 * 1024;

// largest counts over the tiles: what the kernels' LDS is carved for
struct ConDims {
  int atoms = 0, clusters = 0, cons = 0;
};
// LDS of one workgroup.  Reals: the solved vector (3 per atom: displacement or velocity), 1/m per atom, per constraint d^2
// and the direction s (3); k_con_project also keeps the vector between the positions being moved (3 per constraint:
// with_base).  Ints: 2 slots per constraint and the clusters' constraint ranges.
inline size_t con_lds_reals(const ConDims& d, bool with_base) { return 4 * (size_t)d.atoms + (with_base ? 7 : 4) * (size_t)d.cons; }
inline size_t con_lds_ints(const ConDims& d) { return 2 * (size_t)d.cons + (size_t)d.clusters + 1; }
inline size_t con_lds_bytes(const ConDims& d, size_t real_bytes, bool with_base) {
  return con_lds_reals(d, with_base) * real_bytes + con_lds_ints(d) * sizeof(int);
}

struct ConPlan {
  int n_atoms = 0, tile_atoms = 0, n_tiles = 0, n_clusters = 0, max_cluster = 0, n_cons = 0;
  ConDims dims;
  std::vector<int> tile_atom0;      // (n_tiles + 1) first global slot of a tile; global slot = tile_atom0[t] + local slot
  std::vector<int> atom_id;         // (n_atoms) global slot -> atom
  std::vector<int> tile_clu0;       // (n_tiles + 1) first cluster of a tile
  std::vector<int> clu_atom0;       // (n_clusters + 1) first global slot of a cluster
  std::vector<int> clu_con0;        // (n_clusters + 1) first constraint of a cluster in the plan's order; a tile's constraints
                                    // are clu_con0[tile_clu0[t]] .. clu_con0[tile_clu0[t + 1]]
  std::vector<int> con_slot;        // (n_cons, 2) local slots (i, j)
  std::vector<int> con_order;       // (n_cons) the caller's index of the plan's constraint
  std::vector<double> con_d2;       // (n_cons) d^2
  std::string error;                // empty: the plan is valid
};

// pairs (n_cons, 2), lengths (n_cons).  On refusal plan.error says why and the arrays are unspecified.
inline ConPlan con_make_plan(int n_atoms, int n_cons, const int32_t* pairs, const double* lengths, int tile_atoms) {
  using mts_detail::find;
  ConPlan p;
  p.n_atoms = n_atoms; p.tile_atoms = tile_atoms; p.n_cons = n_cons;
  if (n_atoms < 1 || n_cons < 0) { p.error = "n_atoms must be positive and the number of constraints not negative"; return p; }
  if (tile_atoms < 1 || tile_atoms > kConMaxTileAtoms) {
    p.error = "tile_atoms " + std::to_string(tile_atoms) + " outside 1.." + std::to_string(kConMaxTileAtoms);
    return p;
  }
  if (n_cons > INT32_MAX / 8) { p.error = "too many constraints"; return p; }
  for (int k = 0; k < n_cons; ++k) {
    const int i = pairs[2 * (size_t)k], j = pairs[2 * (size_t)k + 1];
    const std::string who = "constraint " + std::to_string(k) + " (" + std::to_string(i) + ", " + std::to_string(j) + ")";
    if (i < 0 || i >= n_atoms || j < 0 || j >= n_atoms) { p.error = who + ": atom index out of range"; return p; }
    if (i == j) { p.error = who + ": an atom cannot be constrained to itself"; return p; }
    if (!(lengths[k] > 0.0) || !std::isfinite(lengths[k])) { p.error = who + ": the length must be positive and finite"; return p; }
  }
  std::vector<int> parent(n_atoms);
  for (int i = 0; i < n_atoms; ++i) parent[i] = i;
  for (int k = 0; k < n_cons; ++k) mts_detail::join(parent, pairs[2 * (size_t)k], pairs[2 * (size_t)k + 1]);
  std::vector<int> size(n_atoms, 0);
  for (int i = 0; i < n_atoms; ++i) size[find(parent, i)] += 1;
  for (int i = 0; i < n_atoms; ++i) {
    if (size[i] > p.max_cluster) p.max_cluster = size[i];
    if (size[i] > tile_atoms) {      // (ascending i: the first one found has the smallest atom)
      p.error = "a cluster of " + std::to_string(size[i]) + " atoms (smallest atom " + std::to_string(i) + ") exceeds tile_atoms " +
                std::to_string(tile_atoms) + ": a cluster's constraints are solved in one workgroup";
      return p;
    }
  }
  // clusters in root order; tiles by next fit
  std::vector<int> clu_of(n_atoms, -1);      // root -> cluster, then atom -> cluster
  int used = 0;
  for (int i = 0; i < n_atoms; ++i) {
    if (parent[i] != i) continue;
    if (p.n_tiles == 0 || used + size[i] > tile_atoms) { p.n_tiles += 1; used = 0; p.tile_clu0.push_back(p.n_clusters); }
    clu_of[i] = p.n_clusters++;
    used += size[i];
  }
  p.tile_clu0.push_back(p.n_clusters);
  p.clu_atom0.assign(p.n_clusters + 1, 0);
  for (int i = 0; i < n_atoms; ++i)
    if (parent[i] == i) p.clu_atom0[clu_of[i] + 1] = size[i];
  for (int c = 0; c < p.n_clusters; ++c) p.clu_atom0[c + 1] += p.clu_atom0[c];
  p.tile_atom0.assign(p.n_tiles + 1, 0);
  for (int t = 0; t <= p.n_tiles; ++t) p.tile_atom0[t] = p.clu_atom0[p.tile_clu0[t]];
  std::vector<int> tile_of_clu(p.n_clusters);
  for (int t = 0; t < p.n_tiles; ++t)
    for (int c = p.tile_clu0[t]; c < p.tile_clu0[t + 1]; ++c) tile_of_clu[c] = t;
  std::vector<int> next(p.clu_atom0.begin(), p.clu_atom0.end() - 1), slot(n_atoms);      // atom -> global slot
  p.atom_id.assign(n_atoms, 0);
  for (int i = 0; i < n_atoms; ++i) {
    const int c = clu_of[find(parent, i)];
    clu_of[i] = c;
    slot[i] = next[c]++;
    p.atom_id[slot[i]] = i;
  }
  // constraints by cluster, stable
  p.clu_con0.assign(p.n_clusters + 1, 0);
  for (int k = 0; k < n_cons; ++k) p.clu_con0[clu_of[pairs[2 * (size_t)k]] + 1] += 1;
  for (int c = 0; c < p.n_clusters; ++c) p.clu_con0[c + 1] += p.clu_con0[c];
  std::vector<int> at(p.clu_con0.begin(), p.clu_con0.end() - 1);
  p.con_slot.assign(2 * (size_t)n_cons, 0);
  p.con_order.assign(n_cons, 0);
  p.con_d2.assign(n_cons, 0.0);
  for (int k = 0; k < n_cons; ++k) {
    const int c = clu_of[pairs[2 * (size_t)k]], q = at[c]++, a0 = p.tile_atom0[tile_of_clu[c]];
    p.con_slot[2 * (size_t)q] = slot[pairs[2 * (size_t)k]] - a0;
    p.con_slot[2 * (size_t)q + 1] = slot[pairs[2 * (size_t)k + 1]] - a0;
    p.con_order[q] = k;
    p.con_d2[q] = lengths[k] * lengths[k];
  }
  for (int t = 0; t < p.n_tiles; ++t) {
    ConDims& d = p.dims;
    const int n = p.tile_atom0[t + 1] - p.tile_atom0[t], nc = p.tile_clu0[t + 1] - p.tile_clu0[t];
    const int nq = p.clu_con0[p.tile_clu0[t + 1]] - p.clu_con0[p.tile_clu0[t]];
    d.atoms = n > d.atoms ? n : d.atoms;
    d.clusters = nc > d.clusters ? nc : d.clusters;
    d.cons = nq > d.cons ? nq : d.cons;
  }
  if (con_lds_bytes(p.dims, sizeof(double), true) > kConLdsLimit)
    p.error = "a tile's constraints need " + std::to_string(con_lds_bytes(p.dims, sizeof(double), true)) + " bytes of LDS (limit " +
              std::to_string(kConLdsLimit) + "): lower tile_atoms";
  return p;
}

}  // namespace admp
