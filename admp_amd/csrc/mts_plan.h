// Host-side plan of the multiple-time-step kernel (mts_kernels.hip k_md_mts): the connected components of the bond / angle
// lists packed whole into tiles, one workgroup each, with the tile's items in local slots and, per atom, the list of item
// contributions its force is summed from.  Plain C++ (no HIP), so that tests/mts_shim/main.cpp can compile it for the host and
// tests/test_mts_plan_cpu.py can check it without a GPU.
//
// Components: an atom is connected to every atom it shares a bond or an angle with (an angle connects its three atoms even
// where no bond does); an atom in no item is a component of its own and is integrated like any other.  Packing: components in
// the order of their smallest atom index, a component's atoms in ascending order; a new tile is opened when the next
// component does not fit (next fit: earlier tiles are not revisited, so a tile is a contiguous run of components).  A
// component larger than a tile refuses the plan: the inner loop of a molecule needs all its atoms in one workgroup's LDS.
//
// Determinism: the items of a tile keep the order of the caller's lists, and an atom's references are its bonds in that order,
// then its angles in that order.  The kernel sums an atom's force over its references in sequence, so r and v do not depend
// on the tile capacity, the grid or the launch.  Duplicate items are kept (each counts, as in k_md_bonded).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace admp {

// Capacity.  The kernel gives every atom of a tile one lane for the whole inner loop (v, f, 1/m and the noise amplitude stay
// in its registers); only what other lanes read goes to LDS.  The largest workgroup used is 256 lanes, hence the maximum.  In
// double precision a tile keeps, in bytes: r 24 per atom; per bond one force slot (24), its parameters (16) and slots (8);
// per angle two force slots (48), parameters (16), slots (12); per atom a reference offset (4) and per reference 4.  A water
// (3 atoms, 2 bonds, 1 angle, 7 references) takes 72 + 96 + 76 + 12 + 28 = 284 B, i.e. 95 B per atom: 24 KiB for 255 atoms,
// far below the 64 KiB a workgroup may claim without asking (kMtsLdsLimit: item-heavy inputs are refused by bytes).
// Default.  The 98 304-atom box (32 768 waters) on 256 CUs: capacity 256 holds 85 waters and yields 386 four-wave workgroups,
// 1.5 per CU, 24 KiB of LDS each; 128 gives 781 two-wave workgroups, 64 gives 1 561 single-wave ones (21 waters = 63 lanes,
// no workgroup barrier, 6.1 per CU), 32 gives 3 277 that use 30 of 64 lanes.  More and smaller workgroups looked right for a
// latency-bound loop; measured, the time follows the number of workgroups instead (94 / 53 / 35 / 26 us
// at capacities 32 / 64 / 128 / 256 for this box in double, the same order at 648 and 1 048 575 atoms).  A wavefront walks the
// atom pass, the bond pass and the angle pass whatever share of its lanes has an item, and the angle pass (acos in double, a
// dozen divisions) is the long one: at 64 every wavefront runs it for 21 lanes, at 256 two of four wavefronts run it for 64
// and 21.  Hence the largest capacity is the default.
constexpr int kMtsMaxTileAtoms = 256;
constexpr int kMtsDefaultTileAtoms = 256;
constexpr size_t kMtsLdsLimit = 64 * 1024;

// largest counts over the tiles: what the kernel's LDS is carved for
struct MtsDims {
  int atoms = 0, bonds = 0, angles = 0, refs = 0;
};
// LDS of one workgroup: reals first (r, force slots, bond and angle parameters), then the ints (bond and angle slots, the
// atoms' reference offsets, the references)
inline size_t mts_lds_reals(const MtsDims& d) { return 3 * (size_t)d.atoms + 3 * ((size_t)d.bonds + 2 * (size_t)d.angles) + 2 * (size_t)d.bonds + 2 * (size_t)d.angles; }
inline size_t mts_lds_ints(const MtsDims& d) { return 2 * (size_t)d.bonds + 3 * (size_t)d.angles + (size_t)d.atoms + 1 + (size_t)d.refs; }
inline size_t mts_lds_bytes(const MtsDims& d, size_t real_bytes) { return mts_lds_reals(d) * real_bytes + mts_lds_ints(d) * sizeof(int); }
// lanes of the workgroup for a capacity: one per atom, whole wavefronts
inline int mts_threads(int tile_atoms) { return tile_atoms <= 64 ? 64 : (tile_atoms <= 128 ? 128 : 256); }

struct MtsPlan {
  int n_atoms = 0, tile_atoms = 0, n_tiles = 0, max_component = 0, n_bonds = 0, n_angles = 0;
  MtsDims dims;
  std::vector<int> tile_atom0;      // (n_tiles + 1) first global slot of a tile; global slot = tile_atom0[t] + local slot
  std::vector<int> atom_id;         // (n_atoms) global slot -> atom
  std::vector<int> tile_bond0;      // (n_tiles + 1)
  std::vector<int> bond_slot;       // (n_bonds, 2) local slots (i, j), the caller's order within a tile
  std::vector<double> bond_par;     // (n_bonds, 2) = (k, r0)
  std::vector<int> tile_angle0;     // (n_tiles + 1)
  std::vector<int> angle_slot;      // (n_angles, 3) local slots (i, centre, k)
  std::vector<double> angle_par;    // (n_angles, 2) = (k, theta0)
  std::vector<int> ref0;            // (n_atoms + 1) by global slot: first reference of the atom
  std::vector<int> ref;             // (2 n_bonds + 3 n_angles) 4 * force slot + kind (md_bonded_math.h); force slot of the tile's
                                    // bond b: b, of its angle a: bonds of the tile + 2 a (gu) and + 1 (gv)
  std::string error;                // empty: the plan is valid
};

namespace mts_detail {
inline int find(std::vector<int>& p, int i) {
  while (p[i] != i) { p[i] = p[p[i]]; i = p[i]; }
  return i;
}
// the root of a component is its smallest atom
inline void join(std::vector<int>& p, int a, int b) {
  a = find(p, a); b = find(p, b);
  if (a < b) p[b] = a; else p[a] = b;
}
}  // namespace mts_detail

// bonds (n_bonds, 2), bond_par (n_bonds, 2), angles (n_angles, 3), angle_par (n_angles, 2).  On refusal plan.error says why
// and the arrays are unspecified.
inline MtsPlan mts_make_plan(int n_atoms, int n_bonds, const int32_t* bonds, const double* bond_par, int n_angles,
                             const int32_t* angles, const double* angle_par, int tile_atoms) {
  using mts_detail::find;
  MtsPlan p;
  p.n_atoms = n_atoms; p.tile_atoms = tile_atoms; p.n_bonds = n_bonds; p.n_angles = n_angles;
  if (n_atoms < 1 || n_bonds < 0 || n_angles < 0) { p.error = "n_atoms must be positive and the item counts not negative"; return p; }
  if (tile_atoms < 1 || tile_atoms > kMtsMaxTileAtoms) {
    p.error = "tile_atoms " + std::to_string(tile_atoms) + " outside 1.." + std::to_string(kMtsMaxTileAtoms);
    return p;
  }
  if ((int64_t)2 * n_bonds + (int64_t)3 * n_angles > INT32_MAX / 4) { p.error = "too many items"; return p; }
  for (int64_t k = 0; k < (int64_t)2 * n_bonds; ++k)
    if (bonds[k] < 0 || bonds[k] >= n_atoms) { p.error = "bond atom index out of range"; return p; }
  for (int64_t k = 0; k < (int64_t)3 * n_angles; ++k)
    if (angles[k] < 0 || angles[k] >= n_atoms) { p.error = "angle atom index out of range"; return p; }

  std::vector<int> parent(n_atoms);
  for (int i = 0; i < n_atoms; ++i) parent[i] = i;
  for (int b = 0; b < n_bonds; ++b) mts_detail::join(parent, bonds[2 * b], bonds[2 * b + 1]);
  for (int a = 0; a < n_angles; ++a) {
    mts_detail::join(parent, angles[3 * a], angles[3 * a + 1]);
    mts_detail::join(parent, angles[3 * a + 1], angles[3 * a + 2]);
  }
  std::vector<int> size(n_atoms, 0);
  for (int i = 0; i < n_atoms; ++i) size[find(parent, i)] += 1;
  for (int i = 0; i < n_atoms; ++i) {
    if (size[i] > p.max_component) p.max_component = size[i];
    if (size[i] > tile_atoms) {      // (ascending i: the first one found has the smallest atom)
      p.error = "a component of " + std::to_string(size[i]) + " atoms (smallest atom " + std::to_string(i) + ") exceeds tile_atoms " +
                std::to_string(tile_atoms) + ": a molecule's inner loop needs all its atoms in one workgroup";
      return p;
    }
  }
  // tiles: roots in ascending order; tile_of_root, then the atoms of each tile in (component, atom) order
  std::vector<int> tile_of(n_atoms, -1), fill;
  int used = 0;
  for (int i = 0; i < n_atoms; ++i) {
    if (parent[i] != i) continue;
    if (p.n_tiles == 0 || used + size[i] > tile_atoms) { p.n_tiles += 1; used = 0; fill.push_back(0); }
    tile_of[i] = p.n_tiles - 1;
    used += size[i];
    fill.back() = used;
  }
  p.tile_atom0.assign(p.n_tiles + 1, 0);
  for (int t = 0; t < p.n_tiles; ++t) p.tile_atom0[t + 1] = p.tile_atom0[t] + fill[t];
  // a component's first global slot, in root order within its tile; its atoms follow in ascending order
  std::vector<int> next(n_atoms, 0), cursor(p.tile_atom0.begin(), p.tile_atom0.end() - 1);
  for (int i = 0; i < n_atoms; ++i)
    if (parent[i] == i) { next[i] = cursor[tile_of[i]]; cursor[tile_of[i]] += size[i]; }
  std::vector<int> slot(n_atoms);      // atom -> global slot
  p.atom_id.assign(n_atoms, 0);
  for (int i = 0; i < n_atoms; ++i) {
    const int r = find(parent, i);
    tile_of[i] = tile_of[r];
    slot[i] = next[r]++;
    p.atom_id[slot[i]] = i;
  }
  // items by tile, stable
  auto by_tile = [&](int n, int w, const int32_t* idx, const double* par, std::vector<int>& first, std::vector<int>& out,
                     std::vector<double>& out_par) {
    first.assign(p.n_tiles + 1, 0);
    for (int k = 0; k < n; ++k) first[tile_of[idx[(size_t)w * k]] + 1] += 1;
    for (int t = 0; t < p.n_tiles; ++t) first[t + 1] += first[t];
    std::vector<int> at(first.begin(), first.end() - 1);
    out.assign((size_t)w * n, 0);
    out_par.assign((size_t)2 * n, 0.0);
    for (int k = 0; k < n; ++k) {
      const int t = tile_of[idx[(size_t)w * k]], q = at[t]++;
      for (int c = 0; c < w; ++c) out[(size_t)w * q + c] = slot[idx[(size_t)w * k + c]] - p.tile_atom0[t];
      out_par[2 * (size_t)q] = par[2 * (size_t)k];
      out_par[2 * (size_t)q + 1] = par[2 * (size_t)k + 1];
    }
  };
  by_tile(n_bonds, 2, bonds, bond_par, p.tile_bond0, p.bond_slot, p.bond_par);
  by_tile(n_angles, 3, angles, angle_par, p.tile_angle0, p.angle_slot, p.angle_par);
  // references: count, then fill -- bonds before angles, each in the tile's (= the caller's) order
  p.ref0.assign(n_atoms + 1, 0);
  for (int t = 0; t < p.n_tiles; ++t) {
    const int a0 = p.tile_atom0[t];
    for (int b = p.tile_bond0[t]; b < p.tile_bond0[t + 1]; ++b)
      for (int c = 0; c < 2; ++c) p.ref0[a0 + p.bond_slot[2 * (size_t)b + c] + 1] += 1;
    for (int a = p.tile_angle0[t]; a < p.tile_angle0[t + 1]; ++a)
      for (int c = 0; c < 3; ++c) p.ref0[a0 + p.angle_slot[3 * (size_t)a + c] + 1] += 1;
  }
  for (int g = 0; g < n_atoms; ++g) p.ref0[g + 1] += p.ref0[g];
  p.ref.assign(p.ref0[n_atoms], 0);
  std::vector<int> at(p.ref0.begin(), p.ref0.end() - 1);
  for (int t = 0; t < p.n_tiles; ++t) {
    const int a0 = p.tile_atom0[t], nb = p.tile_bond0[t + 1] - p.tile_bond0[t];
    for (int b = p.tile_bond0[t]; b < p.tile_bond0[t + 1]; ++b) {
      const int s = b - p.tile_bond0[t];
      p.ref[at[a0 + p.bond_slot[2 * (size_t)b]]++] = 4 * s + 1;          // kMtsRefMinus: dE/dr_i = -g
      p.ref[at[a0 + p.bond_slot[2 * (size_t)b + 1]]++] = 4 * s + 0;      // kMtsRefPlus
    }
    for (int a = p.tile_angle0[t]; a < p.tile_angle0[t + 1]; ++a) {
      const int s = nb + 2 * (a - p.tile_angle0[t]);
      p.ref[at[a0 + p.angle_slot[3 * (size_t)a]]++] = 4 * s + 0;          // gu
      p.ref[at[a0 + p.angle_slot[3 * (size_t)a + 1]]++] = 4 * s + 2;      // kMtsRefCentre: -(gu + gv)
      p.ref[at[a0 + p.angle_slot[3 * (size_t)a + 2]]++] = 4 * (s + 1) + 0;      // gv
    }
    MtsDims& d = p.dims;
    const int na = p.tile_angle0[t + 1] - p.tile_angle0[t], n = p.tile_atom0[t + 1] - a0, nr = p.ref0[p.tile_atom0[t + 1]] - p.ref0[a0];
    d.atoms = n > d.atoms ? n : d.atoms;
    d.bonds = nb > d.bonds ? nb : d.bonds;
    d.angles = na > d.angles ? na : d.angles;
    d.refs = nr > d.refs ? nr : d.refs;
  }
  if (mts_lds_bytes(p.dims, sizeof(double)) > kMtsLdsLimit)
    p.error = "a tile's items need " + std::to_string(mts_lds_bytes(p.dims, sizeof(double))) + " bytes of LDS (limit " +
              std::to_string(kMtsLdsLimit) + "): lower tile_atoms";
  return p;
}

}  // namespace admp
