// Arithmetic of the radial distribution functions (rdf_kernels.hip; include/admp_hip.h admp_md_rdf), host and device: the kernels
// and the host program of tests/rdf_shim compile this text.
//
//   tag      one int32 per atom, type | group << 4.  type 0 .. n_types - 1 (n_types <= 8) is a counted type; 15 means "not
//            counted", and so does every other value (8 .. 14, and a type >= n_types, which would have no channel); group is
//            0 .. 2^27 - 1.  A pair is counted when both types are counted and the groups differ: "no exclusions" is every
//            atom its own group.
//   channel  the index of the unordered type pair, with a <= b: a n_types - a (a - 1) / 2 + (b - a); n_types (n_types + 1) / 2
//            of them.  The same triangular index numbers the pairs of tiles (I <= J) of the tile form.
//   bin      -1 unless r2 < rmax2 (which also drops NaN), else min((int)(sqrt(r2) inv_dr), n_bins - 1): r just under r_max may
//            round to n_bins, and the index goes straight into LDS.
//   r2       |min_image(r_i - r_j)|^2 in the handle's precision: the arithmetic of the pair and cell kernels (pme_math.h).
//   sweep    the half sweep of the cell form: which of the cells around a home cell a workgroup takes, so that every unordered
//            pair of neighbouring cells is met exactly once (rdf_sweep_take).
#pragma once
#include "pme_math.h"

namespace admp {

constexpr int kRdfMaxTypes = 8;
constexpr int kRdfNotCounted = 15;
constexpr int kRdfMaxCounters = 16384;      // channels x n_bins: 64 KB of 32-bit LDS counters

// index of the unordered pair (a, b), a <= b < n, in the row-major upper triangle
ADMP_HD int rdf_tri_index(int a, int b, int n) { return a * n - a * (a - 1) / 2 + (b - a); }
// ... and back: w in 0 .. n (n + 1) / 2 - 1
ADMP_HD void rdf_tri_pair(int w, int n, int* a, int* b) {
  int i = 0;
  while (w >= n - i) { w -= n - i; ++i; }
  *a = i; *b = i + w;
}

ADMP_HD int rdf_channels(int n_types) { return n_types * (n_types + 1) / 2; }
ADMP_HD int rdf_channel(int ta, int tb, int n_types) { return ta <= tb ? rdf_tri_index(ta, tb, n_types) : rdf_tri_index(tb, ta, n_types); }
ADMP_HD int rdf_tag_type(int tag) { return tag & 15; }
ADMP_HD int rdf_tag_group(int tag) { return (int)((unsigned)tag >> 4); }

// the channel of a pair of tags, or -1 when the pair is not counted
ADMP_HD int rdf_pair_channel(int tag_a, int tag_b, int n_types) {
  const int ta = rdf_tag_type(tag_a), tb = rdf_tag_type(tag_b);
  if (ta >= n_types || tb >= n_types || rdf_tag_group(tag_a) == rdf_tag_group(tag_b)) return -1;
  return rdf_channel(ta, tb, n_types);
}

template <class T>
ADMP_HD int rdf_bin(T r2, T rmax2, T inv_dr, int n_bins) {
  if (!(r2 < rmax2)) return -1;
  const int k = (int)(m_sqrt(r2) * inv_dr);
  return k < n_bins - 1 ? k : n_bins - 1;
}

// the bin of the pair (i, j), or -1
template <class T>
ADMP_HD int rdf_pair_bin(const Box<T>& box, const T ri[3], const T rj[3], T rmax2, T inv_dr, int n_bins) {
  T d[3] = {ri[0] - rj[0], ri[1] - rj[1], ri[2] - rj[2]};
  min_image(box, d);
  return rdf_bin(d[0] * d[0] + d[1] * d[1] + d[2] * d[2], rmax2, inv_dr, n_bins);
}

// The sweep around the home cell c of a grid n: a direction with at least 3 cells visits c - 1, c, c + 1 (periodic), one with
// fewer visits every cell once (the rule of k_cell_pairs), so no cell appears twice and the full sweep meets every ordered pair
// of neighbouring cells exactly once.  cnt[d] is the number of steps along d; step k of direction d leads to the cell
// coordinate *to and has the sign s: k - 1 where the direction has 3 cells or more, to - c where it has fewer.  Seen from the
// other cell every sign is reversed, so "the first sign that is not zero is positive" takes exactly one of the two visits: for
// a grid of at least 3 cells each way these are 13 of the 26 neighbours.  All signs zero is the home cell itself.
ADMP_HD int rdf_sweep_count(int n_d) { return n_d >= 3 ? 3 : n_d; }
ADMP_HD int rdf_sweep_step(int n_d, int c_d, int k, int* to) {
  if (n_d >= 3) {
    const int t = c_d + k - 1;
    *to = t < 0 ? t + n_d : (t >= n_d ? t - n_d : t);
    return k - 1;
  }
  *to = k;
  return k - c_d;
}
// 0: the home cell, 1: taken by this home cell, -1: left to the other cell
ADMP_HD int rdf_sweep_take(int s0, int s1, int s2) {
  const int s = s0 != 0 ? s0 : (s1 != 0 ? s1 : s2);
  return s > 0 ? 1 : (s < 0 ? -1 : 0);
}

}  // namespace admp
