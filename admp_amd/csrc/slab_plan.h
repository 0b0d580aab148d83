// The integer planning of a slab rank's decomposition (slab_decomp.hip runs it, slab_kernels.hip fills the columns): the plain
// constants and records the kernels take, which compaction column is which, and what the columns' totals mean for the per-peer
// lists and the exchange buffers.  Host-only, no HIP header: tests/slab_plan_shim/main.cpp compiles it alone and
// tests/test_slab_plan_cpu.py compares it with a restatement.
#pragma once
#include <algorithm>
#include <cstdint>

namespace admp {

// per-atom word of a rank's view of the decomposition (see slab_kernels.hip)
constexpr int kSlabHome = 1 << 30, kSlabPolar = 1 << 29;
constexpr int kSlabMaxRanks = 28, kSlabMaxCols = 3 + 4 * kSlabMaxRanks;
// columns of the ordered compaction: column c keeps x = seq[c][p] (seq[c] == nullptr: x = p), p < len[c], where
// (bits[x] & mask[c]) == want[c]
struct SlabCols {
  int ncols = 0;
  int len[kSlabMaxCols];
  const int* seq[kSlabMaxCols];
  const int* src[kSlabMaxCols];    // the flag words this column tests (nullptr: the `bits` array of the decomposition)
  int mask[kSlabMaxCols];
  int want[kSlabMaxCols];
  int binned[kSlabMaxCols];        // 1: the column is filled by the one-pass bin compaction (SlabBins), not by its own pass
};
// The per-peer columns of a decomposition -- imports from / exports to / atoms taken over from / given away to every rank --
// plus the home and polarizable-home columns, as BINS of one ordered compaction pass over the atoms (round 3 ran one pass over
// all atoms per column: 7 passes on 2 ranks, 31 on 8 -- the part of a rank's step that GREW with the rank count).  c_*: the
// column (index into SlabCols / totals / lists) a bin writes, -1 = absent.
struct SlabBins {
  int N = 0, me = 0;
  int c_home = -1, c_act = -1;
  int c_imp[kSlabMaxRanks], c_exp[kSlabMaxRanks], c_min[kSlabMaxRanks], c_mout[kSlabMaxRanks];
};
// segments of a joined per-peer list: segment s = column col[s] of the compaction, entries off[s] .. off[s+1]-1 of the result
struct SlabSegs {
  int n = 0;
  int off[kSlabMaxRanks + 1];
  int col[kSlabMaxRanks];
};

// The columns of one decomposition.  Only `rows` (the home rows in the table's order: a different sequence) takes a pass of its
// own; home / polarizable home / the per-peer import, export and migrant columns are bins of ONE pass over the atoms
// (slab_kernels.hip k_slab_bins; bins_on false, ADMP_SLAB_BINS=0: a pass per column as in round 3, for A/B and tests).
struct SlabColumnPlan {
  const char* refused = nullptr;   // why there is no plan (the text of the argument error), else nullptr
  int nranks = 0;
  SlabCols cs;
  SlabBins sb;                     // (sb.c_*[t] are the per-peer columns whether or not the bins are on)
  int c_rows = -1;
  // the device side of the columns: every column runs over na entries, `rows` over the table's order (nullptr: natural order),
  // the migrant columns test the words of mig instead of the decomposition's bits
  void bind(int na, const int* order, const int* mig) {
    for (int c = 0; c < cs.ncols; ++c) { cs.len[c] = na; cs.seq[c] = nullptr; cs.src[c] = nullptr; }
    cs.seq[c_rows] = order;
    for (int t = 0; t < kSlabMaxRanks; ++t) {
      if (sb.c_min[t] >= 0) cs.src[sb.c_min[t]] = mig;
      if (sb.c_mout[t] >= 0) cs.src[sb.c_mout[t]] = mig;
    }
  }
};
// Column order: home, rows, polarizable home, then per peer t != me ascending: import, export and -- track: the decomposition
// compares its owners with the previous one's -- migrants in, migrants out.
inline SlabColumnPlan slab_column_plan(int N, int me, bool track, bool bins_on) {
  SlabColumnPlan p;
  if (N > kSlabMaxRanks) { p.refused = "at most 28 slab ranks"; return p; }
  SlabCols& cs = p.cs;
  SlabBins& sb = p.sb;
  p.nranks = N;
  sb.N = bins_on ? N : 0; sb.me = me;
  auto col = [&](int mask, int want, bool binned) {
    cs.len[cs.ncols] = 0; cs.seq[cs.ncols] = nullptr; cs.src[cs.ncols] = nullptr;
    cs.mask[cs.ncols] = mask; cs.want[cs.ncols] = want; cs.binned[cs.ncols] = binned && bins_on ? 1 : 0;
    return cs.ncols++;
  };
  sb.c_home = col(kSlabHome, kSlabHome, true);
  p.c_rows = col(kSlabHome, kSlabHome, false);
  sb.c_act = col(kSlabHome | kSlabPolar, kSlabHome | kSlabPolar, true);
  for (int t = 0; t < kSlabMaxRanks; ++t) sb.c_imp[t] = sb.c_exp[t] = sb.c_min[t] = sb.c_mout[t] = -1;
  for (int t = 0; t < N; ++t) {
    if (t == me) continue;
    const int peer = 1 << t;       // readers of an atom this rank owns / owner of an atom it reads
    sb.c_imp[t] = col(kSlabHome | peer, peer, true);
    sb.c_exp[t] = col(kSlabHome | peer, kSlabHome | peer, true);
    if (track) {
      sb.c_min[t] = col(kSlabHome | peer, peer, true);
      sb.c_mout[t] = col(kSlabHome | peer, kSlabHome | peer, true);
    }
  }
  return p;
}

// What the totals of the columns say: atoms imported from / exported to / taken over from / given away to every rank, the
// segments that join the per-peer columns into one list each, and the rows the exchange buffers must hold.
struct SlabSegments {
  SlabSegs imp, exp, min, mout;
  int64_t imp_cnt[kSlabMaxRanks], exp_cnt[kSlabMaxRanks], min_cnt[kSlabMaxRanks], mout_cnt[kSlabMaxRanks];
  int n_home = 0, n_act = 0, n_imp = 0, n_exp = 0, n_min = 0, n_mout = 0;
  int buf_rows = 1;                // the longest of the four lists, at least 1
};
// totals: the host copy of the first plan.cs.ncols words the decomposition left (absent columns count nothing)
inline SlabSegments slab_segments(const SlabColumnPlan& plan, const int* totals) {
  SlabSegments s;
  s.n_home = totals[plan.sb.c_home];
  s.n_act = totals[plan.sb.c_act];
  // one per-peer list: the count of every rank (0 for this rank and for an absent column), its segments, its length
  auto join = [&](const int* c, SlabSegs& g, int64_t* cnt) {
    g.off[0] = 0;
    for (int t = 0; t < plan.nranks; ++t) {
      cnt[t] = c[t] < 0 ? 0 : totals[c[t]];
      if (c[t] < 0) continue;
      g.col[g.n] = c[t]; g.off[g.n + 1] = g.off[g.n] + totals[c[t]]; ++g.n;
    }
    return g.off[g.n];
  };
  s.n_imp = join(plan.sb.c_imp, s.imp, s.imp_cnt);
  s.n_exp = join(plan.sb.c_exp, s.exp, s.exp_cnt);
  s.n_min = join(plan.sb.c_min, s.min, s.min_cnt);
  s.n_mout = join(plan.sb.c_mout, s.mout, s.mout_cnt);
  s.buf_rows = std::max(1, std::max(std::max(s.n_imp, s.n_exp), std::max(s.n_min, s.n_mout)));
  return s;
}

}  // namespace admp
