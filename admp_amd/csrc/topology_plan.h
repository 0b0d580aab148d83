// What admp_set_topology derives from the frame definitions (engine.hip uploads it, launch.h Topology describes it): the
// inverse frame map and, where the frames allow them, the frame groups with their runs.  Host-only, no HIP header:
// tests/topology_shim/main.cpp compiles it alone and tests/test_topology_plan_cpu.py compares it with
// tests/site_ref.py group_layout.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

namespace admp {

// the axis rules that decide which of a site's three axis atoms its frame uses (frame_math.h AxisType, checked in engine.hip)
constexpr int kTopoZBisect = 2, kTopoThreeFold = 3, kTopoZonly = 4, kTopoNoAxis = 5;

struct TopologyPlan {
  std::vector<int> inv_ptr, inv_idx;                     // na + 1; the sites whose frame involves each atom
  std::vector<int> grp_ptr, rows_blk, gath_blk, grp_of;   // empty: the topology is not made of groups (or groups are off)
};

// axis_type in 0..5 and axis_idx in -1..na-1 (3 per atom), as admp_set_topology has checked them; max_group, finish_block,
// gather_run: kMaxGroup, kFinishBlock, kGatherRun of launch.h; groups_on: ADMP_FINISH_GROUPS
inline TopologyPlan topology_plan(int na, const int32_t* at, const int32_t* ai, int max_group, int finish_block,
                                  int gather_run, bool groups_on) {
  TopologyPlan p;
  // the atoms site i takes its frame from: z, x (all rules but Zonly), y (ZBisect, ThreeFold); none for a site without a frame
  auto members = [&](int i, int mem[3]) {
    if (at[i] == kTopoNoAxis || ai[3 * i] < 0) return false;
    mem[0] = ai[3 * i];
    mem[1] = at[i] != kTopoZonly ? ai[3 * i + 1] : -1;
    mem[2] = (at[i] == kTopoZBisect || at[i] == kTopoThreeFold) ? ai[3 * i + 2] : -1;
    return true;
  };
  {   // inverse frame map for the atomics-free closing kernel
    std::vector<std::vector<int>> inv(na);
    for (int i = 0; i < na; ++i) {
      int mem[4] = {i, -1, -1, -1};
      if (!members(i, mem + 1)) { inv[i].push_back(i); continue; }
      for (int m = 0; m < 4; ++m) {
        if (mem[m] < 0) continue;
        bool dup = false;
        for (int q = 0; q < m; ++q) dup = dup || mem[q] == mem[m];
        if (!dup) inv[mem[m]].push_back(i);
      }
    }
    p.inv_ptr.assign((size_t)na + 1, 0);
    for (int a = 0; a < na; ++a) {
      p.inv_ptr[a + 1] = p.inv_ptr[a] + (int)inv[a].size();
      p.inv_idx.insert(p.inv_idx.end(), inv[a].begin(), inv[a].end());
    }
  }
  // frame groups (see Topology): union-find over "site i uses atom m in its frame"
  std::vector<int> parent(na);
  for (int i = 0; i < na; ++i) parent[i] = i;
  auto find = [&](int a) { while (parent[a] != a) { parent[a] = parent[parent[a]]; a = parent[a]; } return a; };
  for (int i = 0; i < na; ++i) {
    int mem[3];
    if (!members(i, mem)) continue;
    for (int m = 0; m < 3; ++m)
      if (mem[m] >= 0) { const int a = find(i), b = find(mem[m]); if (a != b) parent[std::max(a, b)] = std::min(a, b); }
  }
  // the root of a component is its lowest atom: components are runs of consecutive atoms iff root(i) is
  // non-decreasing in i and every run is short enough
  std::vector<int> gp;
  bool ok = true;
  int prev_root = -1;
  for (int i = 0; i < na && ok; ++i) {
    const int r = find(i);
    if (r != prev_root) {
      if (r != i) ok = false;                      // joins an earlier, already closed run
      gp.push_back(i);
      prev_root = r;
    } else if (i - r >= max_group) ok = false;
  }
  gp.push_back(na);
  if (!ok || !groups_on) return p;
  const int ngroups = (int)gp.size() - 1;
  // row form: workgroups of whole groups (greedy runs of at most finish_block atoms), group record per atom; the same cut
  // into runs of at most gather_run atoms for the gather with the closing epilogue
  p.rows_blk.assign(1, 0);
  p.gath_blk.assign(1, 0);
  p.grp_of.resize((size_t)na);
  for (int gi = 0; gi < ngroups; ++gi) {
    const int a0 = gp[gi], n = gp[gi + 1] - a0;
    if (gp[gi + 1] - p.rows_blk.back() > finish_block) p.rows_blk.push_back(a0);
    if (gp[gi + 1] - p.gath_blk.back() > gather_run) p.gath_blk.push_back(a0);
    for (int m = 0; m < n; ++m) p.grp_of[(size_t)a0 + m] = (a0 << 2) | (n - 1);
  }
  p.rows_blk.push_back(na);
  p.gath_blk.push_back(na);
  p.grp_ptr.swap(gp);
  return p;
}

}  // namespace admp
