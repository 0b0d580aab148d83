// Host program around admp_amd/csrc/topology_plan.h for tests/test_topology_plan_cpu.py.  Input: max_group finish_block
// gather_run, then any number of topologies, each as `na groups_on` and na rows `axis_type z x y`.  Output: the six arrays of
// each topology, one line each (the count, then the values), in the order inv_ptr inv_idx grp_ptr rows_blk gath_blk grp_of.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "topology_plan.h"

static void line(const std::vector<int>& v) {
  std::printf("%zu", v.size());
  for (int x : v) std::printf(" %d", x);
  std::printf("\n");
}

int main() {
  int max_group, finish_block, gather_run;
  if (std::scanf("%d %d %d", &max_group, &finish_block, &gather_run) != 3) return 1;
  for (;;) {
    int na, groups_on;
    const int got = std::scanf("%d %d", &na, &groups_on);
    if (got == EOF) return 0;
    if (got != 2 || na <= 0) return 1;
    std::vector<int32_t> at((size_t)na), ai(3 * (size_t)na);
    for (int i = 0; i < na; ++i) {
      int t, z, x, y;
      if (std::scanf("%d %d %d %d", &t, &z, &x, &y) != 4) return 1;      // (a partial topology is an error)
      if (t < 0 || t > 5 || z < -1 || z >= na || x < -1 || x >= na || y < -1 || y >= na) return 2;   // admp_set_topology's checks
      at[i] = t; ai[3 * i] = z; ai[3 * i + 1] = x; ai[3 * i + 2] = y;
    }
    const admp::TopologyPlan p = admp::topology_plan(na, at.data(), ai.data(), max_group, finish_block, gather_run, groups_on != 0);
    line(p.inv_ptr); line(p.inv_idx); line(p.grp_ptr); line(p.rows_blk); line(p.gath_blk); line(p.grp_of);
  }
}
