// Host program around admp_amd/csrc/slab_plan.h for tests/test_slab_plan_cpu.py.  Input: any number of cases, each as
// `N me track bins_on` and kSlabMaxCols totals (the plan reads its first ncols).  Output per case: `refused <text>`, or lines
// `<name> <values...>` -- the plan (bound to 7 atoms, an order and a migrant array), then the segments -- closed by `end`.
#include <cstdint>
#include <cstdio>

#include "slab_plan.h"

template <class V>
static void line(const char* name, const V* v, int n) {
  std::printf("%s", name);
  for (int k = 0; k < n; ++k) std::printf(" %lld", (long long)v[k]);
  std::printf("\n");
}
static void segs(const char* name, const admp::SlabSegs& s) {
  char key[32];
  std::snprintf(key, sizeof key, "%s_off", name);
  line(key, s.off, s.n + 1);
  std::snprintf(key, sizeof key, "%s_col", name);
  line(key, s.col, s.n);
}

int main() {
  using namespace admp;
  for (;;) {
    int N, me, track, bins_on;
    const int got = std::scanf("%d %d %d %d", &N, &me, &track, &bins_on);
    if (got == EOF) return 0;
    if (got != 4 || N < 1 || me < 0 || me >= N) return 1;
    int totals[kSlabMaxCols];
    for (int k = 0; k < kSlabMaxCols; ++k)
      if (std::scanf("%d", &totals[k]) != 1) return 1;
    SlabColumnPlan p = slab_column_plan(N, me, track != 0, bins_on != 0);
    if (p.refused) { std::printf("refused %s\n", p.refused); continue; }
    if (p.cs.ncols > kSlabMaxCols) return 2;
    const int order = 0, mig = 0;
    p.bind(7, &order, &mig);
    const int head[7] = {p.cs.ncols, p.nranks, p.sb.N, p.sb.me, p.sb.c_home, p.c_rows, p.sb.c_act};
    line("head", head, 7);
    line("len", p.cs.len, p.cs.ncols);
    line("mask", p.cs.mask, p.cs.ncols);
    line("want", p.cs.want, p.cs.ncols);
    line("binned", p.cs.binned, p.cs.ncols);
    int seq[kSlabMaxCols], src[kSlabMaxCols];
    for (int c = 0; c < p.cs.ncols; ++c) {
      if ((p.cs.seq[c] && p.cs.seq[c] != &order) || (p.cs.src[c] && p.cs.src[c] != &mig)) return 3;
      seq[c] = p.cs.seq[c] ? 1 : 0; src[c] = p.cs.src[c] ? 1 : 0;
    }
    line("seq", seq, p.cs.ncols);
    line("src", src, p.cs.ncols);
    line("c_imp", p.sb.c_imp, kSlabMaxRanks);
    line("c_exp", p.sb.c_exp, kSlabMaxRanks);
    line("c_min", p.sb.c_min, kSlabMaxRanks);
    line("c_mout", p.sb.c_mout, kSlabMaxRanks);
    const SlabSegments s = slab_segments(p, totals);
    const int n[7] = {s.n_home, s.n_act, s.n_imp, s.n_exp, s.n_min, s.n_mout, s.buf_rows};
    line("n", n, 7);
    line("imp_cnt", s.imp_cnt, N);
    line("exp_cnt", s.exp_cnt, N);
    line("min_cnt", s.min_cnt, N);
    line("mout_cnt", s.mout_cnt, N);
    segs("imp", s.imp);
    segs("exp", s.exp);
    segs("min", s.min);
    segs("mout", s.mout);
    std::printf("end\n");
  }
}
