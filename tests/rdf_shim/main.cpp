// Stand-alone host program over the arithmetic and the plan of the radial distribution functions (admp_amd/csrc/rdf_math.h,
// rdf_plan.h), the text the kernels of rdf_kernels.hip compile; tests/test_rdf_cpu.py compiles and runs it.
//   rdf_shim f|d h < input   every pair i < j as a lane tests it (rdf_pair_channel, rdf_pair_bin) in float or double arithmetic;
//                            prints the histogram, channels x n_bins counts
//   rdf_shim f|d r < input   prints "i j r" for every counted pair with r2 < rmax2, r = sqrt(r2) in that arithmetic
//     input (whitespace separated): n_atoms n_types n_bins r_max, box (9, rows), then per atom r (3) and the tag
//   rdf_shim tiles NT        prints "w I J" for every workgroup w of NT tiles (rdf_tri_pair)
//   rdf_shim sweep G0 G1 G2  prints "home cell take" for every cell a home cell visits and does not leave to the other cell
//                            (take 0: the home cell itself, 1: a neighbour)
//   rdf_shim plan N H0 H1 H2 RMAX NTYPES NBINS REALBYTES FORCE
//                            prints "error <text>" or "ok form n_tiles g0 g1 g2 n_cells workgroups lds_bytes counters"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "rdf_plan.h"

namespace {

template <class T>
int run(char mode) {
  int n = 0, n_types = 0, n_bins = 0;
  double r_max = 0.0, h[9], inv[9];
  if (scanf("%d %d %d %lf", &n, &n_types, &n_bins, &r_max) != 4 || n < 0 || n > (1 << 20)) return 2;
  if (n_types < 1 || n_types > admp::kRdfMaxTypes || n_bins < 1 || (long)admp::rdf_channels(n_types) * n_bins > admp::kRdfMaxCounters) return 2;
  for (double& x : h)
    if (scanf("%lf", &x) != 1) return 2;
  const size_t N = (size_t)n;
  std::vector<T> R(3 * N + 1);
  std::vector<int> tag(N + 1);
  for (size_t i = 0; i < N; ++i) {
    double x[3];
    if (scanf("%lf %lf %lf %d", &x[0], &x[1], &x[2], &tag[i]) != 4) return 2;
    for (int c = 0; c < 3; ++c) R[3 * i + c] = (T)x[c];
  }
  const double det = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
  inv[0] = (h[4] * h[8] - h[5] * h[7]) / det; inv[1] = (h[2] * h[7] - h[1] * h[8]) / det; inv[2] = (h[1] * h[5] - h[2] * h[4]) / det;
  inv[3] = (h[5] * h[6] - h[3] * h[8]) / det; inv[4] = (h[0] * h[8] - h[2] * h[6]) / det; inv[5] = (h[2] * h[3] - h[0] * h[5]) / det;
  inv[6] = (h[3] * h[7] - h[4] * h[6]) / det; inv[7] = (h[1] * h[6] - h[0] * h[7]) / det; inv[8] = (h[0] * h[4] - h[1] * h[3]) / det;
  admp::Box<T> box;
  for (int k = 0; k < 9; ++k) { box.h[k] = (T)h[k]; box.hinv[k] = (T)inv[k]; }
  // (the two scalars as launch_rdf makes them)
  const T rmax2 = (T)(r_max * r_max), inv_dr = (T)((double)n_bins / r_max);
  std::vector<unsigned long long> hist((size_t)admp::rdf_channels(n_types) * n_bins, 0ull);
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      const int ch = admp::rdf_pair_channel(tag[i], tag[j], n_types);
      if (ch < 0) continue;
      if (mode == 'h') {
        const int b = admp::rdf_pair_bin(box, &R[3 * (size_t)i], &R[3 * (size_t)j], rmax2, inv_dr, n_bins);
        if (b >= 0) hist[(size_t)ch * n_bins + b] += 1;
      } else {
        T d[3] = {R[3 * (size_t)i] - R[3 * (size_t)j], R[3 * (size_t)i + 1] - R[3 * (size_t)j + 1], R[3 * (size_t)i + 2] - R[3 * (size_t)j + 2]};
        admp::min_image(box, d);
        const T r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        if (r2 < rmax2) printf("%d %d %.17g\n", i, j, (double)admp::m_sqrt(r2));
      }
    }
  if (mode == 'h')
    for (unsigned long long v : hist) printf("%llu\n", v);
  return 0;
}

int tiles(int nt) {
  if (nt < 1 || nt > 4096) return 2;
  for (int w = 0; w < nt * (nt + 1) / 2; ++w) {
    int I, J;
    admp::rdf_tri_pair(w, nt, &I, &J);
    printf("%d %d %d\n", w, I, J);
  }
  return 0;
}

// the loops of k_rdf_cells over the cells around every home cell
int sweep(const int g[3]) {
  for (int d = 0; d < 3; ++d)
    if (g[d] < 1 || g[d] > 64) return 2;
  for (int home = 0; home < g[0] * g[1] * g[2]; ++home) {
    const int c[3] = {home / g[2] / g[1], home / g[2] % g[1], home % g[2]};
    for (int a = 0; a < admp::rdf_sweep_count(g[0]); ++a)
      for (int b = 0; b < admp::rdf_sweep_count(g[1]); ++b)
        for (int e = 0; e < admp::rdf_sweep_count(g[2]); ++e) {
          int t0, t1, t2;
          const int s0 = admp::rdf_sweep_step(g[0], c[0], a, &t0), s1 = admp::rdf_sweep_step(g[1], c[1], b, &t1),
                    s2 = admp::rdf_sweep_step(g[2], c[2], e, &t2);
          const int take = admp::rdf_sweep_take(s0, s1, s2);
          if (take >= 0) printf("%d %d %d\n", home, (t0 * g[1] + t1) * g[2] + t2, take);
        }
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && (argv[1][0] == 'f' || argv[1][0] == 'd') && (argv[2][0] == 'h' || argv[2][0] == 'r'))
    return argv[1][0] == 'f' ? run<float>(argv[2][0]) : run<double>(argv[2][0]);
  if (argc == 3 && !strcmp(argv[1], "tiles")) return tiles(atoi(argv[2]));
  if (argc == 5 && !strcmp(argv[1], "sweep")) {
    const int g[3] = {atoi(argv[2]), atoi(argv[3]), atoi(argv[4])};
    return sweep(g);
  }
  if (argc == 11 && !strcmp(argv[1], "plan")) {
    const double heights[3] = {atof(argv[3]), atof(argv[4]), atof(argv[5])};
    const admp::RdfPlan p = admp::rdf_make_plan(atoi(argv[2]), heights, atof(argv[6]), atoi(argv[7]), atoi(argv[8]), (size_t)atoi(argv[9]),
                                                atoi(argv[10]));
    if (p.error) printf("error %s\n", p.error);
    else printf("ok %d %d %d %d %d %ld %ld %zu %d\n", p.form, p.n_tiles, p.grid[0], p.grid[1], p.grid[2], p.n_cells, p.workgroups, p.lds_bytes, p.counters);
    return 0;
  }
  fprintf(stderr, "usage: %s f|d h|r < input | tiles NT | sweep G0 G1 G2 | plan N H0 H1 H2 RMAX NTYPES NBINS REALBYTES FORCE\n", argv[0]);
  return 2;
}
