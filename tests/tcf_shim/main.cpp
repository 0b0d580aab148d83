// Stand-alone host program over the arithmetic and the plan of the time correlation functions (admp_amd/csrc/tcf_math.h,
// tcf_plan.h), the text the kernels of tcf_kernels.hip compile; tests/test_tcf_cpu.py compiles and runs it.
//   tcf_shim f|d sums < input   the frames one after the other as the three kernels take them, with a ring of float or double words:
//                               push per slot (tcf_unwrap, tcf_ring_word), then per tile and lag the terms of a lane's slots, the
//                               lanes of a wave by the shuffle tree, the waves in order, the tiles of a type in order.  Prints the
//                               accumulators (2 x n_types x n_lags) and then the jump word.
//     input (whitespace separated): n_atoms n_types n_lags tile_atoms n_tiles frames, slot_atom (n_tiles tile_atoms), tile_type
//     (n_tiles), then per frame the box (9, rows) and per atom r (3) and v (3)
//   tcf_shim plan N NSLOTS NTILES TILE NTYPES NLAGS FRAME
//                               prints "error <text>" or "ok threads slots_per_lane lags_now lag_blocks workgroups ring_slot
//                               scratch_bytes"
//   tcf_shim slots FRAMES L     prints "frame lag slot" for every lag every frame reaches (tcf_lags_reached, tcf_ring_slot)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tcf_math.h"
#include "tcf_plan.h"

namespace {

// x[0] after the steps of tcf_wave_sum: lane l adds lane l + o for o = 32, 16, .. 1 (a lane past the end returns the caller's own
// value, which never reaches lane 0)
double wave_sum(double* x) {
  for (int o = 32; o >= 1; o >>= 1)
    for (int l = 0; l + o < 64; ++l) x[l] += x[l + o];
  return x[0];
}

template <class T>
int sums() {
  int n = 0, n_types = 0, L = 0, ta = 0, n_tiles = 0, frames = 0;
  if (scanf("%d %d %d %d %d %d", &n, &n_types, &L, &ta, &n_tiles, &frames) != 6) return 2;
  if (n < 0 || n > (1 << 20) || n_tiles < 0 || n_tiles > 4096 || frames < 0 || frames > 4096 || L > 4096) return 2;
  const admp::TcfPlan chk = admp::tcf_make_plan(n, n_tiles * ta, n_tiles, ta, n_types, L, 0);
  if (chk.error) { fprintf(stderr, "%s\n", chk.error); return 2; }
  const int n_slots = n_tiles * ta;
  std::vector<int> slot_atom((size_t)n_slots + 1), tile_type((size_t)n_tiles + 1);
  for (int s = 0; s < n_slots; ++s)
    if (scanf("%d", &slot_atom[s]) != 1) return 2;
  for (int t = 0; t < n_tiles; ++t)
    if (scanf("%d", &tile_type[t]) != 1) return 2;
  const size_t S = (size_t)n_slots;
  std::vector<T> ring((size_t)L * 6 * S + 1, T(0)), last(3 * S + 1, T(0)), pos(3 * (size_t)n + 1), vel(3 * (size_t)n + 1);
  std::vector<double> unwrapped(3 * S + 1, 0.0), acc((size_t)2 * n_types * L, 0.0);
  unsigned long long jumps = 0;
  for (int64_t frame = 0; frame < frames; ++frame) {
    double h[9], inv[9];
    for (double& x : h)
      if (scanf("%lf", &x) != 1) return 2;
    for (int i = 0; i < n; ++i) {
      double x[6];
      if (scanf("%lf %lf %lf %lf %lf %lf", &x[0], &x[1], &x[2], &x[3], &x[4], &x[5]) != 6) return 2;
      for (int c = 0; c < 3; ++c) { pos[3 * (size_t)i + c] = (T)x[c]; vel[3 * (size_t)i + c] = (T)x[3 + c]; }
    }
    const double det = h[0] * (h[4] * h[8] - h[5] * h[7]) - h[1] * (h[3] * h[8] - h[5] * h[6]) + h[2] * (h[3] * h[7] - h[4] * h[6]);
    inv[0] = (h[4] * h[8] - h[5] * h[7]) / det; inv[1] = (h[2] * h[7] - h[1] * h[8]) / det; inv[2] = (h[1] * h[5] - h[2] * h[4]) / det;
    inv[3] = (h[5] * h[6] - h[3] * h[8]) / det; inv[4] = (h[0] * h[8] - h[2] * h[6]) / det; inv[5] = (h[2] * h[3] - h[0] * h[5]) / det;
    inv[6] = (h[3] * h[7] - h[4] * h[6]) / det; inv[7] = (h[1] * h[6] - h[0] * h[7]) / det; inv[8] = (h[0] * h[4] - h[1] * h[3]) / det;
    admp::Box<double> box;
    for (int k = 0; k < 9; ++k) { box.h[k] = h[k]; box.hinv[k] = inv[k]; }
    const admp::TcfPlan p = admp::tcf_make_plan(n, n_slots, n_tiles, ta, n_types, L, frame);
    if (p.error) return 2;
    // k_tcf_push
    T* row = ring.data() + (size_t)p.ring_slot * 6 * S;
    for (int s = 0; s < n_slots; ++s) {
      const int a = slot_atom[s];
      if (a < 0 || a >= n) continue;
      const size_t s3 = 3 * (size_t)s, a3 = 3 * (size_t)a;
      double d[3] = {0.0, 0.0, 0.0};
      if (frame != 0) {
        const double pd[3] = {(double)pos[a3], (double)pos[a3 + 1], (double)pos[a3 + 2]};
        const double ld[3] = {(double)last[s3], (double)last[s3 + 1], (double)last[s3 + 2]};
        for (int c = 0; c < 3; ++c) d[c] = unwrapped[s3 + c];
        if (admp::tcf_unwrap(box, pd, ld, d)) ++jumps;
      }
      for (int c = 0; c < 3; ++c) {
        unwrapped[s3 + c] = d[c];
        last[s3 + c] = pos[a3 + c];
        row[(size_t)c * S + s] = admp::tcf_ring_word<T>(d[c]);
        row[(size_t)(3 + c) * S + s] = vel[a3 + c];
      }
    }
    // k_tcf_lags
    std::vector<double> partial((size_t)2 * n_tiles * L + 1, 0.0);
    const int nw = p.threads / 64;
    for (int tile = 0; tile < n_tiles; ++tile) {
      if (tile_type[tile] < 0 || tile_type[tile] >= n_types) continue;
      const size_t t0 = (size_t)tile * ta;
      const T* cur = ring.data() + (size_t)p.ring_slot * 6 * S + t0;
      for (int lag = 0; lag < p.lags_now; ++lag) {
        const T* old = ring.data() + (size_t)admp::tcf_ring_slot(frame, lag, L) * 6 * S + t0;
        double tot[2] = {0.0, 0.0};
        for (int w = 0; w < nw; ++w) {
          double m[64], v[64];
          for (int l = 0; l < 64; ++l) {
            m[l] = v[l] = 0.0;
            for (int j = 0; j < p.slots_per_lane; ++j) {
              const int sl = w * 64 + l + j * p.threads;
              if (sl >= ta) continue;
              const int a = slot_atom[t0 + sl];
              if (a < 0 || a >= n) continue;
              if (lag != 0)
                m[l] += admp::tcf_msd_term(cur[sl], cur[S + sl], cur[2 * S + sl], old[sl], old[S + sl], old[2 * S + sl]);
              v[l] += admp::tcf_vacf_term(cur[3 * S + sl], cur[4 * S + sl], cur[5 * S + sl], old[3 * S + sl], old[4 * S + sl],
                                          old[5 * S + sl]);
            }
          }
          const double wm = wave_sum(m), wv = wave_sum(v);
          tot[0] = w == 0 ? wm : tot[0] + wm;
          tot[1] = w == 0 ? wv : tot[1] + wv;
        }
        for (int q = 0; q < 2; ++q) partial[((size_t)q * n_tiles + tile) * L + lag] = tot[q];
      }
    }
    // k_tcf_fold
    for (int q = 0; q < 2; ++q)
      for (int ty = 0; ty < n_types; ++ty)
        for (int lag = 0; lag < p.lags_now; ++lag) {
          double sum = 0.0;
          for (int t = 0; t < n_tiles; ++t)
            if (tile_type[t] == ty) sum += partial[((size_t)q * n_tiles + t) * L + lag];
          acc[((size_t)q * n_types + ty) * L + lag] += sum;
        }
  }
  for (double x : acc) printf("%.17g\n", x);
  printf("%llu\n", jumps);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 3 && (argv[1][0] == 'f' || argv[1][0] == 'd') && !strcmp(argv[2], "sums"))
    return argv[1][0] == 'f' ? sums<float>() : sums<double>();
  if (argc == 9 && !strcmp(argv[1], "plan")) {
    const admp::TcfPlan p = admp::tcf_make_plan(atoi(argv[2]), atoi(argv[3]), atoi(argv[4]), atoi(argv[5]), atoi(argv[6]), atoi(argv[7]),
                                                atoll(argv[8]));
    if (p.error) printf("error %s\n", p.error);
    else printf("ok %d %d %d %d %ld %d %zu\n", p.threads, p.slots_per_lane, p.lags_now, p.lag_blocks, p.workgroups, p.ring_slot, p.scratch_bytes);
    return 0;
  }
  if (argc == 4 && !strcmp(argv[1], "slots")) {
    const int frames = atoi(argv[2]), L = atoi(argv[3]);
    if (frames < 0 || frames > 4096 || L < 1) return 2;
    for (int64_t f = 0; f < frames; ++f)
      for (int k = 0; k < admp::tcf_lags_reached(f, L); ++k) printf("%lld %d %d\n", (long long)f, k, admp::tcf_ring_slot(f, k, L));
    return 0;
  }
  fprintf(stderr, "usage: %s f|d sums < input | plan N NSLOTS NTILES TILE NTYPES NLAGS FRAME | slots FRAMES L\n", argv[0]);
  return 2;
}
