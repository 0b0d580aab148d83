// Launch shape of the direct-DFT line kernels and the plan of the x pass: how many lines (columns) a workgroup takes, how many
// tiles a y row has and how much LDS the launch asks for.  Host arithmetic with no device-only construct, in a header of its
// own (included by dft_lines.h) so that the host-compiled test shim can call it (tests/test_pair_rider_layout_cpu.py).
#pragma once
#include <stddef.h>

#include "dft_math.h"

namespace admp {

#ifndef ADMP_DFT_BLOCK
#define ADMP_DFT_BLOCK 256
#endif
constexpr int kDftBlock = ADMP_DFT_BLOCK;
constexpr size_t kDftLdsBudget = 60 * 1024;

// Two output pairs per thread (they share one read of the pair sums), one thread per output set.  Round 2 measured the
// alternatives on the 97^3 f64 mesh and dropped them (variants in the history): 1 or 4 output pairs per thread, and two
// lanes per output set (each summing half of the pair positions: x pass 36.8 -> 44.4 us) -- more, thinner threads do not
// help these latency-bound passes.  The kernels keep the two template parameters; one instantiation is compiled.
static inline int dft_kq() { return 2; }
static inline int dft_js() { return 1; }
// thread-tasks per line and lines (columns) per block
static inline int dft_tasks(int N, int KQ) { return (N / 2 + 1 + KQ - 1) / KQ; }
static inline int dft_cols(int N, int KQ, size_t bytes_per_col, size_t fixed_bytes) {
  int nc = (kDftBlock / dft_js()) / dft_tasks(N, KQ);
  if (nc < 1) nc = 1;
  while (nc > 1 && fixed_bytes + bytes_per_col * nc > kDftLdsBudget) --nc;
  return nc;
}

// LDS of an x pass over lines of N words of w bytes (a complex number is 2 words, a pair sum 4): per column of the tile and
// per workgroup.  Transform form (dft_x_conv_body): pair sums [H], x0, xn and the spectrum [N] per column, the twiddles [N]
// once.  Circulant form (dft_x_circ_body): pair sums [H], x0, xn and the extended table [circ_ext_len] per column.
static inline size_t dft_x_col_bytes(int N, size_t w, bool circ) {
  const size_t H = (size_t)((N - 1) / 2);
  return circ ? 4 * w * H + 2 * 2 * w + w * (size_t)circ_ext_len(N) : 4 * w * H + 2 * w * (size_t)(2 + N);
}
static inline size_t dft_x_fixed_bytes(int N, size_t w, bool circ) { return circ ? 0 : 2 * w * (size_t)N; }

// The x pass of a mesh K in words of w bytes: lines of N = K[0] points, Kh = K[2] / 2 + 1 columns per y row in tiles of NC
// (TK thread-tasks per column), nbx tiles per row, lds bytes of dynamic LDS per workgroup.
struct XPassPlan {
  int N, Kh, TK, NC, nbx;
  size_t lds;
};
static inline XPassPlan dft_x_plan(const int K[3], size_t w, bool circ) {
  XPassPlan p;
  p.N = K[0]; p.Kh = K[2] / 2 + 1; p.TK = dft_tasks(p.N, dft_kq());
  p.NC = dft_cols(p.N, dft_kq(), dft_x_col_bytes(p.N, w, circ), dft_x_fixed_bytes(p.N, w, circ));
  p.nbx = (p.Kh + p.NC - 1) / p.NC;
  p.lds = dft_x_fixed_bytes(p.N, w, circ) + dft_x_col_bytes(p.N, w, circ) * (size_t)p.NC;
  return p;
}

}  // namespace admp
