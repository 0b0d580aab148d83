// Host build of the circulant x-pass arithmetic of admp_amd/csrc/dft_math.h (tests/test_dft_circulant_cpu.py).
#include <cstdint>
#include <vector>

#include "../../admp_amd/csrc/dft_math.h"

using namespace admp;

namespace {

// G[N] (double) -> the column's first circulant column c[0..N/2] rounded to T (returned as double); returns 1 when the
// column, as stored in T, passes circ_column_even
template <class T>
int table(int N, const double* G, double* c) {
  std::vector<T> g(N);
  for (int k = 0; k < N; ++k) g[k] = (T)G[k];
  for (int d = 0; d <= N / 2; ++d)
    c[d] = (double)(T)circ_table_entry(N, d, (double)g[0], [&](int k) { return (double)g[k] + (double)g[N - k]; },
                                       (N & 1) ? 0.0 : (double)g[N / 2], [&](int m) { return circ_cos(m, N); });
  return circ_column_even(N, [&](int k) { return (double)g[k]; }, sizeof(T) == 4 ? 0x1p-24 : 0x1p-53) ? 1 : 0;
}

// one line x[N] (re, im interleaved) through circ_pair_outputs with the thread layout of the kernels (KQ = 2, TK tasks);
// out[N] interleaved, *energy = sum_x Re(conj(in_x) out_x) as the kernels sum it
template <class T>
void apply(int N, const double* c, const double* x, double* out, double* energy) {
  constexpr int KQ = 2;
  const int H = (N - 1) / 2, Kh = N / 2 + 1, TK = (Kh + KQ - 1) / KQ, L = circ_ext_len(N);
  std::vector<T> cext(L);
  for (int r = 0; r < L; ++r) cext[r] = (T)c[circ_fold(r - N / 2, N)];
  std::vector<PairCx<T>> ab(H > 0 ? H : 1);
  for (int j = 0; j < H; ++j) {
    const T are = (T)x[2 * (1 + j)], aim = (T)x[2 * (1 + j) + 1], bre = (T)x[2 * (N - 1 - j)], bim = (T)x[2 * (N - 1 - j) + 1];
    ab[j] = PairCx<T>{are + bre, aim + bim, are - bre, aim - bim};
  }
  const Cx<T> x0{(T)x[0], (T)x[1]};
  const Cx<T> xn = (N & 1) ? Cx<T>{T(0), T(0)} : Cx<T>{(T)x[N], (T)x[N + 1]};
  double e = 0.0;
  for (int g = 0; g < TK; ++g) {
    int i[KQ];
    for (int q = 0; q < KQ; ++q) i[q] = (g + q * TK < Kh) ? g + q * TK : 0;
    Cx<T> P[KQ], M[KQ];
    circ_pair_outputs<T, KQ>(N, i, 1, cext.data() + N / 2, 1, ab.data(), x0, xn, P, M);
    for (int q = 0; q < KQ; ++q) {
      const int iq = g + q * TK;
      if (iq >= Kh) continue;
      const bool single = iq == 0 || 2 * iq == N;
      e += circ_pair_energy<T>(N, iq, P[q], M[q], ab[single ? 0 : iq - 1], x0, xn);
      out[2 * iq] = (double)(T(0.5) * (P[q].re + M[q].re));
      out[2 * iq + 1] = (double)(T(0.5) * (P[q].im + M[q].im));
      if (!single) {
        out[2 * (N - iq)] = (double)(T(0.5) * (P[q].re - M[q].re));
        out[2 * (N - iq) + 1] = (double)(T(0.5) * (P[q].im - M[q].im));
      }
    }
  }
  *energy = e;
}

}  // namespace

extern "C" {
int circ_table(int f32, int N, const double* G, double* c) { return f32 ? table<float>(N, G, c) : table<double>(N, G, c); }
void circ_apply(int f32, int N, const double* c, const double* x, double* out, double* energy) {
  if (f32) apply<float>(N, c, x, out, energy);
  else apply<double>(N, c, x, out, energy);
}
}
