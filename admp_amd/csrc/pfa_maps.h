// Index maps of the two-level (Good-Thomas) direct DFT of pfa_kernels.hip: the split of an axis N = N1 * N2, position <->
// (n1, n2), and which frequency every slot of the slot-ordered spectrum holds.
// Host arithmetic (pfa_pos also on the device): the engine builds its tables with these, tests/hostshim drives them on the CPU.
#pragma once
#include "dft_math.h"

namespace admp {

struct PfaAxis { int N, N1, N2; };            // N1 = 1: plain direct lines

constexpr int kPfaMaxN1 = 32, kPfaMaxN2 = 160;

ADMP_HD int pfa_pos(const PfaAxis& a, int n1, int n2) { return (a.N2 * n1 + a.N1 * n2) % a.N; }

// split of one axis; lengths up to plain_max stay whole (N1 = 1).  false: this length neither fits the plain lines nor has a
// usable coprime split
inline bool pfa_split_at(int N, int plain_max, PfaAxis* out) {
  int p = largest_prime_factor(N), N2 = 1, m = N;
  while (m % p == 0) { N2 *= p; m /= p; }
  PfaAxis a;
  a.N = N;
  if (N <= plain_max || m == 1) { a.N1 = 1; a.N2 = N; }
  else { a.N1 = m; a.N2 = N2; }
  if (a.N2 > kPfaMaxN2 || a.N1 > kPfaMaxN1 || a.N2 < 2) return false;
  *out = a;
  return true;
}
inline void pfa_index_table(const PfaAxis& a, int* t) {      // t[n1 * N2 + n2] = position (low 16 bits) | n1 << 16
  for (int n1 = 0; n1 < a.N1; ++n1)
    for (int n2 = 0; n2 < a.N2; ++n2) t[n1 * a.N2 + n2] = pfa_pos(a, n1, n2) | (n1 << 16);
}
inline void pfa_freq_of_slot(const PfaAxis& a, int* f) {      // f[slot] = the frequency stored there
  for (int k1 = 0; k1 < a.N1; ++k1)
    for (int k2 = 0; k2 < a.N2; ++k2) {
      int k = k2;
      while (k % a.N1 != k1) k += a.N2;               // CRT by search (N1 <= 32 steps)
      f[pfa_pos(a, k1, k2)] = k;
    }
}
inline void pfa_freq_of_zcolumn(const PfaAxis& a, int* f) {   // f[cz] for the stored z half, cz = k2 * N1 + k1
  const int Kh2 = a.N2 / 2 + 1;
  for (int k2 = 0; k2 < Kh2; ++k2)
    for (int k1 = 0; k1 < a.N1; ++k1) {
      int k = k2;
      while (k % a.N1 != k1) k += a.N2;
      f[k2 * a.N1 + k1] = k;
    }
}

}  // namespace admp
