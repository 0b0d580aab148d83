// Host build of the index maps of the two-level direct DFT, admp_amd/csrc/pfa_maps.h (tests/test_pfa_maps_cpu.py).
#include "../../admp_amd/csrc/pfa_maps.h"

using namespace admp;

extern "C" {
// out3 = {N, N1, N2}; returns 1 when the length has a usable split (or stays whole), 0 when not
int pfa_shim_split(int N, int plain_max, int* out3) {
  PfaAxis a;
  if (!pfa_split_at(N, plain_max, &a)) return 0;
  out3[0] = a.N; out3[1] = a.N1; out3[2] = a.N2;
  return 1;
}
int pfa_shim_pos(int N, int N1, int N2, int n1, int n2) { return pfa_pos(PfaAxis{N, N1, N2}, n1, n2); }
void pfa_shim_index_table(int N, int N1, int N2, int* t) { pfa_index_table(PfaAxis{N, N1, N2}, t); }
void pfa_shim_freq_of_slot(int N, int N1, int N2, int* f) { pfa_freq_of_slot(PfaAxis{N, N1, N2}, f); }
void pfa_shim_freq_of_zcolumn(int N, int N1, int N2, int* f) { pfa_freq_of_zcolumn(PfaAxis{N, N1, N2}, f); }
}
