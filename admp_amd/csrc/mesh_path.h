// Which path the k-space leg of a mesh takes (mesh_conv.hip MeshConv::ensure builds what the result needs): a pure function of
// the mesh, the ranks, the three switches and three facts the kernel files own.  Host-only, no HIP header:
// tests/mesh_path_shim/main.cpp compiles it alone and tests/test_mesh_path_cpu.py walks its input space.
#pragma once
#include <initializer_list>

namespace admp {

enum class MeshPath {
  Rocfft3D,       // one rank: rocFFT 3-D r2c, k_kspace, rocFFT 3-D c2r
  FusedX,         // one rank, power-of-two K[0]: rocFFT y-z planes around the fused x pass (fftx_kernels.hip)
  DirectPlanes,   // one rank, a Bluestein dimension, every dimension <= 160: plane kernels + x pass (dft_kernels.hip)
  DirectLines,    // ... whose planes do not fit the LDS: z, y, x line kernels
  TwoLevel,       // one rank, a Bluestein dimension too long for plain lines: split N = N1 * N2 (pfa_kernels.hip)
  SlabRocfftX,    // slab rank: batched rocFFT y-z planes, transposes, rocFFT x lines + k_kspace
  SlabFusedX      // slab rank: ... with the fused x pass on the transposed layout
};

struct MeshPathIn {
  int K[3];
  int snranks;          // ranks of the slab decomposition (1: the whole mesh is local)
  int dft_mode;         // ADMP_DFT: -1 (unset) the rule below, 0 never a direct form, 1 the direct form for any mesh with all
                        // dimensions <= 160, 2 the two-level form for any mesh it can split, else as 1 (tests)
  bool pfa_on;          // ADMP_PFA
  bool fused_x_on;      // ADMP_FUSED_X
  bool fftx_ok;         // fftx_usable(K[0])
  bool splits;          // pfa_split takes all three dimensions
  bool zy_fits;         // dft_zy_fits<T>(K)
};

// rocFFT needs Bluestein's algorithm for a length with a prime factor above 13
inline bool mesh_dim_hard(int n) {
  for (int p : {2, 3, 5, 7, 11, 13})
    while (n > 1 && n % p == 0) n /= p;
  return n > 1;
}

inline MeshPath mesh_path(const MeshPathIn& in) {
  const bool fx = in.fused_x_on && in.fftx_ok;
  if (in.snranks > 1) return fx ? MeshPath::SlabFusedX : MeshPath::SlabRocfftX;      // slabs never take the direct forms
  if (in.dft_mode != 0) {
    bool small = true, hard = false;      // small enough for O(N^2) lines; some dimension is hard for rocFFT
    for (int d = 0; d < 3; ++d) {
      small = small && in.K[d] >= 2 && in.K[d] <= 160;
      hard = hard || mesh_dim_hard(in.K[d]);
    }
    const bool split = in.pfa_on && in.splits;
    if (split && (in.dft_mode == 2 || (!small && hard))) return MeshPath::TwoLevel;
    if (small && (hard || in.dft_mode == 1 || in.dft_mode == 2)) return in.zy_fits ? MeshPath::DirectPlanes : MeshPath::DirectLines;
  }
  return fx ? MeshPath::FusedX : MeshPath::Rocfft3D;
}

inline const char* mesh_path_name(MeshPath p) {
  switch (p) {
    case MeshPath::Rocfft3D: return "Rocfft3D";
    case MeshPath::FusedX: return "FusedX";
    case MeshPath::DirectPlanes: return "DirectPlanes";
    case MeshPath::DirectLines: return "DirectLines";
    case MeshPath::TwoLevel: return "TwoLevel";
    case MeshPath::SlabRocfftX: return "SlabRocfftX";
    case MeshPath::SlabFusedX: return "SlabFusedX";
  }
  return "?";
}

}  // namespace admp
