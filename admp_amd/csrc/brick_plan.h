// The brick rule of the LDS-tiled spread (recip_kernels.hip, disp_kernels.hip; k_prepare_sites writes the codes): how a mesh is
// cut into bricks and how an atom's stencil is binned.  Plain C++ when compiled without HIP, so that
// tests/hostshim/brick_plan_shim.cpp can compile it for the host and tests/test_mesh_ref_cpu.py can check its restatement.
#pragma once

#if defined(__HIPCC__)
#define ADMP_BRICK_HD __host__ __device__ inline
#else
#define ADMP_BRICK_HD inline
#endif

namespace admp {

// Mesh bricks for the LDS-tiled spread: dimension d is cut into nb[d] = ceil(K/16) bricks of 15..16
// (>= 6) points, brick b covering [b*K/nb, (b+1)*K/nb).  An atom is binned by the brick of its
// lowest stencil point; its 6-point stencil then reaches at most the next brick.
struct BrickGrid {
  int nb[3];
  int ncell;
};
ADMP_BRICK_HD BrickGrid make_bricks(const int K[3]) {
  BrickGrid b;
  for (int d = 0; d < 3; ++d) b.nb[d] = (K[d] + 15) / 16;
  b.ncell = b.nb[0] * b.nb[1] * b.nb[2];
  return b;
}
// brick index of mesh index i on an axis of K points cut into nb bricks [b*K/nb, (b+1)*K/nb)
ADMP_BRICK_HD int brick_of(int i, int nb, int K) { return ((i + 1) * nb - 1) / K; }
// Packed brick code of a stencil with lowest indices base[3]: 9 bits per axis = brick of `base`, bits 27..29 = the
// stencil (6 points) reaches into the next brick on that axis.  Computed once per atom (the integer divisions are the
// expensive part of binning) by k_prepare_sites, stored in the .w of the atom's int4 base record.
ADMP_BRICK_HD int brick_code(const int base[3], const int dims[3], const BrickGrid& bg) {
  int code = 0;
  for (int d = 0; d < 3; ++d) {
    const int b = brick_of(base[d], bg.nb[d], dims[d]);
    const int end = ((b + 1) * dims[d]) / bg.nb[d];          // first index past the brick of `base`
    code |= b << (9 * d);
    if (bg.nb[d] > 1 && base[d] + 5 >= end) code |= 1 << (27 + d);
  }
  return code;
}

}  // namespace admp
