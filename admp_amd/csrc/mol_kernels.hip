// Molecular (centre-of-mass) cell scaling of the MD drivers (admp_amd/md.py MolecularCRescaleBarostat; md_mol_math.h has the
// scheme): groups of atoms are scaled as rigid bodies about their centres of mass, so constrained distances survive an
// application of the barostat, and the pressure counts the groups' kinetic energy and virial only.  A workgroup takes a tile
// of whole groups (mol_plan.h), one lane per atom: r, v, g and 1/m stay in its registers.
//
//   k_md_mol_sums   out[0..8] += sum_c M_c V_c (x) V_c, out[9..17] += sum_i R_c(i) (x) g_i, out[18..20] = the barostat's normals
//                   (layout and units of k_md_virial: the host code is shared)
//   k_md_mol_scale  r_i += (mu - 1) R_c(i), v_i += (1/mu - 1) V_c, in place
//
// Phases: every lane reads its anchor's position from memory (the first slot of its group; no other workgroup writes it),
// forms d and s and puts d, v, 1/m into LDS | barrier | ONE lane per group sums M, m d and m v in double in slot order over
// LDS and leaves M, sum m d / M, V_c there -- no float atomics, so r and v are bit-identical from run to run and for every tile
// capacity | barrier | every lane reads its group's words back.  k_md_mol_scale has no atomics at all; k_md_mol_sums adds its
// 18 words with one atomic per workgroup and word, after a workgroup reduction in double -- its launch is capped, a workgroup
// walks the tiles blockIdx.x, blockIdx.x + gridDim.x, ... and sums its share in registers first.
// LDS (64 banks of 4 B): the groups' words first (7 doubles per group), then d and v with slot a at words 3 a .. 3 a + 2
// (6 a .. in double) and 1/m.  Elementwise phases: stride 3 is odd in single; in double the 32 lanes of a 64-bit access group
// land on 32 different even banks.  Sum phase: lane c owns group c; for waters (slots 3 c ..) the lanes read d and v with a
// stride of 9 words (18 in double: distinct over a group of 32) and write with a stride of 14 words (2-way over 64 lanes).
#include <hip/hip_runtime.h>

#include "launch.h"
#include "md_math.h"
#include "md_mol_math.h"
#include "mol_plan.h"
#include "reduce.h"

namespace admp {

template <class T>
struct MolLds {
  double* grp;
  T *d, *v, *im;
};
template <class T>
__device__ __forceinline__ MolLds<T> mol_carve(unsigned char* raw, const MolDims& dims) {
  MolLds<T> L;
  L.grp = reinterpret_cast<double*>(raw);
  L.d = reinterpret_cast<T*>(L.grp + kMolGroupWords * dims.groups);
  L.v = L.d + 3 * dims.atoms;
  L.im = L.v + 3 * dims.atoms;
  return L;
}

// what both kernels do first: on return r, v, s, ra are the lane's own (zero in an idle lane), my the first word of its
// group in LDS, and every group of the tile has been summed (two barriers inside).  Returns the lane's atom, -1 in an idle lane.
template <class T, int THREADS>
__device__ __forceinline__ int mol_gather(const MolTiles& P, int t, const MolLds<T>& L, const T* pos, const T* vel, const T* inv_mass,
                                          const Box<T>& box, T r[3], T v[3], T s[3], T ra[3], int& my, int& n_groups) {
  const int tid = threadIdx.x;
  const int a0 = P.tile_atom0[t], n = P.tile_atom0[t + 1] - a0;      // (n <= tile capacity <= THREADS: one lane per atom)
  const int g0 = P.tile_grp0[t];
  n_groups = P.tile_grp0[t + 1] - g0;
  const bool mine = tid < n;
  int atom = -1;
  my = 0;
  for (int c = 0; c < 3; ++c) r[c] = v[c] = s[c] = ra[c] = T(0);
  if (mine) {
    atom = P.atom_id[a0 + tid];
    my = P.slot_grp[a0 + tid];
    const int anchor = P.atom_id[P.grp_atom0[g0 + my]];
    T d[3];
    for (int c = 0; c < 3; ++c) { r[c] = pos[3 * (size_t)atom + c]; v[c] = vel[3 * (size_t)atom + c]; ra[c] = pos[3 * (size_t)anchor + c]; }
    md_mol_image(box, r, ra, d, s);
    for (int c = 0; c < 3; ++c) { L.d[3 * tid + c] = d[c]; L.v[3 * tid + c] = v[c]; }
    L.im[tid] = inv_mass[atom];
  }
  __syncthreads();      // d, v and 1/m of the tile are in LDS
  if (tid < n_groups) {      // (a tile has at most as many groups as atoms)
    double w[kMolGroupWords];
    md_mol_group(L.d, L.v, L.im, P.grp_atom0[g0 + tid] - a0, P.grp_atom0[g0 + tid + 1] - a0, w);
    for (int k = 0; k < kMolGroupWords; ++k) L.grp[kMolGroupWords * tid + k] = w[k];
  }
  __syncthreads();      // the groups' words are in LDS
  return atom;
}

template <class T, int THREADS>
__global__ __launch_bounds__(THREADS) void k_md_mol_sums(MolTiles P, const T* __restrict__ pos, const T* __restrict__ vel,
                                                         const T* __restrict__ grad, const T* __restrict__ inv_mass, Box<T> box,
                                                         uint64_t seed, uint64_t step, double* __restrict__ out) {
  extern __shared__ __align__(8) unsigned char lds_raw[];
  const MolLds<T> L = mol_carve<T>(lds_raw, P.dims);
  const int tid = threadIdx.x;
  double acc[18];
#pragma unroll
  for (int w = 0; w < 18; ++w) acc[w] = 0.0;
  // the launch is capped (kMolSumsMaxBlocks): a workgroup walks its tiles and keeps its share of the 18 words in registers
  for (int t = blockIdx.x; t < P.n_tiles; t += gridDim.x) {
    T r[3], v[3], s[3], ra[3];
    int my, n_groups;
    const int atom = mol_gather<T, THREADS>(P, t, L, pos, vel, inv_mass, box, r, v, s, ra, my, n_groups);
    if (tid < n_groups) {      // the lane that summed group tid: M V (x) V
      const double* w = L.grp + kMolGroupWords * tid;
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) acc[3 * a + b] += w[0] * w[4 + a] * w[4 + b];
    }
    if (atom >= 0) {
      double Rc[3];
      md_mol_centre(ra, L.grp + kMolGroupWords * my, s, Rc);
      const double g[3] = {(double)grad[3 * (size_t)atom], (double)grad[3 * (size_t)atom + 1], (double)grad[3 * (size_t)atom + 2]};
#pragma unroll
      for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) acc[9 + 3 * a + b] += Rc[a] * g[b];
    }
    __syncthreads();      // every lane has read its group's words: the next tile may overwrite the LDS
  }
#pragma unroll
  for (int w = 0; w < 18; ++w) acc[w] = block_reduce_sum<THREADS>(acc[w]);
  if (tid == 0) {
#pragma unroll
    for (int w = 0; w < 18; ++w)
      if (acc[w] != 0.0) atomicAdd(&out[w], acc[w]);
    if (blockIdx.x == 0) {
      double xi[3];
      md_random_normals(seed, step, kStreamBarostat, 0u, xi);
      out[18] = xi[0]; out[19] = xi[1]; out[20] = xi[2];
    }
  }
}

// (pos is read at the anchors and written at the lane's own atom: no __restrict__; the reads precede the barriers of
// mol_gather, the writes follow them, and a tile's atoms belong to one workgroup)
template <class T, int THREADS>
__global__ __launch_bounds__(THREADS) void k_md_mol_scale(MolTiles P, T* pos, T* vel, const T* __restrict__ inv_mass, Box<T> box,
                                                          double mu_minus_1, double inv_mu_minus_1) {
  extern __shared__ __align__(8) unsigned char lds_raw[];
  const MolLds<T> L = mol_carve<T>(lds_raw, P.dims);
  T r[3], v[3], s[3], ra[3];
  int my, n_groups;
  const int atom = mol_gather<T, THREADS>(P, blockIdx.x, L, pos, vel, inv_mass, box, r, v, s, ra, my, n_groups);
  if (atom < 0) return;
  const double* w = L.grp + kMolGroupWords * my;
  double Rc[3];
  md_mol_centre(ra, w, s, Rc);
  md_mol_scale(r, v, Rc, w, mu_minus_1, inv_mu_minus_1);
  for (int c = 0; c < 3; ++c) { pos[3 * (size_t)atom + c] = r[c]; vel[3 * (size_t)atom + c] = v[c]; }
}

#define ADMP_MOL_GO(KERNEL, BLOCKS, ...)                                            \
  do {                                                                               \
    if (threads == 64) KERNEL<T, 64><<<BLOCKS, 64, lds, st>>>(__VA_ARGS__);          \
    else if (threads == 128) KERNEL<T, 128><<<BLOCKS, 128, lds, st>>>(__VA_ARGS__);  \
    else KERNEL<T, 256><<<BLOCKS, 256, lds, st>>>(__VA_ARGS__);                      \
  } while (0)

// The 18 words of k_md_mol_sums take one atomic per workgroup and word, all workgroups on the same 18 addresses: measured, a
// launch of one workgroup per tile spends about 0.12 us per workgroup on them whatever else it does (tools/md_mol_bench.py,
// DESIGN.md section 8), so the launch is capped and a workgroup walks several tiles.
constexpr int kMolSumsMaxBlocks = 256;      // of 128 / 256 / 512 / 1024 measured (profiles/README.md)

template <class T>
void launch_md_mol_sums(hipStream_t st, const MolTiles& P, int threads, const T* pos, const T* vel, const T* grad, const T* inv_mass,
                        const Box<T>& box, uint64_t seed, uint64_t step, double* out) {
  if (P.n_tiles <= 0) return;
  const size_t lds = mol_lds_bytes(P.dims, sizeof(T));
  const int blocks = P.n_tiles < kMolSumsMaxBlocks ? P.n_tiles : kMolSumsMaxBlocks;
  ADMP_MOL_GO(k_md_mol_sums, blocks, P, pos, vel, grad, inv_mass, box, seed, step, out);
}
template <class T>
void launch_md_mol_scale(hipStream_t st, const MolTiles& P, int threads, T* pos, T* vel, const T* inv_mass, const Box<T>& box,
                         double mu_minus_1, double inv_mu_minus_1) {
  if (P.n_tiles <= 0) return;
  const size_t lds = mol_lds_bytes(P.dims, sizeof(T));
  ADMP_MOL_GO(k_md_mol_scale, P.n_tiles, P, pos, vel, inv_mass, box, mu_minus_1, inv_mu_minus_1);
}
#undef ADMP_MOL_GO

#define INST(T)                                                                                                                     \
  template void launch_md_mol_sums<T>(hipStream_t, const MolTiles&, int, const T*, const T*, const T*, const T*, const Box<T>&, uint64_t, \
                                      uint64_t, double*);                                                                           \
  template void launch_md_mol_scale<T>(hipStream_t, const MolTiles&, int, T*, T*, const T*, const Box<T>&, double, double);
INST(float)
INST(double)
#undef INST

}  // namespace admp
