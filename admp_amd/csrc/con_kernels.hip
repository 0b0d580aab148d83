// Pairwise distance constraints of the MD drivers (SHAKE / RATTLE inside the two halves of a BAOAB step; md_con_math.h has the
// scheme).  The constraints of a cluster touch only its atoms, so a workgroup takes a tile of whole clusters (con_plan.h) and
// keeps what the solve reads and writes in LDS.  One lane per atom for the elementwise work: r0, v, the unconstrained
// displacement and 1/m stay in its registers.  The solve sits between two barriers: ONE lane per cluster sweeps the cluster's
// constraints sequentially in the plan's order over LDS -- no float atomics, so r and v are bit-identical from run to run and
// for every tile capacity.  A capacity of up to 64 atoms is one wavefront (THREADS = 64): the workgroup barriers are then
// plain LDS waits.
//
//   k_con_step     first half: B, A-O-A on the displacement, SHAKE on it, v += (delta - delta_u) / dt, r = r0 + delta
//   k_con_kick     second half: B (optional), RATTLE on v, optionally sum m v^2 / 2 of the result
//   k_con_project  pos moved onto the constraints along the directions of ref (no velocities)
//
// Phases of a kernel: lists -> LDS | positions -> LDS (x) | barrier | s (and in a projection b) per constraint from x | barrier
// | the solved vector -> x | barrier | solve | barrier | lanes read x back.  s is computed once per call.
// LDS (64 banks of 4 B): x keeps slot a at words 3 a .. 3 a + 2 (6 a .. in double), s and b keep constraint q at 3 q ..
// likewise, d^2 and 1/m are one word (two) per item, the slots two ints per constraint.  Elementwise phases: in single
// precision the stride 3 is odd -- no conflict; in double the 32 lanes of a 64-bit access group land on 32 different even
// banks (6 a mod 64).  Solve phase: lane c owns cluster c, whose items follow the topology; for rigid waters (atom slots 3 c ..,
// constraints 3 c ..) the lanes read x and s with a stride of 9 words (18 in double: distinct over a group of 32), d^2 with
// 3, and the slots with 6 ints, 2-way over 64 lanes -- no padding is needed.
#include <hip/hip_runtime.h>

#include "con_plan.h"
#include "launch.h"
#include "md_con_math.h"
#include "reduce.h"

namespace admp {

template <class T>
struct ConLds {
  T *x, *im, *d2, *s, *b;
  int *slot, *ccon;
};
// carved for the largest tile (P.dims), reals first; without a base the SHAKE base vector is s itself
template <class T>
__device__ __forceinline__ ConLds<T> con_carve(unsigned char* raw, const ConDims& d, bool with_base) {
  ConLds<T> L;
  L.x = reinterpret_cast<T*>(raw);
  L.im = L.x + 3 * d.atoms;
  L.d2 = L.im + d.atoms;
  L.s = L.d2 + d.cons;
  L.b = with_base ? L.s + 3 * d.cons : L.s;
  L.slot = reinterpret_cast<int*>(L.s + (with_base ? 6 : 3) * d.cons);
  L.ccon = L.slot + 2 * d.cons;
  return L;
}

// what every kernel knows of its tile
struct ConTile {
  int a0, n, ncl, nq;
};
template <class T, int THREADS>
__device__ __forceinline__ ConTile con_load_lists(const ConTiles<T>& P, const ConLds<T>& L) {
  const int t = blockIdx.x, tid = threadIdx.x;
  ConTile c;
  c.a0 = P.tile_atom0[t]; c.n = P.tile_atom0[t + 1] - c.a0;
  const int k0 = P.tile_clu0[t];
  c.ncl = P.tile_clu0[t + 1] - k0;
  const int q0 = P.clu_con0[k0];
  c.nq = P.clu_con0[k0 + c.ncl] - q0;
  for (int k = tid; k < 2 * c.nq; k += THREADS) L.slot[k] = P.con_slot[2 * (size_t)q0 + k];
  for (int k = tid; k < c.nq; k += THREADS) L.d2[k] = P.con_d2[(size_t)q0 + k];
  for (int k = tid; k <= c.ncl; k += THREADS) L.ccon[k] = P.clu_con0[k0 + k] - q0;
  return c;
}
// out[3 q ..] = minimum-image vector of constraint q between the positions in x (the slots are in LDS: after a barrier)
template <class T, int THREADS>
__device__ __forceinline__ void con_vectors(const ConLds<T>& L, int nq, const Box<T>& box, T* out) {
  for (int q = threadIdx.x; q < nq; q += THREADS) {
    T s[3];
    md_con_vector(box, L.x + 3 * L.slot[2 * q], L.x + 3 * L.slot[2 * q + 1], s);
    for (int c = 0; c < 3; ++c) out[3 * q + c] = s[c];
  }
}
// counters[0] += clusters that stopped unconverged, counters[1] = max(sweeps of a cluster): one atomic per word and workgroup
template <int THREADS>
__device__ __forceinline__ void con_count(int* counters, bool failed, int sweeps) {
  if (!counters) return;
  const double nf = block_reduce_sum<THREADS>(failed ? 1.0 : 0.0);
  const double ms = block_reduce_max<THREADS>((double)sweeps);
  if (threadIdx.x == 0) {
    if (nf != 0.0) atomicAdd(&counters[0], (int)nf);
    if (ms != 0.0) atomicMax(&counters[1], (int)ms);
  }
}

template <class T, int THREADS>
__global__ __launch_bounds__(THREADS) void k_con_step(ConTiles<T> P, T* __restrict__ pos, T* __restrict__ vel,
                                                      const T* __restrict__ grad, const T* __restrict__ inv_mass, Box<T> box,
                                                      T half_dt_acc, T half_dt, T dt, T c1, T c2sq_kT_acc, uint64_t seed, uint64_t step,
                                                      T tol2, int max_sweeps, int* counters) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const ConLds<T> L = con_carve<T>(lds_raw, P.dims, false);
  const int tid = threadIdx.x;
  const ConTile tile = con_load_lists<T, THREADS>(P, L);
  const bool mine = tid < tile.n;      // (n <= tile capacity <= THREADS: one lane per atom)
  const int atom = mine ? P.atom_id[tile.a0 + tid] : 0;
  T r0[3] = {T(0), T(0), T(0)}, v[3] = {T(0), T(0), T(0)}, du[3] = {T(0), T(0), T(0)};
  if (mine) {
    const T im = inv_mass[atom];
    T g[3];
    for (int c = 0; c < 3; ++c) { r0[c] = pos[3 * (size_t)atom + c]; v[c] = vel[3 * (size_t)atom + c]; g[c] = grad[3 * (size_t)atom + c]; }
    md_con_half_step(v, du, g, im, half_dt_acc, half_dt, c1 < T(1), c1, m_sqrt(c2sq_kT_acc * im), seed, step, (uint32_t)atom);
    for (int c = 0; c < 3; ++c) L.x[3 * tid + c] = r0[c];
    L.im[tid] = im;
  }
  __syncthreads();      // r0, 1/m and the lists are in LDS
  con_vectors<T, THREADS>(L, tile.nq, box, L.s);
  __syncthreads();      // every s has read r0
  if (mine)
    for (int c = 0; c < 3; ++c) L.x[3 * tid + c] = du[c];
  __syncthreads();      // the displacements and s are in LDS
  bool failed = false;
  int sweeps = 0;
  if (tid < tile.ncl)      // (a tile has at most as many clusters as atoms)
    sweeps = md_con_solve_shake(L.x, L.im, L.slot, L.d2, L.s, L.s, L.ccon[tid], L.ccon[tid + 1], tol2, max_sweeps, failed);
  __syncthreads();      // the solve is over
  if (mine) {
    T d[3], r[3];
    for (int c = 0; c < 3; ++c) d[c] = L.x[3 * tid + c];
    md_con_finish(r, v, r0, d, du, dt);
    for (int c = 0; c < 3; ++c) { pos[3 * (size_t)atom + c] = r[c]; vel[3 * (size_t)atom + c] = v[c]; }
  }
  con_count<THREADS>(counters, failed, sweeps);
}

// grad == nullptr: no kick (a pure velocity projection)
template <class T, int THREADS>
__global__ __launch_bounds__(THREADS) void k_con_kick(ConTiles<T> P, const T* __restrict__ pos, T* __restrict__ vel,
                                                      const T* __restrict__ grad, const T* __restrict__ inv_mass, Box<T> box,
                                                      T half_dt_acc, T tol_dt, int max_sweeps, double* ekin, int* counters) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const ConLds<T> L = con_carve<T>(lds_raw, P.dims, false);
  const int tid = threadIdx.x;
  const ConTile tile = con_load_lists<T, THREADS>(P, L);
  const bool mine = tid < tile.n;
  const int atom = mine ? P.atom_id[tile.a0 + tid] : 0;
  T v[3] = {T(0), T(0), T(0)}, im = T(1);
  if (mine) {
    im = inv_mass[atom];
    for (int c = 0; c < 3; ++c) { v[c] = vel[3 * (size_t)atom + c]; L.x[3 * tid + c] = pos[3 * (size_t)atom + c]; }
    if (grad) {
      T g[3];
      for (int c = 0; c < 3; ++c) g[c] = grad[3 * (size_t)atom + c];
      md_mts_kick(v, g, im, half_dt_acc);
    }
    L.im[tid] = im;
  }
  __syncthreads();
  con_vectors<T, THREADS>(L, tile.nq, box, L.s);
  __syncthreads();
  if (mine)
    for (int c = 0; c < 3; ++c) L.x[3 * tid + c] = v[c];
  __syncthreads();
  bool failed = false;
  int sweeps = 0;
  if (tid < tile.ncl) sweeps = md_con_solve_rattle(L.x, L.im, L.slot, L.d2, L.s, L.ccon[tid], L.ccon[tid + 1], tol_dt, max_sweeps, failed);
  __syncthreads();
  double ek = 0.0;
  if (mine)
    for (int c = 0; c < 3; ++c) {
      const T w = L.x[3 * tid + c];
      vel[3 * (size_t)atom + c] = w;
      ek += 0.5 * (double)w * (double)w / (double)im;
    }
  if (ekin) {      // a double sum; one atomic per workgroup
    ek = block_reduce_sum<THREADS>(ek);
    if (tid == 0) atomicAdd(ekin, ek);
  }
  con_count<THREADS>(counters, failed, sweeps);
}

// ref may be pos itself
template <class T, int THREADS>
__global__ __launch_bounds__(THREADS) void k_con_project(ConTiles<T> P, T* pos, const T* ref, const T* __restrict__ inv_mass, Box<T> box,
                                                         T tol2, int max_sweeps, int* counters) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  const ConLds<T> L = con_carve<T>(lds_raw, P.dims, true);
  const int tid = threadIdx.x;
  const ConTile tile = con_load_lists<T, THREADS>(P, L);
  const bool mine = tid < tile.n;
  const int atom = mine ? P.atom_id[tile.a0 + tid] : 0;
  T r0[3] = {T(0), T(0), T(0)};
  if (mine) {
    for (int c = 0; c < 3; ++c) { r0[c] = pos[3 * (size_t)atom + c]; L.x[3 * tid + c] = r0[c]; }
    L.im[tid] = inv_mass[atom];
  }
  __syncthreads();
  con_vectors<T, THREADS>(L, tile.nq, box, L.b);
  __syncthreads();
  if (mine)
    for (int c = 0; c < 3; ++c) L.x[3 * tid + c] = ref[3 * (size_t)atom + c];
  __syncthreads();
  con_vectors<T, THREADS>(L, tile.nq, box, L.s);
  __syncthreads();
  if (mine)
    for (int c = 0; c < 3; ++c) L.x[3 * tid + c] = T(0);
  __syncthreads();
  bool failed = false;
  int sweeps = 0;
  if (tid < tile.ncl)
    sweeps = md_con_solve_shake(L.x, L.im, L.slot, L.d2, L.s, L.b, L.ccon[tid], L.ccon[tid + 1], tol2, max_sweeps, failed);
  __syncthreads();
  if (mine)
    for (int c = 0; c < 3; ++c) pos[3 * (size_t)atom + c] = r0[c] + L.x[3 * tid + c];
  con_count<THREADS>(counters, failed, sweeps);
}

#define ADMP_CON_GO(KERNEL, LDS, ...)                                            \
  do {                                                                           \
    if (threads == 64) KERNEL<T, 64><<<P.n_tiles, 64, LDS, st>>>(__VA_ARGS__);   \
    else if (threads == 128) KERNEL<T, 128><<<P.n_tiles, 128, LDS, st>>>(__VA_ARGS__); \
    else KERNEL<T, 256><<<P.n_tiles, 256, LDS, st>>>(__VA_ARGS__);               \
  } while (0)

template <class T>
void launch_con_step(hipStream_t st, const ConTiles<T>& P, int threads, T* pos, T* vel, const T* grad, const T* inv_mass,
                     const Box<T>& box, double half_dt_acc, double dt, double c1, double c2sq_kT_acc, uint64_t seed, uint64_t step,
                     double tol, int max_sweeps, int* counters) {
  if (P.n_tiles <= 0) return;
  const size_t lds = con_lds_bytes(P.dims, sizeof(T), false);
  ADMP_CON_GO(k_con_step, lds, P, pos, vel, grad, inv_mass, box, (T)half_dt_acc, (T)(0.5 * dt), (T)dt, (T)c1, (T)c2sq_kT_acc, seed, step,
              (T)(2.0 * tol), max_sweeps, counters);
}
template <class T>
void launch_con_kick(hipStream_t st, const ConTiles<T>& P, int threads, const T* pos, T* vel, const T* grad, const T* inv_mass,
                     const Box<T>& box, double half_dt_acc, double dt, double tol, int max_sweeps, double* ekin, int* counters) {
  if (P.n_tiles <= 0) return;
  const size_t lds = con_lds_bytes(P.dims, sizeof(T), false);
  ADMP_CON_GO(k_con_kick, lds, P, pos, vel, grad, inv_mass, box, (T)half_dt_acc, (T)(tol / dt), max_sweeps, ekin, counters);
}
template <class T>
void launch_con_project(hipStream_t st, const ConTiles<T>& P, int threads, T* pos, const T* ref, const T* inv_mass, const Box<T>& box,
                        double tol, int max_sweeps, int* counters) {
  if (P.n_tiles <= 0) return;
  const size_t lds = con_lds_bytes(P.dims, sizeof(T), true);
  ADMP_CON_GO(k_con_project, lds, P, pos, ref, inv_mass, box, (T)(2.0 * tol), max_sweeps, counters);
}
#undef ADMP_CON_GO

#define INST(T)                                                                                                                  \
  template void launch_con_step<T>(hipStream_t, const ConTiles<T>&, int, T*, T*, const T*, const T*, const Box<T>&, double, double, \
                                   double, double, uint64_t, uint64_t, double, int, int*);                                          \
  template void launch_con_kick<T>(hipStream_t, const ConTiles<T>&, int, const T*, T*, const T*, const T*, const Box<T>&, double,   \
                                   double, double, int, double*, int*);                                                             \
  template void launch_con_project<T>(hipStream_t, const ConTiles<T>&, int, T*, const T*, const T*, const Box<T>&, double, int, int*);
INST(float)
INST(double)
#undef INST

}  // namespace admp
