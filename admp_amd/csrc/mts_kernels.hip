// Multiple-time-step integrator of the MD drivers (impulse r-RESPA / OpenMM's MTSLangevinIntegrator with two levels): the
// bonded terms advance by n inner BAOAB steps of length delta inside ONE kernel, between the two half kicks of the slow
// gradient that the calculators produce once per outer step Delta = n delta:
//
//   v -= (Delta/2) 1e-4 g_slow / m;   f = bonded gradient at r
//   n times:  v -= (delta/2) 1e-4 f / m;  r += (delta/2) v;  v = c1 v + sig xi;  r += (delta/2) v;  f = bonded gradient at r;
//             v -= (delta/2) 1e-4 f / m
//
// (the closing outer half kick is k_md_kick_drift with dt = 0, after the calculators).  The bonded terms of a molecule touch
// only its atoms, so a workgroup takes a tile of whole molecules (mts_plan.h), keeps their positions in LDS for the whole
// loop and reads / writes r and v in HBM once.  One lane per atom: v, f, 1/m and the noise amplitude stay in its registers.
// A force evaluation is: lanes write r to LDS | lanes walk the tile's items and write each item's contribution to its force
// slot (md_bonded_math.h: the arithmetic of k_md_bonded) | every lane sums its atom's references in the plan's order -- no
// float atomics, so r and v are bit-identical from run to run and for every tile capacity.  A capacity of up to 64 atoms is
// one wavefront (THREADS = 64): the compiler then turns the workgroup barriers into plain LDS waits.
// LDS banks: lane a keeps r at words 3 a .. 3 a + 2 (6 a .. in double) and item i its slot at 3 i ..: in single precision the
// stride 3 is odd (no conflict over 32 banks), in double the 16 lanes of a store group land on 16 different even banks
// (6 a mod 32) -- no padding is needed.  The item reads of r and the reference reads of the slots follow the topology; for
// waters (atom slots 3 m, 3 m + 1, 3 m + 2) they are strided by 9 or 18 words, again odd or 2-way at most.
#include <hip/hip_runtime.h>

#include "launch.h"
#include "md_bonded_math.h"
#include "mts_plan.h"
#include "reduce.h"

namespace admp {

template <class T, int THREADS>
__global__ __launch_bounds__(THREADS) void k_md_mts(MtsTiles<T> P, T* __restrict__ pos, T* __restrict__ vel,
                                                    const T* __restrict__ grad_slow, const T* __restrict__ inv_mass, Box<T> box,
                                                    T half_dt_acc_outer, T half_dt_acc, T half_dt, int n_inner, T c1, T c2sq_kT_acc,
                                                    uint64_t seed, uint64_t step0, double* E, T* __restrict__ grad_fast) {
  extern __shared__ __align__(16) unsigned char lds_raw[];
  // carved for the largest tile (P.dims), reals first
  T* const l_r = reinterpret_cast<T*>(lds_raw);
  T* const l_slot = l_r + 3 * P.dims.atoms;
  T* const l_bpar = l_slot + 3 * (P.dims.bonds + 2 * P.dims.angles);
  T* const l_apar = l_bpar + 2 * P.dims.bonds;
  int* const l_bidx = reinterpret_cast<int*>(l_apar + 2 * P.dims.angles);
  int* const l_aidx = l_bidx + 2 * P.dims.bonds;
  int* const l_ref0 = l_aidx + 3 * P.dims.angles;
  int* const l_ref = l_ref0 + P.dims.atoms + 1;

  const int t = blockIdx.x, tid = threadIdx.x;
  const int a0 = P.tile_atom0[t], n = P.tile_atom0[t + 1] - a0;
  const int b0 = P.tile_bond0[t], nb = P.tile_bond0[t + 1] - b0;
  const int g0 = P.tile_angle0[t], na = P.tile_angle0[t + 1] - g0;
  const int r0 = P.ref0[a0], nr = P.ref0[a0 + n] - r0;
  for (int k = tid; k < 2 * nb; k += THREADS) { l_bidx[k] = P.bond_slot[2 * (size_t)b0 + k]; l_bpar[k] = P.bond_par[2 * (size_t)b0 + k]; }
  for (int k = tid; k < 3 * na; k += THREADS) l_aidx[k] = P.angle_slot[3 * (size_t)g0 + k];
  for (int k = tid; k < 2 * na; k += THREADS) l_apar[k] = P.angle_par[2 * (size_t)g0 + k];
  for (int k = tid; k <= n; k += THREADS) l_ref0[k] = P.ref0[a0 + k] - r0;
  for (int k = tid; k < nr; k += THREADS) l_ref[k] = P.ref[(size_t)r0 + k];

  const bool mine = tid < n;      // (n <= tile capacity <= THREADS: one lane per atom)
  const int atom = mine ? P.atom_id[a0 + tid] : 0;
  T r[3] = {T(0), T(0), T(0)}, v[3] = {T(0), T(0), T(0)}, f[3], im = T(0), sig = T(0);
  if (mine) {
    im = inv_mass[atom];
    sig = m_sqrt(c2sq_kT_acc * im);
    T gs[3];
    for (int c = 0; c < 3; ++c) { r[c] = pos[3 * (size_t)atom + c]; v[c] = vel[3 * (size_t)atom + c]; gs[c] = grad_slow[3 * (size_t)atom + c]; }
    md_mts_kick(v, gs, im, half_dt_acc_outer);
  }
  const bool noisy = c1 < T(1);
  double eb = 0.0, ea = 0.0;
  for (int k = 0; k <= n_inner; ++k) {
    if (k > 0 && mine) {
      md_mts_kick(v, f, im, half_dt_acc);
      md_mts_drift(r, v, half_dt, noisy, c1, sig, seed, step0 + (uint64_t)(k - 1), (uint32_t)atom);
    }
    if (mine)
      for (int c = 0; c < 3; ++c) l_r[3 * tid + c] = r[c];
    __syncthreads();      // r (and, the first time, the item lists) are in LDS; the last pass's slots have been read
    const bool last = k == n_inner;
    for (int i = tid; i < nb; i += THREADS) {
      T g[3];
      const double e = md_bond_item(box, l_r + 3 * l_bidx[2 * i], l_r + 3 * l_bidx[2 * i + 1], l_bpar[2 * i], l_bpar[2 * i + 1], g);
      for (int c = 0; c < 3; ++c) l_slot[3 * i + c] = g[c];
      if (last) eb += e;
    }
    for (int i = tid; i < na; i += THREADS) {
      T gu[3], gv[3];
      const double e = md_angle_item(box, l_r + 3 * l_aidx[3 * i], l_r + 3 * l_aidx[3 * i + 1], l_r + 3 * l_aidx[3 * i + 2],
                                     l_apar[2 * i], l_apar[2 * i + 1], gu, gv);
      T* s = l_slot + 3 * (nb + 2 * i);
      for (int c = 0; c < 3; ++c) { s[c] = gu[c]; s[3 + c] = gv[c]; }
      if (last) ea += e;
    }
    __syncthreads();      // the slots are written; every item has read r
    f[0] = f[1] = f[2] = T(0);
    if (mine) {
      for (int q = l_ref0[tid]; q < l_ref0[tid + 1]; ++q) md_mts_add_ref(l_slot, l_ref[q], f);
      if (k > 0) md_mts_kick(v, f, im, half_dt_acc);
    }
  }
  if (mine)
    for (int c = 0; c < 3; ++c) {
      pos[3 * (size_t)atom + c] = r[c];
      vel[3 * (size_t)atom + c] = v[c];
      if (grad_fast) grad_fast[3 * (size_t)atom + c] = f[c];
    }
  if (E) {      // double sums; one atomic per word and workgroup
    eb = block_reduce_sum<THREADS>(eb);
    ea = block_reduce_sum<THREADS>(ea);
    if (tid == 0) {
      if (eb != 0.0) atomicAdd(&E[0], eb);
      if (ea != 0.0) atomicAdd(&E[1], ea);
    }
  }
}

template <class T>
void launch_md_mts(hipStream_t st, const MtsTiles<T>& P, int threads, size_t lds_bytes, T* pos, T* vel, const T* grad_slow,
                   const T* inv_mass, const Box<T>& box, double half_dt_acc_outer, double dt_outer, int n_inner, double c1,
                   double c2sq_kT_acc, uint64_t seed, uint64_t outer_step, double* E, T* grad_fast) {
  if (P.n_tiles <= 0) return;
  const T hdo = (T)half_dt_acc_outer, hdi = (T)(half_dt_acc_outer / n_inner), hd = (T)(0.5 * dt_outer / n_inner);
  const uint64_t step0 = outer_step * (uint64_t)n_inner;      // (wraps: the counter words are taken modulo 2^64)
#define ADMP_MTS_GO(TH)                                                                                                       \
  k_md_mts<T, TH><<<P.n_tiles, TH, lds_bytes, st>>>(P, pos, vel, grad_slow, inv_mass, box, hdo, hdi, hd, n_inner, (T)c1,     \
                                                    (T)c2sq_kT_acc, seed, step0, E, grad_fast)
  if (threads == 64) ADMP_MTS_GO(64);
  else if (threads == 128) ADMP_MTS_GO(128);
  else ADMP_MTS_GO(256);
#undef ADMP_MTS_GO
}
#define INST(T)                                                                                                               \
  template void launch_md_mts<T>(hipStream_t, const MtsTiles<T>&, int, size_t, T*, T*, const T*, const T*, const Box<T>&, double, \
                                 double, int, double, double, uint64_t, uint64_t, double*, T*);
INST(float)
INST(double)
#undef INST

}  // namespace admp
